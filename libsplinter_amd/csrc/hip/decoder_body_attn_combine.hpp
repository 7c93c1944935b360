// No include guard: the body of k_attn_combine (decoder_kernels.hip) and k_attn_combine_b
// (decoder_batch.hip), included once by each after its own signature and prologue.  The prologue leaves
// ws at this sequence's partials; out, S and hd are kernel parameters, and with DEC_SLOTS (defined by
// decoder_batch.hip) so are the slot b and its output stride ldo.
//
// out[h] = sum_j acc_j e^(m_j - M) / sum_j l_j e^(m_j - M) over the S partials of head h
  const int h = blockIdx.x;
  const float* p = ws + (long)h * S * (hd + 2);
  float M = -INFINITY;
  for (int j = 0; j < S; ++j) M = fmaxf(M, p[(long)j * (hd + 2)]);
  float den = 0.f, a = 0.f;
  const int d = threadIdx.x;
  for (int j = 0; j < S; ++j) {
    const float* pj = p + (long)j * (hd + 2);
    const float c = pj[0] == -INFINITY ? 0.f : __expf(pj[0] - M);
    den += pj[1] * c;
    if (d < hd) a += pj[2 + d] * c;
  }
#ifdef DEC_SLOTS  // out is slot 0's row: offsetting it in the prologue compiles to other instructions
  if (d < hd) out[b * ldo + (long)h * hd + d] = __builtin_bit_cast(uint16_t, (__bf16)(a / den));
#else
  if (d < hd) out[(long)h * hd + d] = __builtin_bit_cast(uint16_t, (__bf16)(a / den));
#endif
