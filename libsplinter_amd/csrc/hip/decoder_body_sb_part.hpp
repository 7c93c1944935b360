// No include guard: the body of k_sb_part (decoder_kernels.hip) and k_sb_part_b (decoder_batch.hip),
// included once by each after its own signature and prologue.  The prologue leaves logits and ws at this
// sequence's row and workspace; V, mask, temp and nucleus are kernel parameters.
//
// F: kept (tempered) mass per block; with top_p >= 1 the cut is -inf and M comes from the maxima
  float M, cut;
  if (nucleus) {
    M = ws[SB_SCAL + 0];
    cut = ws[SB_SCAL + 5];
  } else {
    float m = -INFINITY;
    for (int b = 0; b < kSbBlocks; ++b) m = fmaxf(m, ws[SB_BMAX + b]);
    M = m;
    cut = -INFINITY;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ws[SB_SCAL + 0] = M; ws[SB_SCAL + 5] = cut; }
  }
  const float it = 1.f / fmaxf(temp, 1e-6f);
  const int chunk = (V + kSbBlocks - 1) / kSbBlocks, b0 = blockIdx.x * chunk, b1 = min(V, b0 + chunk);
  float part = 0.f;
#pragma unroll 8
  for (int i = b0 + (int)threadIdx.x; i < b1; i += kSbThreads) {
    const float l = sb_logit(logits, mask, i);
    if (l >= cut) part += __expf((l - M) * it);
  }
  part = sb_reduce<kSbThreads>(part, false);
  if (threadIdx.x == 0) ws[SB_BPART + blockIdx.x] = part;
