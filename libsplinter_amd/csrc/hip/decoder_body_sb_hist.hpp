// No include guard: the body of k_sb_hist (decoder_kernels.hip) and k_sb_hist_b (decoder_batch.hip),
// included once by each after its own signature and prologue.  The prologue leaves logits and ws at this
// sequence's row and workspace; LEVEL, V and mask are kernel parameters.
//
// B / D: block mass (level 0) and the mass histogram of [lo, lo + 1024 w) (replicated bins, as k_sample_reg)
  __shared__ float h8[kSbBins * 8];
  const int tid = threadIdx.x;
  float M, lo, w;
  if (LEVEL == 0) {
    float m = -INFINITY;
    for (int b = 0; b < kSbBlocks; ++b) m = fmaxf(m, ws[SB_BMAX + b]);
    M = m;
    lo = M - 40.f;
    w = 40.f / kSbBins * (1.f + 1e-6f);
  } else {
    M = ws[SB_SCAL + 0];
    lo = ws[SB_SCAL + 2];
    w = ws[SB_SCAL + 3];
  }
  for (int i = tid; i < kSbBins * 8; i += kSbThreads) h8[i] = 0.f;
  __syncthreads();
  const float inv_w = 1.f / w, hi = lo + w * kSbBins;
  const int chunk = (V + kSbBlocks - 1) / kSbBlocks, b0 = blockIdx.x * chunk, b1 = min(V, b0 + chunk);
  float z = 0.f;
#pragma unroll 8
  for (int i = b0 + tid; i < b1; i += kSbThreads) {
    const float l = sb_logit(logits, mask, i);
    const float e = __expf(l - M);
    if (LEVEL == 0) z += e;
    if (l >= lo && l < hi) atomicAdd(&h8[min(kSbBins - 1, (int)((l - lo) * inv_w)) * 8 + (tid & 7)], e);
  }
  if (LEVEL == 0) {
    z = sb_reduce<kSbThreads>(z, false);
    if (tid == 0) ws[SB_BZ + blockIdx.x] = z;
  }
  __syncthreads();
  float* out = ws + SB_HIST + (long)blockIdx.x * kSbBins;
  for (int t = tid; t < kSbBins; t += kSbThreads) {
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) v += h8[t * 8 + c];
    out[t] = v;
  }
