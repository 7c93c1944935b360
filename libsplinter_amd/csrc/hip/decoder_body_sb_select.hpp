// No include guard: the body of k_sb_select (decoder_kernels.hip) and k_sb_select_b (decoder_batch.hip),
// included once by each after its own signature and prologue.  The prologue leaves ws at this sequence's
// workspace; LEVEL and top_p are kernel parameters.
//
// C / E: one workgroup of 1024 threads sums the block histograms, finds the bin where the suffix
// mass crosses top_p Z and narrows [lo, lo + 1024 w) to it (level 1: the cut)
  __shared__ float hs[kSbBins];
  __shared__ int jstar;
  const int tid = threadIdx.x;
  float M, Z, lo, w, above;
  if (LEVEL == 0) {
    float m = -INFINITY;
    for (int b = 0; b < kSbBlocks; ++b) m = fmaxf(m, ws[SB_BMAX + b]);
    M = m;
    Z = 0.f;
    for (int b = 0; b < kSbBlocks; ++b) Z += ws[SB_BZ + b];
    lo = M - 40.f;
    w = 40.f / kSbBins * (1.f + 1e-6f);
    above = 0.f;
  } else {
    M = ws[SB_SCAL + 0]; Z = ws[SB_SCAL + 1]; lo = ws[SB_SCAL + 2]; w = ws[SB_SCAL + 3]; above = ws[SB_SCAL + 4];
  }
  float h = 0.f;
  for (int b = 0; b < kSbBlocks; ++b) h += ws[SB_HIST + (long)b * kSbBins + tid];
  hs[tid] = h;
  if (tid == 0) jstar = 0;
  __syncthreads();
  for (int off = 1; off < kSbBins; off <<= 1) {  // suffix sums
    const float x = tid + off < kSbBins ? hs[tid + off] : 0.f;
    __syncthreads();
    hs[tid] += x;
    __syncthreads();
  }
  if (hs[tid] + above >= top_p * Z) atomicMax(&jstar, tid);
  __syncthreads();
  if (tid == 0) {
    const int j = jstar;
    ws[SB_SCAL + 0] = M;
    ws[SB_SCAL + 1] = Z;
    ws[SB_SCAL + 4] = above + (j + 1 < kSbBins ? hs[j + 1] : 0.f);
    ws[SB_SCAL + 2] = lo + j * w;
    ws[SB_SCAL + 3] = w * (1.f / kSbBins);
    ws[SB_SCAL + 5] = lo + j * w;  // the cut after the last level
  }
