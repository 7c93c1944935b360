// No include guard: the body of k_sb_max (decoder_kernels.hip) and k_sb_max_b (decoder_batch.hip),
// included once by each after its own signature and prologue.  The prologue leaves logits and ws at this
// sequence's row and workspace; V and mask are kernel parameters.
//
// A: block max and its first index
  const int chunk = (V + kSbBlocks - 1) / kSbBlocks, b0 = blockIdx.x * chunk, b1 = min(V, b0 + chunk);
  float m = -INFINITY;
  int mi = 0x7fffffff;
#pragma unroll 8
  for (int i = b0 + (int)threadIdx.x; i < b1; i += kSbThreads) {
    const float l = sb_logit(logits, mask, i);
    if (l > m) { m = l; mi = i; }
  }
  const float M = sb_reduce<kSbThreads>(m, true);
  __shared__ int first;
  if (threadIdx.x == 0) first = 0x7fffffff;
  __syncthreads();
  if (m == M) atomicMin(&first, mi);
  __syncthreads();
  if (threadIdx.x == 0) {
    ws[SB_BMAX + blockIdx.x] = M;
    ws[SB_BIDX + blockIdx.x] = __int_as_float(first);
  }
