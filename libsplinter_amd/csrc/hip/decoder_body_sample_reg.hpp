// No include guard: the body of k_sample_reg (decoder_kernels.hip) and k_sample_reg_b (decoder_batch.hip),
// included once by each after its own signature and prologue.  The prologue leaves logits (this
// sequence's row), seed, st (its state record) and host_tok; V, mask, top_p, temp, inc_pos are kernel
// parameters.
//
// top-p -> temperature -> categorical draw on the device (the reference's llama sampler chain,
// splainference.cpp:272-279): the nucleus is the smallest set of the most probable tokens whose
// probability reaches top_p, found as a logit threshold (no sort); the kept logits are divided by
// temp and one token is drawn by an inclusive scan over the threads' masses.  Writes state.token
// (and pos += inc_pos, step += 1) and the token to `host_tok` (pinned, may be null).
// One 1024-thread workgroup with the vocabulary held in registers (V <= 1024 * kSampRegs): thread t
// owns tokens t + 1024 k and every pass reads them from VGPRs; the categorical draw walks the
// threads' masses in that fixed order, an equally valid order of the same distribution.
// Nucleus threshold: the largest logit cut whose kept mass reaches top_p, found by two levels of a
// 1024-bin mass histogram over the current interval [lo, hi) (LDS float atomics), each level keeping
// the bin where the suffix mass crosses top_p * Z: a resolution of 40 / 2^20 (a few float ulps of a
// logit) instead of one pass per bisection step.  Every bin has 8 copies, picked by lane & 7: flat
// logits (a random-init model: every logit in one or two bins) put a wave's 64 same-address LDS
// atomics into one 64-way conflict; the copies cut it to 8-way (profiles/r2_decode_q4.md).
// Measured and removed: the same sampler reading the logits from global memory in every pass
// (k_sample, any V) and this one at 32 registers per thread (V <= 32768), both behind dec_sample,
// which only a test called: 255-275 us at V = 128256 and 61-65 us at V = 32000 against 53 and
// 47 us for the k_sb_* chain (profiles/r2_decode_q4.md).
  __shared__ float sh[kSampThreads / 64];
  __shared__ float scan[kSampThreads];
  __shared__ float hist[kSampThreads];
  __shared__ float hist8[kSampThreads * 8];
  __shared__ int jstar, pick;
  const int tid = threadIdx.x;
  constexpr int R = kSampRegs;
  float v[R];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int i = tid + k * kSampThreads;
    v[k] = (i < V && !(mask && !mask[i])) ? logits[i] : -INFINITY;
    m = fmaxf(m, v[k]);
  }
  const float M = block_reduce(m, sh, true);
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < R; ++k) z += __expf(v[k] - M);
  const float Z = block_reduce(z, sh, false);
  float lo = M - 40.f;  // nucleus cut: two levels of the replicated 1024-bin histogram; mass below M - 40 is < V e^-40
  if (top_p < 1.f) {
    const float target = top_p * Z;
    float w = 40.f / kSampThreads * (1.f + 1e-6f);
    float above = 0.f;
    for (int level = 0; level < 2; ++level) {
#pragma unroll
      for (int c = 0; c < 8; ++c) hist8[c * kSampThreads + tid] = 0.f;
      if (tid == 0) jstar = 0;
      __syncthreads();
      const float inv_w = 1.f / w, hi = lo + w * kSampThreads;
#pragma unroll
      for (int k = 0; k < R; ++k)
        if (v[k] >= lo && v[k] < hi)
          atomicAdd(&hist8[min(kSampThreads - 1, (int)((v[k] - lo) * inv_w)) * 8 + (tid & 7)], __expf(v[k] - M));
      __syncthreads();
      float h = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) h += hist8[tid * 8 + c];
      hist[tid] = h;
      __syncthreads();
      for (int off = 1; off < kSampThreads; off <<= 1) {
        const float x = tid + off < kSampThreads ? hist[tid + off] : 0.f;
        __syncthreads();
        hist[tid] += x;
        __syncthreads();
      }
      if (hist[tid] + above >= target) atomicMax(&jstar, tid);
      __syncthreads();
      const int j = jstar;
      above += j + 1 < kSampThreads ? hist[j + 1] : 0.f;
      lo += j * w;
      w *= 1.f / kSampThreads;
      __syncthreads();
    }
  } else {
    lo = -INFINITY;
  }
  const float cut = lo;
  const float it = 1.f / fmaxf(temp, 1e-6f);
  float part = 0.f;
#pragma unroll
  for (int k = 0; k < R; ++k)
    if (v[k] >= cut) part += __expf((v[k] - M) * it);
  scan[tid] = part;
  if (tid == 0) pick = 0x7fffffff;
  __syncthreads();
  for (int off = 1; off < kSampThreads; off <<= 1) {
    const float x = tid >= off ? scan[tid - off] : 0.f;
    __syncthreads();
    scan[tid] += x;
    __syncthreads();
  }
  const float total = scan[kSampThreads - 1];
  const float u = (float)(uniform01(seed, (uint64_t)st[ST_STEP]) * total);
  const float before = tid ? scan[tid - 1] : 0.f;
  if (u >= before && u < scan[tid] && part > 0.f) {
    float run = before;
    int sel = -1;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (sel < 0 && v[k] >= cut) {
        run += __expf((v[k] - M) * it);
        if (u < run) sel = tid + k * kSampThreads;
      }
    }
    if (sel < 0)  // rounding at the thread's upper edge: its last kept token
#pragma unroll
      for (int k = 0; k < R; ++k)
        if (v[k] >= cut) sel = tid + k * kSampThreads;
    atomicMin(&pick, sel);
  }
  __syncthreads();
  if (pick == 0x7fffffff) {  // u landed on a rounding gap at the very top: the most probable token
#pragma unroll
    for (int k = 0; k < R; ++k)
      if (v[k] == M) atomicMin(&pick, tid + k * kSampThreads);
    __syncthreads();
  }
  if (tid == 0) state_commit(st, pick, inc_pos, host_tok);
