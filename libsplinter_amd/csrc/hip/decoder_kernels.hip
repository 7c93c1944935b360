// decoder_kernels.hip — the non-GEMM elementwise kernels of the completion
// daemon's llama-architecture decoder (K18 of SURVEY §2.10; reference
// splainference.cpp:272-330 runs these inside llama_decode).
//
//   dec_rmsnorm   y = x * rsqrt(mean(x^2) + eps) * w      bf16 in/out, fp32 w
//   dec_rope      llama "normal" RoPE (adjacent pairs) applied IN PLACE to the
//                 q and k column ranges of the fused QKV GEMM output
//   dec_attn_decode  single-token GQA attention over the KV cache (split-L over
//                 16 waves, online softmax, LDS merge) — the per-token decode path
//
//   dec_gemv      M = 1 projections of the decode step (optionally with the RMSNorm of x
//                 fused in): weight rows streamed once with 16-B loads, 4 rows per wave in flight
//   dec_embed_tok / dec_rope_kv / dec_sample_ws   (their forms over up to 16 sequence slots: decoder_batch.hip)
//                 the rest of a decode step, driven by a device-resident state {pos, token,
//                 step} so a whole step (all layers + sampling) can be captured once in a HIP
//                 graph and replayed per token with no host arguments changing
//
// Both are HBM-bound row kernels: one 64-lane wave per row, 16-B (8 x bf16)
// vector accesses, statistics reduced with __shfl_xor over the full wavefront.
// The prefill projections run on the MFMA GEMM (gemm_bf16.hip).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>

#include "decoder_common.hpp"
#include "decoder_gemv.hpp"

namespace {

// One wave per row, 4 rows per 256-thread block.  Rows of up to 64 x 8 x 4 =
// 2048 elements stay in registers (single HBM read); wider rows re-read their
// remaining chunks in the second pass (the row is cache-resident by then).
constexpr int kRegChunks = 4;

__global__ __launch_bounds__(256) void k_rmsnorm(const uint16_t* __restrict__ x, long ldx, const float* __restrict__ w,
                                                 long T, int d, float eps, uint16_t* __restrict__ out, long ldo) {
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= T) return;
  const int nch = d >> 3;
  const uint16_t* src = x + row * ldx;
  float v[kRegChunks][8];
  float ss = 0.f;
#pragma unroll
  for (int r = 0; r < kRegChunks; ++r) {
    const int c = lane + r * 64;
    if (c < nch) {
      unpack8(*(const uint4*)(src + c * 8), v[r]);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss += v[r][e] * v[r][e];
    }
  }
  for (int c = lane + kRegChunks * 64; c < nch; c += 64) {
    float t[8];
    unpack8(*(const uint4*)(src + c * 8), t);
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += t[e] * t[e];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float rs = rsqrtf(ss / (float)d + eps);
  uint16_t* dst = out + row * ldo;
#pragma unroll
  for (int r = 0; r < kRegChunks; ++r) {
    const int c = lane + r * 64;
    if (c < nch) {
      const float4 w0 = *(const float4*)(w + c * 8), w1 = *(const float4*)(w + c * 8 + 4);
      const float ww[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = v[r][e] * rs * ww[e];
      *(uint4*)(dst + c * 8) = pack8(o);
    }
  }
  for (int c = lane + kRegChunks * 64; c < nch; c += 64) {
    float t[8], o[8];
    unpack8(*(const uint4*)(src + c * 8), t);
    const float4 w0 = *(const float4*)(w + c * 8), w1 = *(const float4*)(w + c * 8 + 4);
    const float ww[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = t[e] * rs * ww[e];
    *(uint4*)(dst + c * 8) = pack8(o);
  }
}

// In-place RoPE over columns [0, ncols) of each row (q heads then k heads, each hd wide):
// pair (2i, 2i+1) of a head rotates by angle pos * base^(-2i/hd), read from the fp32
// cos/sin tables [n_ctx, hd/2].  One thread per 8 elements (4 pairs).
__global__ __launch_bounds__(256) void k_rope(uint16_t* __restrict__ qkv, long ld, long T, int ncols, int hd,
                                              int pos0, const float* __restrict__ cs, const float* __restrict__ sn) {
  const int per_row = ncols >> 3;
  const long total = T * per_row;
  const int half = hd >> 1;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long row = q / per_row;
    const int col = (int)(q - row * per_row) * 8;
    const int i0 = (col % hd) >> 1;  // first pair index inside the head
    const long p = pos0 + row;
    uint16_t* ptr = qkv + row * ld + col;
    float f[8], o[8];
    unpack8(*(const uint4*)ptr, f);
    const float4 c4 = *(const float4*)(cs + p * half + i0), s4 = *(const float4*)(sn + p * half + i0);
    const float c[4] = {c4.x, c4.y, c4.z, c4.w}, s[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = f[2 * e], b = f[2 * e + 1];
      o[2 * e] = a * c[e] - b * s[e];
      o[2 * e + 1] = a * s[e] + b * c[e];
    }
    *(uint4*)ptr = pack8(o);
  }
}

// Decode attention and the sampler: each kernel here is its signature, the prologue that names this
// generation's operands, and a body that is one text for it and for its slot-indexed form in
// decoder_batch.hip (decoder_body_*.hpp, where the kernels are described).  The bodies are included, not
// called: a shared function moves the register allocation (profiles/decoder_prune/README.md), the same
// tokens do not (profiles/decoder_share/README.md).

// one 1024-thread workgroup per query head, its 16 waves over interleaved 64-key chunks
template <int DPL>
__global__ __launch_bounds__(kDecWaves * 64) void k_attn_decode(const uint16_t* __restrict__ q, const uint16_t* __restrict__ K,
                                                     const uint16_t* __restrict__ V, long ldkv, int L, int grp,
                                                     int hd, float scale, uint16_t* __restrict__ out,
                                                     const int32_t* __restrict__ st) {
  if (st) L = st[0] + 1;  // graph-captured decode step: the cache length lives on the device
#include "decoder_body_attn_walk.hpp"
}

// caches of at most kSmallL keys: one workgroup per KV head serves its G query heads; SPLIT: one split of
// the flash-decoding form
template <int D, int G, bool SPLIT = false>
__global__ __launch_bounds__(256) void k_attn_decode_g(const uint16_t* __restrict__ q, const uint16_t* __restrict__ K,
                                                       const uint16_t* __restrict__ V, long ldkv, int L, float scale,
                                                       uint16_t* __restrict__ out, const int32_t* __restrict__ st,
                                                       float* __restrict__ ws = nullptr) {
  if (st) L = st[0] + 1;
#include "decoder_body_attn_g.hpp"
}

// split-L (flash-decoding) for long caches: grid (H / G, S), partials to ws for k_attn_combine
template <int DPL, int G>
__global__ __launch_bounds__(kSplitWaves * 64) void k_attn_decode_split(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ K, const uint16_t* __restrict__ V, long ldkv, int L,
    int grp, float scale, float* __restrict__ ws, const int32_t* __restrict__ st) {
  if (st) L = st[0] + 1;
#include "decoder_body_attn_split.hpp"
}

// merges the S partials of head h
__global__ void k_attn_combine(const float* __restrict__ ws, int S, int hd, uint16_t* __restrict__ out) {
#include "decoder_body_attn_combine.hpp"
}

// ------------------------------------------------------------------ decode step --
// The device state record {pos, token, step} and the wave reductions: decoder_common.hpp.

// The one-token GEMV: geometry, row map, store epilogue and the Q4G32 / Q8G32 layout are in decoder_gemv.hpp,
// the loop text in decoder_body_gemv.hpp / decoder_body_gemv_q4.hpp (shared with decoder_moe.hip).
template <int MODE, bool RMS>
__global__ __launch_bounds__(256) void k_gemv(const uint16_t* __restrict__ x, const float* __restrict__ rw, float eps,
                                              const uint16_t* __restrict__ W, int K, int nout,
                                              const uint16_t* res, void* out) {
#include "decoder_body_gemv.hpp"
}

// y[n] = x . W[n, :] with W in Q4G32.  Structure of k_gemv: x (optionally RMS-normalised) staged
// in LDS as fp32 together with its 32-group sums (the m term: sum_k (d q_k + m) x_k =
// d sum_k q_k x_k + m sum_k x_k); each wave owns kGemvRows weight rows, each lane one 32-k group per row
// and iteration (one 16-B load of nibbles + one scale word per row).
// Measured and removed: 8 rows per wave (SPL_Q4_ROWS=8: 222 VGPRs, 2 waves per SIMD), 0.788 against
// 0.713 ms/token (profiles/r2_decode_q4.md, r2_q4_rows_ab.jsonl).
// BITS 4: Q4G32 nibbles (16 B per group); BITS 8: Q8G32 bytes (32 B per group, the same (d, m)
// words: w = d * u + m with u in 0..255) -- the >4-bit GGUF tensors (Q6_K / Q5_x / Q8_0 / F16) of a
// mostly-4-bit file keep >= 6 bits instead of being re-gridded to 4
template <int MODE, bool RMS, int BITS>
__global__ __launch_bounds__(256) void k_gemv_q4(const uint16_t* __restrict__ x, const float* __restrict__ rw,
                                                 float eps, const uint8_t* __restrict__ Wq,
                                                 const uint32_t* __restrict__ Wsm, int K, int nout,
                                                 const uint16_t* res, void* out) {
#include "decoder_body_gemv_q4.hpp"
}

// bf16 W [N, K] -> Q4G32 (one thread per 32-weight group): affine min/max grid, d and m rounded
// to bf16 first and the nibbles chosen against the rounded pair
__global__ void k_q4_quant(const uint16_t* __restrict__ W, long groups, int ng, uint8_t* __restrict__ Wq,
                           uint32_t* __restrict__ Wsm) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= groups) return;
  float v[kQ4Group];
  const uint4* src = (const uint4*)(W + i * kQ4Group);
#pragma unroll
  for (int c = 0; c < 4; ++c) unpack8(src[c], v + c * 8);
  float lo = v[0], hi = v[0];
#pragma unroll
  for (int e = 1; e < kQ4Group; ++e) { lo = fminf(lo, v[e]); hi = fmaxf(hi, v[e]); }
  const float m = (float)(__bf16)lo;
  float d = (float)(__bf16)((hi - m) / 15.f);
  if (!(d > 0.f)) d = 0.f;
  const float inv = d > 0.f ? 1.f / d : 0.f;
  uint32_t packed[4] = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < kQ4Group; ++e) {
    int q = (int)rintf((v[e] - m) * inv);
    q = q < 0 ? 0 : (q > 15 ? 15 : q);
    packed[e >> 3] |= (uint32_t)q << (4 * (e & 7));
  }
  *(uint4*)(Wq + i * 16) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
  Wsm[i] = pk2(d, m);
  (void)ng;
}

// Q4G32 -> bf16 W [N, K] (prefill: the MFMA GEMM consumes one dequantised matrix at a time)
__global__ void k_q4_dequant(const uint8_t* __restrict__ Wq, const uint32_t* __restrict__ Wsm, long groups,
                             uint16_t* __restrict__ W) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= groups) return;
  const uint4 q = *(const uint4*)(Wq + i * 16);
  const uint32_t sm = Wsm[i];
  const float d = bf2f(sm & 0xffff), m = bf2f(sm >> 16);
  const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
  uint4* dst = (uint4*)(W + i * kQ4Group);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = fmaf(d, (float)((qw[c] >> (4 * e)) & 15u), m);
    dst[c] = pack8(f);
  }
}

__device__ __forceinline__ float bf16_floor(float x) {
  uint32_t u = __float_as_uint(x) & 0xFFFF0000u;
  if (__uint_as_float(u) > x) u += 0x10000u;  // negative: truncation went toward zero, one ulp down
  return __uint_as_float(u);
}
__device__ __forceinline__ float bf16_ceil(float x) {
  uint32_t u = __float_as_uint(x) & 0xFFFF0000u;
  if (__uint_as_float(u) < x) u += 0x10000u;  // positive: one ulp up
  return __uint_as_float(u);
}

// bf16 W [N, K] <-> Q8G32 (one thread per 32-weight group): affine 255-step grid over the group's
// [min, max], (d, m) rounded to bf16 outward first and the bytes chosen against the rounded pair
__global__ void k_q8_quant(const uint16_t* __restrict__ W, long groups, uint8_t* __restrict__ Wq,
                           uint32_t* __restrict__ Wsm) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= groups) return;
  float v[kQ4Group];
  const uint4* src = (const uint4*)(W + i * kQ4Group);
#pragma unroll
  for (int c = 0; c < 4; ++c) unpack8(src[c], v + c * 8);
  float lo = v[0], hi = v[0];
#pragma unroll
  for (int e = 1; e < kQ4Group; ++e) { lo = fminf(lo, v[e]); hi = fmaxf(hi, v[e]); }
  // m rounded DOWN and d UP to bf16, so the 255-step grid still spans [lo, hi]: at 8 bits a
  // round-to-nearest m would move the grid by up to |m| 2^-9, most of a step
  const float m = bf16_floor(lo);
  float d = bf16_ceil((hi - m) / 255.f);
  if (!(d > 0.f)) d = 0.f;
  const float inv = d > 0.f ? 1.f / d : 0.f;
  uint32_t packed[8] = {};
#pragma unroll
  for (int e = 0; e < kQ4Group; ++e) {
    int q = (int)rintf((v[e] - m) * inv);
    q = q < 0 ? 0 : (q > 255 ? 255 : q);
    packed[e >> 2] |= (uint32_t)q << (8 * (e & 3));
  }
  *(uint4*)(Wq + i * 32) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
  *(uint4*)(Wq + i * 32 + 16) = make_uint4(packed[4], packed[5], packed[6], packed[7]);
  Wsm[i] = pk2(d, m);
}

__global__ void k_q8_dequant(const uint8_t* __restrict__ Wq, const uint32_t* __restrict__ Wsm, long groups,
                             uint16_t* __restrict__ W) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= groups) return;
  const uint4 a = *(const uint4*)(Wq + i * 32), b = *(const uint4*)(Wq + i * 32 + 16);
  const uint32_t sm = Wsm[i];
  const float d = bf2f(sm & 0xffff), m = bf2f(sm >> 16);
  const uint32_t qw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint4* dst = (uint4*)(W + i * kQ4Group);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = fmaf(d, (float)((qw[2 * c + (e >> 2)] >> (8 * (e & 3))) & 255u), m);
    dst[c] = pack8(f);
  }
}

// x = emb[state.token]
__global__ void k_embed_tok(const uint16_t* __restrict__ emb, int d, const int32_t* __restrict__ st,
                            uint16_t* __restrict__ x) {
  const long t = st[ST_TOK];
  for (int c = threadIdx.x; c < d / 8; c += blockDim.x) *(uint4*)(x + c * 8) = *(const uint4*)(emb + t * d + c * 8);
}

// RoPE of the step's q (in place) and k at position state.pos, k / v appended to the layer's KV cache
__global__ void k_rope_kv(uint16_t* __restrict__ qkv, int H, int KVH, int hd, const float* __restrict__ cs,
                          const float* __restrict__ sn, const int32_t* __restrict__ st, uint16_t* __restrict__ kc,
                          uint16_t* __restrict__ vc, long ldkv) {
  const long p = st[ST_POS];
#include "decoder_body_rope_kv.hpp"
}

// top-p -> temperature -> categorical draw on the device, the vocabulary in registers (V <= 1024 * kSampRegs)
__global__ __launch_bounds__(kSampThreads) void k_sample_reg(const float* __restrict__ logits, int V,
                                                             const uint8_t* __restrict__ mask, float top_p,
                                                             float temp, uint64_t seed, int32_t* __restrict__ st,
                                                             int inc_pos, int32_t* host_tok) {
#include "decoder_body_sample_reg.hpp"
}

// ------------------------------------------------------------------ multi-block sampler --
// The same sampler spread over kSbBlocks workgroups (one contiguous vocabulary slice each), as a
// chain of small kernels: a single workgroup is bound by one CU (61 us at V 32000, 255-275 us at
// V 128256).  The workspace (floats, caller-owned so the chain can be graph-captured) is laid out in
// decoder_common.hpp.

// A .. G of the chain: decoder_body_sb_*.hpp
__global__ __launch_bounds__(kSbThreads) void k_sb_max(const float* __restrict__ logits, int V,
                                                       const uint8_t* __restrict__ mask, float* __restrict__ ws) {
#include "decoder_body_sb_max.hpp"
}

template <int LEVEL>
__global__ __launch_bounds__(kSbThreads) void k_sb_hist(const float* __restrict__ logits, int V,
                                                        const uint8_t* __restrict__ mask, float* __restrict__ ws) {
#include "decoder_body_sb_hist.hpp"
}

template <int LEVEL>
__global__ __launch_bounds__(kSbBins) void k_sb_select(float top_p, float* __restrict__ ws) {
#include "decoder_body_sb_select.hpp"
}

__global__ __launch_bounds__(kSbThreads) void k_sb_part(const float* __restrict__ logits, int V,
                                                        const uint8_t* __restrict__ mask, float temp, int nucleus,
                                                        float* __restrict__ ws) {
#include "decoder_body_sb_part.hpp"
}

__global__ __launch_bounds__(kSbBins) void k_sb_draw(const float* __restrict__ logits, int V,
                                                     const uint8_t* __restrict__ mask, float temp, uint64_t seed,
                                                     const float* __restrict__ ws, int32_t* __restrict__ st,
                                                     int inc_pos, int32_t* host_tok) {
#include "decoder_body_sb_draw.hpp"
}

// ------------------------------------------------------- prefill attention over the KV cache --
// Causal grouped-query attention of a prompt chunk of n tokens at absolute positions pos0 ..
// pos0+n-1 against the KV cache rows 0 .. pos0+n-1 (the chunk's own k/v already appended): the
// first prompt (pos0 = 0) and every continuation (a new turn over a live cache) alike, for head
// dims 64 and 128 (llama 1B-class and 7B-class).  One 256-thread workgroup = 128 query rows of
// one q head, 4 waves x 2 16-row q-blocks; per 64-key tile (LDS double buffer, register-staged
// one tile ahead):
//   S^T = K Q^T    mfma_f32_16x16x32_bf16 with the K rows as the A operand, so one query's
//                  scores sit in one lane column and the softmax statistics reduce in-lane plus
//                  two permlane swaps;
//   O^T += V^T P^T the rounded probabilities are the B operand as they lie; V^T fragments come
//                  from the row-major V tile through ds_read_b64_tr_b16.
// The K tile's 16-B chunks are XOR-swizzled by the key (mod HD/8 chunks) so a 16-lane group's
// b128 reads of 16 key rows cover all 64 banks; V chunks swap bits 1..2 by key pair for the
// transposing reads.  Grid: nqb * heads blocks through the bijective XCD remap, so the q-blocks
// of one head (which stream the same K/V) share one XCD's L2.
typedef __bf16 pa_bf16x8 __attribute__((ext_vector_type(8)));
typedef float pa_f32x4 __attribute__((ext_vector_type(4)));
typedef float pa_f32x2 __attribute__((ext_vector_type(2)));
typedef short pa_v4i16 __attribute__((ext_vector_type(4)));
typedef short pa_v8i16 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) pa_v4i16 pa_lds_v4i16;

__device__ __forceinline__ float pa_xg_max(float x) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(q[0]), __uint_as_float(q[1]));
}
__device__ __forceinline__ float pa_xg_sum(float x) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(q[0]) + __uint_as_float(q[1]);
}

// SEG: empty for one prompt chunk (dec_attn_prefill_kv), or one PrefillSegs table by value
// (dec_attn_prefill_kv_seg): the grid is then the sum over the segments of q-blocks x heads, ordered
// segment, head, q-block, so the q-blocks of one (segment, head) are neighbours under the XCD remap; a
// block finds its segment, takes n / pos0 from it and moves the q / out / cache bases to the segment's rows
// and slot.  q-blocks start at the segment's first row, so everything below is the single-chunk kernel on
// that segment alone.  The parameter pack keeps the signature, and with it the code, of the two
// single-chunk instantiations as they were (profiles/prefill_batch/README.md).
template <int HD, class... SEG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_prefill_attn(const uint16_t* __restrict__ qg, long ldq,
                                                      const uint16_t* __restrict__ kc,
                                                      const uint16_t* __restrict__ vc, long ldkv, int n, int pos0,
                                                      int heads, int kv_heads, float scale_log2,
                                                      uint16_t* __restrict__ out, long ldo, SEG... seg) {
  static_assert(sizeof...(SEG) <= 1, "at most one segment table");
  constexpr int KT = HD == 128 ? 32 : 64, RB = HD * 2, NCH = HD / 8, NKK = HD / 32, NDB = HD / 16, NL = KT * NCH / 256;
  __shared__ __attribute__((aligned(16))) char lds[2][2][KT * RB];  // [buf][K | V][key * RB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int nwg = gridDim.x, orig = blockIdx.x, q8 = nwg / 8, r8 = nwg % 8, xcd = orig % 8;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
  int head, qstart;
  if constexpr (sizeof...(SEG) == 0) {
    const int nqb = nwg / heads;
    head = lid / nqb;
    qstart = (lid - head * nqb) * 128;
  } else {
    const PrefillSegs& tb = (seg, ...);
    int rem = lid, si = 0;
#pragma unroll
    for (int j = 0; j < kMaxSegs - 1; ++j) {  // the launcher sized the grid: lid falls inside the table
      const int w = ((tb.n[j] + 127) >> 7) * heads;
      if (j == si && j + 1 < tb.nseg && rem >= w) {
        rem -= w;
        si = j + 1;
      }
    }
    const PrefillSeg sg = prefill_seg_at(tb, si);
    const int nqb = (sg.n + 127) >> 7;
    head = rem / nqb;
    qstart = (rem - head * nqb) * 128;
    n = sg.n;
    pos0 = sg.pos0;
    qg += (long)sg.row0 * ldq;
    out += (long)sg.row0 * ldo;
    kc += (long)sg.slot * tb.seq_stride;
    vc += (long)sg.slot * tb.seq_stride;
  }
  const int kvhead = head / (heads / kv_heads);
  const long lenk = (long)pos0 + n;
  auto ksw = [](int key, int c) { return c ^ (key & (NCH - 1)); };
  auto vsw = [](int key, int c) { return c ^ (((key >> 1) & 3) << 1); };

  pa_bf16x8 qf[2][NKK];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int qrow = qstart + wave * 32 + qb * 16 + li;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
      qf[qb][kk] = qrow < n ? *(const pa_bf16x8*)(qg + (long)qrow * ldq + head * HD + kk * 32 + g * 8) : pa_bf16x8{};
  }
  pa_f32x4 o[NDB][2];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) o[db][qb] = pa_f32x4{0.f, 0.f, 0.f, 0.f};
  float m[2] = {-1e30f, -1e30f}, l[2] = {0.f, 0.f};

  uint4 rk[NL], rv[NL];
  const uint16_t* kp = kc + (long)kvhead * HD;
  const uint16_t* vp = vc + (long)kvhead * HD;
  auto gload = [&](long k0) {
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int c = tid + it * 256, key = c / NCH, ch = c % NCH;
      if (k0 + key < lenk) {
        rk[it] = *(const uint4*)(kp + (k0 + key) * ldkv + ch * 8);
        rv[it] = *(const uint4*)(vp + (k0 + key) * ldkv + ch * 8);
      } else {
        rk[it] = make_uint4(0, 0, 0, 0);
        rv[it] = make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto lwrite = [&](int buf) {
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int c = tid + it * 256, key = c / NCH, ch = c % NCH;
      *(uint4*)(lds[buf][0] + key * RB + (ksw(key, ch) << 4)) = rk[it];
      *(uint4*)(lds[buf][1] + key * RB + (vsw(key, ch) << 4)) = rv[it];
    }
  };

  // causal: the block's last query (absolute pos0 + qstart + 127) bounds the key tiles
  const int ntiles = (int)min((lenk + KT - 1) / KT, ((long)pos0 + qstart + 128 + KT - 1) / KT);
  gload(0);
  lwrite(0);
  __syncthreads();
  const int tq = li >> 2, tp = li & 3;
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    const long k0 = (long)t * KT;
    if (t + 1 < ntiles) gload(k0 + KT);
    const char* Ks = lds[buf][0];
    const char* Vs = lds[buf][1];
    pa_f32x4 s[KT / 16][2];
#pragma unroll
    for (int kb = 0; kb < KT / 16; ++kb) {
      const int row = kb * 16 + li;
      pa_bf16x8 kf[NKK];
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) kf[kk] = *(const pa_bf16x8*)(Ks + row * RB + (ksw(row, kk * 4 + g) << 4));
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        s[kb][qb] = pa_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk)
          s[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kk], qf[qb][kk], s[kb][qb], 0, 0, 0);
      }
    }
    // online softmax with the deferred rescale (max moves only past a 2^8 margin); keys after a
    // query's absolute position are masked on the diagonal tiles, which also covers the keys
    // past the cache length for every stored row
    constexpr float kThr = 8.f;
    const bool diag = k0 + KT - 1 > (long)pos0 + qstart + wave * 32;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      if (diag) {
        const long qabs = (long)pos0 + qstart + wave * 32 + qb * 16 + li;
#pragma unroll
        for (int kb = 0; kb < KT / 16; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (k0 + kb * 16 + 4 * g + r > qabs) s[kb][qb][r] = -1e30f;
      }
      float mx = -1e30f;
#pragma unroll
      for (int kb = 0; kb < KT / 16; ++kb)
        mx = fmaxf(fmaxf(mx, fmaxf(s[kb][qb][0], s[kb][qb][1])), fmaxf(s[kb][qb][2], s[kb][qb][3]));
      const float mxs = pa_xg_max(mx) * scale_log2;
      if (!__all(mxs - m[qb] <= kThr)) {
        const float mn = fmaxf(m[qb], mxs);
        const float alpha = __builtin_amdgcn_exp2f(m[qb] - mn);
        m[qb] = mn;
        l[qb] *= alpha;
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db][qb] *= alpha;
      }
      const pa_f32x2 sc2 = {scale_log2, scale_log2}, nm2 = {-m[qb], -m[qb]};
      pa_f32x2 acc2 = {0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KT / 16; ++kb)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          pa_f32x2 x = {s[kb][qb][2 * h], s[kb][qb][2 * h + 1]};
          x = x * sc2 + nm2;
          x.x = __builtin_amdgcn_exp2f(x.x);
          x.y = __builtin_amdgcn_exp2f(x.y);
          s[kb][qb][2 * h] = x.x;
          s[kb][qb][2 * h + 1] = x.y;
          acc2 += x;
        }
      l[qb] += pa_xg_sum(acc2.x + acc2.y);
    }
#pragma unroll
    for (int st = 0; st < KT / 32; ++st) {
      pa_bf16x8 pf[2];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pf[qb][j] = (__bf16)s[2 * st][qb][j];
          pf[qb][4 + j] = (__bf16)s[2 * st + 1][qb][j];
        }
      const int row1 = st * 32 + 4 * g + tq, row2 = row1 + 16;
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const int ch = db * 2 + (tp >> 1);
        const pa_v4i16 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (pa_lds_v4i16*)(Vs + row1 * RB + (vsw(row1, ch) << 4) + 8 * (tp & 1)));
        const pa_v4i16 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (pa_lds_v4i16*)(Vs + row2 * RB + (vsw(row2, ch) << 4) + 8 * (tp & 1)));
        const pa_bf16x8 vf = __builtin_bit_cast(pa_bf16x8, (pa_v8i16)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
          o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qb], o[db][qb], 0, 0, 0);
      }
    }
    if (t + 1 < ntiles) lwrite(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int qrow = qstart + wave * 32 + qb * 16 + li;
    if (qrow >= n) continue;
    const float inv = 1.f / l[qb];
    uint16_t* dst = out + (long)qrow * ldo + head * HD + 4 * g;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      uint2 w;
      w.x = pk2(o[db][qb][0] * inv, o[db][qb][1] * inv);
      w.y = pk2(o[db][qb][2] * inv, o[db][qb][3] * inv);
      *(uint2*)(dst + db * 16) = w;
    }
  }
}

// ------------------------------------------------------------------ host dispatch --
// ic, with_d, with_d_g: decoder_common.hpp

// f(ic<MODE>, bool_constant<RMS>) for a GEMV epilogue mode (0, 1, 2, 4); false: no such mode
template <class F>
bool with_mode_rms(int mode, bool rms, F f) {
  auto on_rms = [&](auto M) {
    if (rms) f(M, std::true_type{});
    else f(M, std::false_type{});
  };
  switch (mode) {
    case 0: on_rms(ic<0>{}); return true;
    case 1: on_rms(ic<1>{}); return true;
    case 2: on_rms(ic<2>{}); return true;
    case 4: on_rms(ic<4>{}); return true;
    default: return false;
  }
}

// dec_gemv over Q4G32 / Q8G32 weights (k_gemv_q4<.., BITS>)
template <int BITS>
int gemv_qn(int mode, const void* x, const float* rms_w, float eps, const void* Wq, const void* Wsm, int N, int K,
            const void* res, void* out, hipStream_t s) {
  if (K <= 0 || K % kQ4Group || K > kGemvQ4MaxK || N <= 0 || (mode == 2 && N % 32) || (mode == 1 && !res) ||
      ((uintptr_t)Wq | (uintptr_t)x) % 16 || (uintptr_t)Wsm % 4 || (rms_w && (uintptr_t)rms_w % 16))
    return (int)hipErrorInvalidValue;
  const int nout = mode == 2 ? N / 2 : N;
  const int per_block = 4 * (mode == 2 ? kGemvRows / 2 : kGemvRows);
  const dim3 g((unsigned)((nout + per_block - 1) / per_block)), b(256);
  const size_t lds = (size_t)(K / kQ4Group) * kQ4Rec * sizeof(float);
  const bool known = with_mode_rms(mode, rms_w != nullptr, [&](auto M, auto R) {
    hipLaunchKernelGGL((k_gemv_q4<M(), R(), BITS>), g, b, lds, s, (const uint16_t*)x, rms_w, eps, (const uint8_t*)Wq,
                       (const uint32_t*)Wsm, K, nout, (const uint16_t*)res, out);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

// the four quantise / dequantise entry points: W bf16 [N, K] row-major and contiguous, one thread per
// 32-weight group; launch(grid, groups) starts the kernel
template <class F>
int quant_launch(const void* W, long N, int K, const void* Wq, const void* Wsm, F launch) {
  if (N <= 0 || K <= 0 || K % kQ4Group || ((uintptr_t)W | (uintptr_t)Wq) % 16 || (uintptr_t)Wsm % 4)
    return (int)hipErrorInvalidValue;
  const long groups = N * (K / kQ4Group);
  launch(dim3((unsigned)((groups + 255) / 256)), groups);
  return (int)hipGetLastError();
}

// split-L workspace, one per stream (the decode step's layers run in order on one stream): H <= 128
// heads x kMaxSplits partials of hd + 2 floats, allocated on first use (outside graph capture: the
// decode engine runs one step eagerly before capturing)
float* split_workspace(hipStream_t s) {
  static std::mutex mu;
  static std::map<hipStream_t, float*> table;
  std::lock_guard<std::mutex> g(mu);
  auto it = table.find(s);
  if (it != table.end()) return it->second;
  float* w = nullptr;
  if (hipMalloc((void**)&w, (size_t)128 * kMaxSplits * (256 + 2) * sizeof(float)) != hipSuccess) return nullptr;
  return table[s] = w;
}

}  // namespace

extern "C" {

// Causal prefill attention over the KV cache (k_prefill_attn): q rows [n, ldq] (H heads x hd,
// RoPE applied), k / v cache rows [pos0 + n, ldkv] (KVH heads x hd; rows pos0 .. pos0+n-1 are
// this chunk's), out rows [n, ldo].  hd 64 or 128; rows and bases 16-B aligned.
int dec_attn_prefill_kv(const void* q, long ldq, const void* k, const void* v, long ldkv, int n, int pos0, int H,
                        int KVH, int hd, float scale, void* out, long ldo, hipStream_t s) {
  if (n <= 0) return 0;
  if (pos0 < 0 || H <= 0 || KVH <= 0 || H % KVH || (hd != 64 && hd != 128) || ldq % 8 || ldkv % 8 || ldo % 8 ||
      ldq < (long)H * hd || ldkv < (long)KVH * hd || ldo < (long)H * hd ||
      ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15)
    return (int)hipErrorInvalidValue;
  const int nqb = (n + 127) / 128;
  const float sl2 = scale * 1.4426950408889634f;
  if (hd == 64)
    hipLaunchKernelGGL(k_prefill_attn<64>, dim3(nqb * H), dim3(256), 0, s, (const uint16_t*)q, ldq,
                       (const uint16_t*)k, (const uint16_t*)v, ldkv, n, pos0, H, KVH, sl2, (uint16_t*)out, ldo);
  else
    hipLaunchKernelGGL(k_prefill_attn<128>, dim3(nqb * H), dim3(256), 0, s, (const uint16_t*)q, ldq,
                       (const uint16_t*)k, (const uint16_t*)v, ldkv, n, pos0, H, KVH, sl2, (uint16_t*)out, ldo);
  return (int)hipGetLastError();
}

// dec_attn_prefill_kv over up to 16 prompt chunks in one launch.  q rows [T, ldq] and out rows [T, ldo]
// are packed; segs: HOST int32 [nseg][4] = {row0, n, pos0, slot} (decoder_common.hpp PrefillSegs): rows
// row0 .. row0+n-1 are the tokens at positions pos0 .. pos0+n-1 of the prompt in cache slot `slot`; k / v:
// slot 0's layer cache rows [n_ctx, ldkv], slot b's at + b * seq_stride elements.  The table is checked
// here (n >= 1, rows inside T and disjoint, slot < nslots and used once, 0 <= pos0, pos0 + n <= n_ctx;
// alignment and head dim as dec_attn_prefill_kv) and passed by value; hipErrorInvalidValue with nothing
// launched when a check fails.  A segment's output is bit-identical to dec_attn_prefill_kv on it alone.
int dec_attn_prefill_kv_seg(const void* q, long ldq, long T, const int32_t* segs, int nseg, const void* k,
                            const void* v, long ldkv, long seq_stride, int nslots, int n_ctx, int H, int KVH, int hd,
                            float scale, void* out, long ldo, hipStream_t s) {
  PrefillSegs tb;
  if (H <= 0 || KVH <= 0 || H % KVH || (hd != 64 && hd != 128) || ldq % 8 || ldkv % 8 || ldo % 8 || seq_stride % 8 ||
      ldq < (long)H * hd || ldkv < (long)KVH * hd || ldo < (long)H * hd || seq_stride < (long)n_ctx * ldkv ||
      !q || !k || !v || !out || ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15 ||
      !prefill_segs_build(segs, nseg, T, nslots, n_ctx, seq_stride, tb))
    return (int)hipErrorInvalidValue;
  long blocks = 0;
  for (int i = 0; i < tb.nseg; ++i) blocks += (long)((tb.n[i] + 127) / 128) * H;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const float sl2 = scale * 1.4426950408889634f;
  if (hd == 64)
    hipLaunchKernelGGL((k_prefill_attn<64, PrefillSegs>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint16_t*)q,
                       ldq, (const uint16_t*)k, (const uint16_t*)v, ldkv, 0, 0, H, KVH, sl2, (uint16_t*)out, ldo, tb);
  else
    hipLaunchKernelGGL((k_prefill_attn<128, PrefillSegs>), dim3((unsigned)blocks), dim3(256), 0, s, (const uint16_t*)q,
                       ldq, (const uint16_t*)k, (const uint16_t*)v, ldkv, 0, 0, H, KVH, sl2, (uint16_t*)out, ldo, tb);
  return (int)hipGetLastError();
}

// Single-token decode attention.  q: bf16 [H*hd] (one token, RoPE applied); k/v: bf16 cache rows
// [L, ldkv] (ldkv = KVH*hd); out: bf16 [H*hd].  hd in {64, 128, 192, 256}, H % KVH == 0, L >= 1, 16-B
// aligned rows.  With st != null the cache length is st[0] + 1, read on the device, and L is the cache
// CAPACITY (it sizes the split count).  ws: the caller's split workspace (H * 32 * (hd + 2) floats);
// null: a per-stream one allocated on first use -- a graph-captured step must pass its own, since
// nothing may be allocated during capture.
// Kernel choice: head dims 64 / 128 / 256 with a query-group size of 1, 2, 4 or 8 run the grouped
// three-phase kernel (k_attn_decode_g), whole up to kSmallL keys and as the splits of longer caches;
// every other shape walks the keys (k_attn_decode, k_attn_decode_split).
// Measured and removed: SPL_DEC_SMALL=0, which put the grouped shapes back on the walking kernels:
// 28 against 11.5 us per layer at a 300-key cache, q4 decode 0.715 against 0.577 ms/token
// (profiles/r3_decode_attn_small_ab.jsonl).
int dec_attn_decode_ws(const void* q, const void* k, const void* v, long ldkv, int L, int H, int KVH, int hd,
                       float scale, void* out, const int32_t* st, float* ws, hipStream_t s) {
  if (L <= 0 || H <= 0 || KVH <= 0 || H % KVH || hd <= 0 || hd % 64 || hd > 256 || ldkv % 8 ||
      ldkv < (long)KVH * hd || ((uintptr_t)k | (uintptr_t)v | (uintptr_t)q) % 16)  // q: 16-B loads in k_attn_decode_g
    return (int)hipErrorInvalidValue;
  const int grp = H / KVH;
  const int S = decode_splits(L);
  const bool grouped = (hd == 64 || hd == 128 || hd == 256) && (grp == 1 || grp == 2 || grp == 4 || grp == 8);
  const uint16_t *qq = (const uint16_t*)q, *kk = (const uint16_t*)k, *vv = (const uint16_t*)v;
  uint16_t* oo = (uint16_t*)out;
  if (S > 1 && H <= 128) {
    if (!ws) ws = split_workspace(s);
    if (!ws) return (int)hipErrorOutOfMemory;
    if (grouped && ((L + S - 1) / S + 63) / 64 * 64 <= kSmallL) {
      with_d_g(hd / 64, grp, [&](auto D, auto G) {
        if constexpr (D() != 3)
          hipLaunchKernelGGL((k_attn_decode_g<D(), G(), true>), dim3((unsigned)KVH, (unsigned)S), dim3(256), 0, s, qq,
                             kk, vv, ldkv, L, scale, (uint16_t*)nullptr, st, ws);
      });
    } else {
      // heads per workgroup: the whole kv group when it is 2, 4 or 8 heads (shared K/V rows), else 1
      const int wg = (grp == 2 || grp == 4 || grp == 8) ? grp : 1;
      with_d_g(hd / 64, wg, [&](auto D, auto G) {
        hipLaunchKernelGGL((k_attn_decode_split<D(), G()>), dim3((unsigned)(H / G()), (unsigned)S),
                           dim3(kSplitWaves * 64), 0, s, qq, kk, vv, ldkv, L, grp, scale, ws, st);
      });
    }
    hipLaunchKernelGGL(k_attn_combine, dim3((unsigned)H), dim3(256), 0, s, ws, S, hd, oo);
  } else if (grouped && L <= kSmallL) {
    with_d_g(hd / 64, grp, [&](auto D, auto G) {
      if constexpr (D() != 3)
        hipLaunchKernelGGL((k_attn_decode_g<D(), G()>), dim3((unsigned)KVH), dim3(256), 0, s, qq, kk, vv, ldkv, L,
                           scale, oo, st, (float*)nullptr);
    });
  } else {
    with_d(hd / 64, [&](auto D) {
      hipLaunchKernelGGL(k_attn_decode<D()>, dim3((unsigned)H), dim3(kDecWaves * 64), 0, s, qq, kk, vv, ldkv, L, grp,
                         hd, scale, oo, st);
    });
  }
  return (int)hipGetLastError();
}

int dec_attn_decode_st(const void* q, const void* k, const void* v, long ldkv, int L, int H, int KVH, int hd,
                       float scale, void* out, const int32_t* st, hipStream_t s) {
  return dec_attn_decode_ws(q, k, v, ldkv, L, H, KVH, hd, scale, out, st, nullptr, s);
}
int dec_attn_decode(const void* q, const void* k, const void* v, long ldkv, int L, int H, int KVH, int hd,
                    float scale, void* out, hipStream_t s) {
  return dec_attn_decode_ws(q, k, v, ldkv, L, H, KVH, hd, scale, out, nullptr, nullptr, s);
}

// x/out: bf16 rows (strides in elements), w: fp32 [d]; d % 8 == 0, 16-B aligned rows.
int dec_rmsnorm(const void* x, long ldx, const float* w, long T, int d, float eps, void* out, long ldo,
                hipStream_t s) {
  if (T <= 0) return 0;
  if (d <= 0 || d % 8 || ldx % 8 || ldo % 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rmsnorm, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, (const uint16_t*)x, ldx, w, T, d, eps,
                     (uint16_t*)out, ldo);
  return (int)hipGetLastError();
}

// qkv: bf16 [T, ld]; columns [0, ncols) hold q|k heads of width hd; row t has position pos0 + t;
// cos/sin: fp32 [n_ctx, hd/2] (the caller guarantees pos0 + T <= n_ctx).
int dec_rope(void* qkv, long ld, long T, int ncols, int hd, int pos0, const float* cos_tab, const float* sin_tab,
             hipStream_t s) {
  if (T <= 0) return 0;
  if (hd % 8 || ncols % hd || ld % 8 || pos0 < 0) return (int)hipErrorInvalidValue;
  const long work = T * (ncols / 8);
  long g = (work + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_rope, dim3((unsigned)g), dim3(256), 0, s, (uint16_t*)qkv, ld, T, ncols, hd, pos0, cos_tab,
                     sin_tab);
  return (int)hipGetLastError();
}

// y = x . W^T for one token (see k_gemv).  mode 0 store, 1 residual, 2 SwiGLU (N = packed rows,
// out has N / 2), 4 fp32; rms_w != null: x is RMS-normalised with rms_w / eps first.
// K % 8 == 0, K <= 16384, 16-B aligned W / x.
int dec_gemv(int mode, const void* x, const float* rms_w, float eps, const void* W, int N, int K, const void* res,
             void* out, hipStream_t s) {
  if (K <= 0 || K % 8 || K > kGemvMaxK || N <= 0 || (mode == 2 && N % 32) || (mode == 1 && !res) ||
      ((uintptr_t)W | (uintptr_t)x) % 16)
    return (int)hipErrorInvalidValue;
  const int nout = mode == 2 ? N / 2 : N;
  const int per_block = 4 * (mode == 2 ? kGemvRows / 2 : kGemvRows);
  const dim3 g((unsigned)((nout + per_block - 1) / per_block)), b(256);
  const bool known = with_mode_rms(mode, rms_w != nullptr, [&](auto M, auto R) {
    hipLaunchKernelGGL((k_gemv<M(), R()>), g, b, 0, s, (const uint16_t*)x, rms_w, eps, (const uint16_t*)W, K, nout,
                       (const uint16_t*)res, out);
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

// dec_gemv over Q4G32 weights (k_gemv_q4): Wq [N, K/2] nibbles, Wsm [N, K/32] bf16 (d, m) pairs.
// K % 32 == 0, K <= 16384, 16-B aligned x / Wq, 4-B aligned Wsm.
int dec_gemv_q4(int mode, const void* x, const float* rms_w, float eps, const void* Wq, const void* Wsm, int N,
                int K, const void* res, void* out, hipStream_t s) {
  return gemv_qn<4>(mode, x, rms_w, eps, Wq, Wsm, N, K, res, out, s);
}

// dec_gemv over Q8G32 weights: Wq [N, K] bytes, Wsm [N, K/32] bf16 (d, m) pairs, w = d u + m
int dec_gemv_q8(int mode, const void* x, const float* rms_w, float eps, const void* Wq, const void* Wsm, int N,
                int K, const void* res, void* out, hipStream_t s) {
  return gemv_qn<8>(mode, x, rms_w, eps, Wq, Wsm, N, K, res, out, s);
}

// bf16 W [N, K] (row-major, contiguous) <-> Q8G32 planes
int dec_q8_quantize(const void* W, long N, int K, void* Wq, void* Wsm, hipStream_t s) {
  return quant_launch(W, N, K, Wq, Wsm, [&](dim3 g, long groups) {
    hipLaunchKernelGGL(k_q8_quant, g, dim3(256), 0, s, (const uint16_t*)W, groups, (uint8_t*)Wq, (uint32_t*)Wsm);
  });
}

int dec_q8_dequant(const void* Wq, const void* Wsm, long N, int K, void* W, hipStream_t s) {
  return quant_launch(W, N, K, Wq, Wsm, [&](dim3 g, long groups) {
    hipLaunchKernelGGL(k_q8_dequant, g, dim3(256), 0, s, (const uint8_t*)Wq, (const uint32_t*)Wsm, groups,
                       (uint16_t*)W);
  });
}

// bf16 W [N, K] (row-major, contiguous) <-> Q4G32 planes
int dec_q4_quantize(const void* W, long N, int K, void* Wq, void* Wsm, hipStream_t s) {
  return quant_launch(W, N, K, Wq, Wsm, [&](dim3 g, long groups) {
    hipLaunchKernelGGL(k_q4_quant, g, dim3(256), 0, s, (const uint16_t*)W, groups, K / kQ4Group, (uint8_t*)Wq,
                       (uint32_t*)Wsm);
  });
}

int dec_q4_dequant(const void* Wq, const void* Wsm, long N, int K, void* W, hipStream_t s) {
  return quant_launch(W, N, K, Wq, Wsm, [&](dim3 g, long groups) {
    hipLaunchKernelGGL(k_q4_dequant, g, dim3(256), 0, s, (const uint8_t*)Wq, (const uint32_t*)Wsm, groups,
                       (uint16_t*)W);
  });
}

int dec_embed_tok(const void* emb, int d, const int32_t* st, void* x, hipStream_t s) {
  if (d % 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_embed_tok, dim3(1), dim3(256), 0, s, (const uint16_t*)emb, d, st, (uint16_t*)x);
  return (int)hipGetLastError();
}

// qkv: bf16 [(H + 2 KVH) hd] of the step's token; kc / vc: the layer's cache [n_ctx, ldkv]
int dec_rope_kv(void* qkv, int H, int KVH, int hd, const float* cos_tab, const float* sin_tab, const int32_t* st,
                void* kc, void* vc, long ldkv, hipStream_t s) {
  if (hd % 2 || H <= 0 || KVH <= 0 || ldkv < (long)KVH * hd) return (int)hipErrorInvalidValue;
  const int work = (H + KVH) * hd / 2 + KVH * hd;
  hipLaunchKernelGGL(k_rope_kv, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, (uint16_t*)qkv, H, KVH, hd,
                     cos_tab, sin_tab, st, (uint16_t*)kc, (uint16_t*)vc, ldkv);
  return (int)hipGetLastError();
}

// floats of the workspace dec_sample_ws needs
long dec_sample_ws_floats() { return SB_FLOATS; }

// The sampler, with a caller-owned workspace (dec_sample_ws_floats() floats): vocabularies past 4096
// tokens run the multi-block chain (k_sb_*), smaller ones the single-workgroup register sampler
int dec_sample_ws(const float* logits, int V, const uint8_t* mask, float top_p, float temp, uint64_t seed,
                  int32_t* st, int inc_pos, int32_t* host_tok, float* ws, hipStream_t s) {
  if (V <= 0 || !ws) return (int)hipErrorInvalidValue;
  if (V <= kSampThreads * kSampRegs) {
    hipLaunchKernelGGL(k_sample_reg, dim3(1), dim3(kSampThreads), 0, s, logits, V, mask, top_p, temp, seed, st,
                       inc_pos, host_tok);
    return (int)hipGetLastError();
  }
  const dim3 g(kSbBlocks), b(kSbThreads);
  hipLaunchKernelGGL(k_sb_max, g, b, 0, s, logits, V, mask, ws);
  const int nucleus = top_p < 1.f;
  if (nucleus) {
    hipLaunchKernelGGL(k_sb_hist<0>, g, b, 0, s, logits, V, mask, ws);
    hipLaunchKernelGGL(k_sb_select<0>, dim3(1), dim3(kSbBins), 0, s, top_p, ws);
    hipLaunchKernelGGL(k_sb_hist<1>, g, b, 0, s, logits, V, mask, ws);
    hipLaunchKernelGGL(k_sb_select<1>, dim3(1), dim3(kSbBins), 0, s, top_p, ws);
  }
  hipLaunchKernelGGL(k_sb_part, g, b, 0, s, logits, V, mask, temp, nucleus, ws);
  hipLaunchKernelGGL(k_sb_draw, dim3(1), dim3(kSbBins), 0, s, logits, V, mask, temp, seed, ws, st, inc_pos, host_tok);
  return (int)hipGetLastError();
}

}  // extern "C"
