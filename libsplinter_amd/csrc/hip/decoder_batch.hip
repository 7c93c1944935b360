// decoder_batch.hip — one decode step for up to 16 generations at once (the completion daemon's
// --batch N path; models/decoder.py BatchDecodeEngine).
//
// A decode step is weight-bandwidth bound: every projection weight is streamed once per token, and the
// bytes streamed do not depend on how many sequences share the step.  The kernels here run the step of
// decoder_kernels.hip over `nseq` sequence slots:
//
//   dec_gemm_small[_q4|_q8]  out[b] = epilogue(x[b] . W^T) for 1..16 token rows: the weight tile is the A
//                            operand of mfma_f32_16x16x32_bf16, the token rows are the B operand
//   dec_embed_tok_b / dec_rope_kv_b / dec_attn_decode_b / dec_sample_b
//                            k_embed_tok, k_rope_kv, the four decode-attention kernels and both sampler
//                            forms with a slot index: each slot reads its position, token, draw index
//                            and seed from its own state record
//   dec_rope_kv_seg          RoPE + cache append of a batched prefill pass, one segment per prompt chunk
//   dec_kv_rows_fanout       the K / V rows of a shared prompt prefix, one source to up to 16 cache slots
//
// Device state: int32 st[nseq][8] = {pos, token, step, active, seed lo, seed hi, 0, 0} (decoder_common.hpp).
// A slot with active == 0 is skipped by every state-driven kernel: its cache rows, its record and its
// attention / logits rows stay untouched, and its host_tok entry is written as -1.  Which slots are live is
// device data, so a captured step never changes when a sequence joins or leaves.
//
// A slot-indexed kernel is its own signature, a prologue that picks the slot's operands (attn_slot,
// SAMPLE_SLOT, SB_SLOT), and the body of its single-sequence twin in decoder_kernels.hip, included as text
// from decoder_body_*.hpp: one source for both, so a slot computes what a solo run computes by construction.
// An include and not a shared function: a function boundary moved the register allocation of 8
// single-sequence kernels (profiles/decoder_prune/README.md); the same tokens after each kernel's own
// prologue compile to the instructions both files had as copies (profiles/decoder_share/README.md).
// DEC_SLOTS marks the two places where the forms differ inside a body: the guard for a wave with no keys in
// k_attn_decode_b's merge and the output row of k_attn_combine_b.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <type_traits>

#include "decoder_common.hpp"

#define DEC_SLOTS 1

namespace {

typedef __bf16 gs_bf16x8 __attribute__((ext_vector_type(8)));
typedef float gs_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxSeqs = 16;
// waves of a workgroup: they split K between them.  Measured and removed: 8 and 4 waves for the 4-bit planes
// (fewer, longer K walks per wave): 1.41 and 1.60 ms per step of 8 sequences against 1.36 with 16
// (profiles/decode_batch/README.md)
constexpr int kGsWaves = 16;
constexpr int kGsLoads = 4;     // 16-row weight loads a wave has in flight: 4 k-steps, 2 with two tiles
constexpr int kGsMaxK = 16384;

// ------------------------------------------------------------------ small GEMM --
// out[b][n] = epilogue(sum_k x[b][k] W[n][k]) for b < nseq <= 16.  One workgroup owns 16 weight rows (32 in
// MODE 2: the up and the gate half of one pack_upgate block), its 16 waves take the 32-k steps of K
// round-robin (wave w: steps w, w + 16, ..), so a 4096-row projection puts 4096 waves on the card and each
// wave still streams its rows with one 16-B load per lane and step.  Fragments (search_api.h, the query
// tiles): lane (li = lane % 16, g = lane / 16) holds k = 32 s + 8 g .. + 7 of weight row li for A and of
// token row li for B; the accumulator tile gives lane (li, g) the weight rows 4 g .. 4 g + 3 of token li.
// Token rows past nseq are zero, weight rows past N recompute row N - 1 and are not stored.  The 16 partial
// tiles meet in LDS and wave 0 adds them in wave order: no atomics, the same bits on every run, and token
// b's column depends on no other column.
// BITS 4 / 8 (Q4G32 / Q8G32): the integer codes go to the MFMA as they are (0..15 and 0..255 are exact in
// bf16); one 32-k group is one k-step, whose result c enters the fp32 accumulator as acc += d c with the
// group's d, and the offset term m sum_k x comes from a second MFMA over a tile of m (a bf16, so exact):
// the arithmetic of k_gemv_q4 (fp32 scales, exact codes) with the code conversion done once for all the
// sequences.  d q + m is never rounded to bf16.
// MODE as dec_gemv: 0 bf16 out, 1 + residual (may alias out: one lane reads and writes an element),
// 2 SwiGLU (up and gate land in the same lanes of the two tiles), 4 fp32 out.
template <int BITS>
__device__ __forceinline__ gs_bf16x8 gs_load_a(const uint8_t* W, long row, int K, int ks, int g, bool valid) {
  if constexpr (BITS == 16) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (valid) v = *(const uint4*)((const uint16_t*)W + row * K + ks * 32 + g * 8);
    return __builtin_bit_cast(gs_bf16x8, v);
  } else if constexpr (BITS == 4) {
    const uint32_t w = *(const uint32_t*)(W + row * (K / 2) + ks * 16 + g * 4);
    uint4 v;
    v.x = pk2((float)(w & 15u), (float)((w >> 4) & 15u));
    v.y = pk2((float)((w >> 8) & 15u), (float)((w >> 12) & 15u));
    v.z = pk2((float)((w >> 16) & 15u), (float)((w >> 20) & 15u));
    v.w = pk2((float)((w >> 24) & 15u), (float)(w >> 28));
    return __builtin_bit_cast(gs_bf16x8, v);
  } else {
    const uint2 w = *(const uint2*)(W + row * (long)K + ks * 32 + g * 8);
    uint4 v;
    v.x = pk2((float)(w.x & 255u), (float)((w.x >> 8) & 255u));
    v.y = pk2((float)((w.x >> 16) & 255u), (float)(w.x >> 24));
    v.z = pk2((float)(w.y & 255u), (float)((w.y >> 8) & 255u));
    v.w = pk2((float)((w.y >> 16) & 255u), (float)(w.y >> 24));
    return __builtin_bit_cast(gs_bf16x8, v);
  }
}

template <int MODE, int BITS>
__global__ __launch_bounds__(kGsWaves * 64) void k_gemm_small(const uint16_t* __restrict__ x, long ldx, int nseq,
                                                              const uint8_t* __restrict__ W,
                                                              const uint32_t* __restrict__ Wsm, int K, int N,
                                                              const uint16_t* res, long ldr, void* out, long ldo) {
  constexpr int RT = MODE == 2 ? 2 : 1;  // 16-row tiles per workgroup
  constexpr int NW = kGsWaves;
  constexpr int kGsUnroll = kGsLoads / RT;
  __shared__ float red[NW][RT * 4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int nks = (K + 31) >> 5, ng = K >> 5;
  long rows[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    long r = (long)blockIdx.x * (16 * RT) + t * 16 + li;
    rows[t] = r < N ? r : N - 1;
  }
  const bool tok = li < nseq;
  const uint16_t* xr = x + (long)li * ldx;
  gs_f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = gs_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int ks0 = wave; ks0 < nks; ks0 += NW * kGsUnroll) {
    gs_bf16x8 a[kGsUnroll][RT], b[kGsUnroll];
    uint32_t sm[kGsUnroll][RT];
#pragma unroll
    for (int u = 0; u < kGsUnroll; ++u) {
      const int ks = ks0 + u * NW;
      const bool valid = ks < nks && ks * 32 + g * 8 < K;
      uint4 xv = make_uint4(0, 0, 0, 0);
      if (valid && tok) xv = *(const uint4*)(xr + ks * 32 + g * 8);
      b[u] = __builtin_bit_cast(gs_bf16x8, xv);
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        if (BITS == 16 || ks < nks) {
          a[u][t] = gs_load_a<BITS>(W, rows[t], K, ks, g, valid);
          if constexpr (BITS != 16) sm[u][t] = Wsm[rows[t] * ng + ks];
        } else {
          a[u][t] = gs_bf16x8{};
          sm[u][t] = 0;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kGsUnroll; ++u) {
      if constexpr (BITS == 16) {
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][t], b[u], acc[t], 0, 0, 0);
      } else {
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          // lane li holds the (d, m) word of weight row li.  m is a bf16: a tile holding m in every k of its
          // row, through the same MFMA, adds m sum_k x exactly and in fp32, with no group sum to prepare
          const uint32_t w = sm[u][t], m2 = (w & 0xffff0000u) | (w >> 16);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(gs_bf16x8, make_uint4(m2, m2, m2, m2)), b[u], acc[t], 0, 0, 0);
          const gs_f32x4 c =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][t], b[u], gs_f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r)  // this lane's rows are 4 g + r: their d from the lanes that hold it
            acc[t][r] = fmaf(bf2f((uint32_t)__shfl((int)w, 4 * g + r, 64) & 0xffff), c[r], acc[t][r]);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][t * 4 + r][lane] = acc[t][r];
  __syncthreads();
  if (wave != 0 || !tok) return;
  float v[RT][4] = {};
#pragma unroll 2
  for (int w = 0; w < NW; ++w)  // wave order: the sum is the same on every run
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[t][r] += red[w][t * 4 + r][lane];
  const int nout = MODE == 2 ? N / 2 : N;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long o = (long)blockIdx.x * 16 + 4 * g + r;
    if (o >= nout) continue;
    if constexpr (MODE == 4) {
      ((float*)out)[(long)li * ldo + o] = v[0][r];
    } else {
      float y = v[0][r];
      if constexpr (MODE == 1) y += bf2f(res[(long)li * ldr + o]);
      if constexpr (MODE == 2) y = v[0][r] * v[1][r] / (1.f + __expf(-v[1][r]));
      ((uint16_t*)out)[(long)li * ldo + o] = __builtin_bit_cast(uint16_t, (__bf16)y);
    }
  }
}

template <int BITS>
int gemm_small(int mode, const void* x, long ldx, int nseq, const void* W, const void* Wsm, int N, int K,
               const void* res, long ldr, void* out, long ldo, hipStream_t s) {
  const int kmul = BITS == 16 ? 8 : 32;
  if (nseq < 1 || nseq > kMaxSeqs || K <= 0 || K % kmul || K > kGsMaxK || N <= 0 || (mode == 2 && N % 32) ||
      (mode == 1 && (!res || ldr < N)) || ldx < K || ldx % 8 || ldo < (mode == 2 ? N / 2 : N) ||
      ((uintptr_t)W | (uintptr_t)x) % 16 || (BITS != 16 && (!Wsm || (uintptr_t)Wsm % 4)))
    return (int)hipErrorInvalidValue;
  const dim3 b(kGsWaves * 64);
  const uint16_t* xx = (const uint16_t*)x;
  const uint8_t* ww = (const uint8_t*)W;
  const uint32_t* sm = (const uint32_t*)Wsm;
  const uint16_t* rr = (const uint16_t*)res;
  switch (mode) {
    case 0:
      hipLaunchKernelGGL((k_gemm_small<0, BITS>), dim3((unsigned)((N + 15) / 16)), b, 0, s, xx, ldx, nseq, ww, sm, K, N,
                         rr, ldr, out, ldo);
      break;
    case 1:
      hipLaunchKernelGGL((k_gemm_small<1, BITS>), dim3((unsigned)((N + 15) / 16)), b, 0, s, xx, ldx, nseq, ww, sm, K, N,
                         rr, ldr, out, ldo);
      break;
    case 2:
      hipLaunchKernelGGL((k_gemm_small<2, BITS>), dim3((unsigned)(N / 32)), b, 0, s, xx, ldx, nseq, ww, sm, K, N, rr,
                         ldr, out, ldo);
      break;
    case 4:
      hipLaunchKernelGGL((k_gemm_small<4, BITS>), dim3((unsigned)((N + 15) / 16)), b, 0, s, xx, ldx, nseq, ww, sm, K, N,
                         rr, ldr, out, ldo);
      break;
    default:
      return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ embedding, RoPE + cache append --
// x[b] = emb[st[b].token]: one workgroup per slot
__global__ void k_embed_tok_b(const uint16_t* __restrict__ emb, int d, const int32_t* __restrict__ st,
                              uint16_t* __restrict__ x, long ldx) {
  const int32_t* sb = st + blockIdx.x * ST_WORDS;
  if (!sb[ST_ACTIVE]) return;
  const long t = sb[ST_TOK];
  uint16_t* xo = x + blockIdx.x * ldx;
  for (int c = threadIdx.x; c < d / 8; c += blockDim.x) *(uint4*)(xo + c * 8) = *(const uint4*)(emb + t * d + c * 8);
}

// k_rope_kv per slot (blockIdx.y): q rotated in place in row b of qkv, k / v appended at row pos of the slot's
// cache (kc + b * seq_stride)
__global__ void k_rope_kv_b(uint16_t* __restrict__ qkv, long ldq, int H, int KVH, int hd, const float* __restrict__ cs,
                            const float* __restrict__ sn, const int32_t* __restrict__ st, uint16_t* __restrict__ kc,
                            uint16_t* __restrict__ vc, long ldkv, long seq_stride) {
  const int32_t* sb = st + blockIdx.y * ST_WORDS;
  if (!sb[ST_ACTIVE]) return;
  qkv += blockIdx.y * ldq;
  kc += blockIdx.y * seq_stride;
  vc += blockIdx.y * seq_stride;
  const long p = sb[ST_POS];
#include "decoder_body_rope_kv.hpp"
}

// RoPE + cache append of a batched prefill pass (BatchDecodeEngine.prefill): blockIdx.y is a segment of the
// by-value table, one thread per 8 columns of a packed qkv row.  q columns rotate in place at the row's own
// position pos0 + r with k_rope's statements (so its bits); a k chunk is rotated the same way and stored at
// row pos0 + r of the slot's cache instead of back into qkv, a v chunk is copied there: the cache holds what
// dec_rope followed by the two slice copies of CausalLM.forward leaves.  The k columns of qkv stay
// unrotated; nothing reads them afterwards.
__global__ __launch_bounds__(256) void k_rope_kv_seg(uint16_t* __restrict__ qkv, long ld, int H, int KVH, int hd,
                                                     const float* __restrict__ cs, const float* __restrict__ sn,
                                                     uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, long ldkv,
                                                     PrefillSegs tb) {
  const PrefillSeg sg = prefill_seg_at(tb, blockIdx.y);
  const int qcols = H * hd, qk = qcols + KVH * hd;
  const int per_row = (qk + KVH * hd) >> 3;
  const long total = (long)sg.n * per_row;
  const int half = hd >> 1;
  qkv += (long)sg.row0 * ld;
  kc += (long)sg.slot * tb.seq_stride;
  vc += (long)sg.slot * tb.seq_stride;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long row = q / per_row;
    const int col = (int)(q - row * per_row) * 8;
    const long p = sg.pos0 + row;
    uint16_t* ptr = qkv + row * ld + col;
    if (col >= qk) {
      *(uint4*)(vc + p * ldkv + (col - qk)) = *(const uint4*)ptr;
      continue;
    }
    const int i0 = (col % hd) >> 1;  // first pair index inside the head
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
    uint16_t* dst = col < qcols ? ptr : kc + p * ldkv + (col - qcols);
    *(uint4*)dst = pack8(o);
  }
}

// Shared prompt prefix (BatchDecodeEngine.set_prefix): the first `rows` rows of every K / V plane of one
// source go to up to 16 cache slots.  The destination slots travel BY VALUE in the kernel arguments, as the
// prefill segment table does.  One thread per 16-B vector of the planes x rows x kvd / 8 source vectors, in a
// grid-stride loop: the vector is loaded once and stored to every destination from registers, so a restore
// to 15 held slots reads the prefix once, not 15 times.
struct FanoutDst {
  int ndst;
  int slot[kMaxSeqs];
};

__global__ __launch_bounds__(256) void k_kv_rows_fanout(const uint16_t* __restrict__ src, long src_plane,
                                                        uint16_t* __restrict__ dst, long dst_plane, long seq_stride,
                                                        int rows, int vec_row, long total, FanoutDst tb) {
  const long per_plane = (long)rows * vec_row;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long plane = q / per_plane;
    const long e = (q - plane * per_plane) * 8;  // rows are contiguous: element offset inside the plane
    const uint4 v = *(const uint4*)(src + plane * src_plane + e);
    uint16_t* d = dst + plane * dst_plane + e;
#pragma unroll
    for (int j = 0; j < kMaxSeqs; ++j)
      if (j < tb.ndst) *(uint4*)(d + (long)tb.slot[j] * seq_stride) = v;
  }
}

// ------------------------------------------------------------------ decode attention --
// The four kernels of dec_attn_decode_ws with the slot in blockIdx.z: the slot's query row, cache, output row
// and workspace slice, and its length st[b].pos + 1.  A slot shorter than the captured span runs empty
// splits, as the single-sequence kernels do under a device-side length.
struct AttnSlot {
  const uint16_t *q, *K, *V;
  uint16_t* out;
  float* ws;
  int L;
};
__device__ __forceinline__ bool attn_slot(AttnSlot& a, const int32_t* st, long ldq, long seq_stride, long ldo,
                                          long ws_stride) {
  const int b = blockIdx.z;
  const int32_t* sb = st + b * ST_WORDS;
  if (!sb[ST_ACTIVE]) return false;
  a.L = sb[ST_POS] + 1;
  a.q += b * ldq;
  a.K += b * seq_stride;
  a.V += b * seq_stride;
  if (a.out) a.out += b * ldo;
  if (a.ws) a.ws += b * ws_stride;
  return true;
}

template <int DPL>
__global__ __launch_bounds__(kDecWaves * 64) void k_attn_decode_b(const uint16_t* __restrict__ q_, long ldq,
                                                                  const uint16_t* __restrict__ K_,
                                                                  const uint16_t* __restrict__ V_, long ldkv,
                                                                  long seq_stride, int grp, int hd, float scale,
                                                                  uint16_t* __restrict__ out_, long ldo,
                                                                  const int32_t* __restrict__ st) {
  AttnSlot sl{q_, K_, V_, out_, nullptr, 0};
  if (!attn_slot(sl, st, ldq, seq_stride, ldo, 0)) return;
  const uint16_t *q = sl.q, *K = sl.K, *V = sl.V;
  uint16_t* out = sl.out;
  const int L = sl.L;
#include "decoder_body_attn_walk.hpp"
}

// SPLIT: partials to the slot's ws slice for k_attn_combine_b
template <int D, int G, bool SPLIT>
__global__ __launch_bounds__(256) void k_attn_decode_g_b(const uint16_t* __restrict__ q_, long ldq,
                                                         const uint16_t* __restrict__ K_,
                                                         const uint16_t* __restrict__ V_, long ldkv, long seq_stride,
                                                         float scale, uint16_t* __restrict__ out_, long ldo,
                                                         const int32_t* __restrict__ st, float* __restrict__ ws_,
                                                         long ws_stride) {
  AttnSlot sl{q_, K_, V_, out_, ws_, 0};
  if (!attn_slot(sl, st, ldq, seq_stride, ldo, ws_stride)) return;
  const uint16_t *q = sl.q, *K = sl.K, *V = sl.V;
  uint16_t* out = sl.out;
  float* ws = sl.ws;
  const int L = sl.L;
#include "decoder_body_attn_g.hpp"
}

// grid (H / G, S, nseq)
template <int DPL, int G>
__global__ __launch_bounds__(kSplitWaves * 64) void k_attn_decode_split_b(
    const uint16_t* __restrict__ q_, long ldq, const uint16_t* __restrict__ K_, const uint16_t* __restrict__ V_,
    long ldkv, long seq_stride, int grp, float scale, float* __restrict__ ws_, long ws_stride,
    const int32_t* __restrict__ st) {
  AttnSlot sl{q_, K_, V_, nullptr, ws_, 0};
  if (!attn_slot(sl, st, ldq, seq_stride, 0, ws_stride)) return;
  const uint16_t *q = sl.q, *K = sl.K, *V = sl.V;
  float* ws = sl.ws;
  const int L = sl.L;
#include "decoder_body_attn_split.hpp"
}

__global__ void k_attn_combine_b(const float* __restrict__ ws_, long ws_stride, int S, int hd,
                                 uint16_t* __restrict__ out, long ldo, const int32_t* __restrict__ st) {
  const int b = blockIdx.z;
  if (!st[b * ST_WORDS + ST_ACTIVE]) return;
  const float* ws = ws_ + b * ws_stride;
#include "decoder_body_attn_combine.hpp"
}

// ------------------------------------------------------------------ sampler --
// k_sample_reg and the k_sb_* chain with a slot index: slot b samples logits row b with the seed and the
// draw index of its own record and its own workspace slice; the statements are the single-sequence
// kernels' own, so a slot draws the token dec_sample_ws draws from the same inputs.
__device__ __forceinline__ uint64_t slot_seed(const int32_t* sb) {
  return (uint64_t)(uint32_t)sb[ST_SEED_LO] | ((uint64_t)(uint32_t)sb[ST_SEED_HI] << 32);
}

// the two kernels that draw: slot b's record, host_tok entry (-1 for an inactive slot), logits row and seed
#define SAMPLE_SLOT(b)                                                                                       \
  int32_t* st = st_ + (b) * ST_WORDS;                                                                        \
  int32_t* host_tok = host_tok_ ? host_tok_ + (b) : nullptr;                                                 \
  if (!st[ST_ACTIVE]) {                                                                                      \
    if (threadIdx.x == 0 && host_tok) __hip_atomic_store(host_tok, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); \
    return;                                                                                                  \
  }                                                                                                          \
  const float* logits = (logits_) + (b) * ldl;                                                               \
  const uint64_t seed = slot_seed(st)

__global__ __launch_bounds__(kSampThreads) void k_sample_reg_b(const float* __restrict__ logits_, long ldl, int V,
                                                               const uint8_t* __restrict__ mask, float top_p,
                                                               float temp, int32_t* __restrict__ st_, int inc_pos,
                                                               int32_t* host_tok_) {
  SAMPLE_SLOT(blockIdx.x);
#include "decoder_body_sample_reg.hpp"
}

// the k_sb_* chain, grid (blocks, nseq): blockIdx.y is the slot
#define SB_SLOT(logits_, ws_)                                         \
  if (!st[blockIdx.y * ST_WORDS + ST_ACTIVE]) return;                 \
  const float* logits = (logits_) + blockIdx.y * ldl;                 \
  float* ws = (ws_) + (long)blockIdx.y * SB_FLOATS

__global__ __launch_bounds__(kSbThreads) void k_sb_max_b(const float* __restrict__ logits_, long ldl, int V,
                                                         const uint8_t* __restrict__ mask, float* __restrict__ ws_,
                                                         const int32_t* __restrict__ st) {
  SB_SLOT(logits_, ws_);
#include "decoder_body_sb_max.hpp"
}

template <int LEVEL>
__global__ __launch_bounds__(kSbThreads) void k_sb_hist_b(const float* __restrict__ logits_, long ldl, int V,
                                                          const uint8_t* __restrict__ mask, float* __restrict__ ws_,
                                                          const int32_t* __restrict__ st) {
  SB_SLOT(logits_, ws_);
#include "decoder_body_sb_hist.hpp"
}

template <int LEVEL>
__global__ __launch_bounds__(kSbBins) void k_sb_select_b(float top_p, float* __restrict__ ws_,
                                                         const int32_t* __restrict__ st) {
  if (!st[blockIdx.y * ST_WORDS + ST_ACTIVE]) return;
  float* ws = ws_ + (long)blockIdx.y * SB_FLOATS;
#include "decoder_body_sb_select.hpp"
}

__global__ __launch_bounds__(kSbThreads) void k_sb_part_b(const float* __restrict__ logits_, long ldl, int V,
                                                          const uint8_t* __restrict__ mask, float temp, int nucleus,
                                                          float* __restrict__ ws_, const int32_t* __restrict__ st) {
  SB_SLOT(logits_, ws_);
#include "decoder_body_sb_part.hpp"
}

__global__ __launch_bounds__(kSbBins) void k_sb_draw_b(const float* __restrict__ logits_, long ldl, int V,
                                                       const uint8_t* __restrict__ mask, float temp,
                                                       const float* __restrict__ ws_, int32_t* __restrict__ st_,
                                                       int inc_pos, int32_t* host_tok_) {
  SAMPLE_SLOT(blockIdx.y);
  const float* ws = ws_ + (long)blockIdx.y * SB_FLOATS;
#include "decoder_body_sb_draw.hpp"
}
#undef SB_SLOT
#undef SAMPLE_SLOT

}  // namespace

extern "C" {

// out[b] = epilogue(x[b] . W^T), b < nseq in 1..16 (k_gemm_small).  x bf16 rows [nseq, ldx], W bf16 [N, K]
// row-major; mode 0 store bf16, 1 + res (bf16 rows [nseq, ldr], may alias out), 2 SwiGLU over pack_upgate
// rows (N packed rows, out has N / 2 columns), 4 fp32 out; out rows [nseq, ldo].  Strides in elements.
// K % 8 == 0, K <= 16384, ldx % 8 == 0, 16-B aligned x / W; N % 32 == 0 in mode 2.
int dec_gemm_small(int mode, const void* x, long ldx, int nseq, const void* W, int N, int K, const void* res, long ldr,
                   void* out, long ldo, hipStream_t s) {
  return gemm_small<16>(mode, x, ldx, nseq, W, nullptr, N, K, res, ldr, out, ldo, s);
}

// dec_gemm_small over Q4G32 planes (Wq [N, K/2] nibbles, Wsm [N, K/32] bf16 (d, m) pairs); K % 32 == 0
int dec_gemm_small_q4(int mode, const void* x, long ldx, int nseq, const void* Wq, const void* Wsm, int N, int K,
                      const void* res, long ldr, void* out, long ldo, hipStream_t s) {
  return gemm_small<4>(mode, x, ldx, nseq, Wq, Wsm, N, K, res, ldr, out, ldo, s);
}

// dec_gemm_small over Q8G32 planes (Wq [N, K] bytes, Wsm [N, K/32]); K % 32 == 0
int dec_gemm_small_q8(int mode, const void* x, long ldx, int nseq, const void* Wq, const void* Wsm, int N, int K,
                      const void* res, long ldr, void* out, long ldo, hipStream_t s) {
  return gemm_small<8>(mode, x, ldx, nseq, Wq, Wsm, N, K, res, ldr, out, ldo, s);
}

// x[b] = emb[st[b].token] for every active slot; x rows [nseq, ldx]
int dec_embed_tok_b(const void* emb, int d, const int32_t* st, int nseq, void* x, long ldx, hipStream_t s) {
  if (nseq < 1 || nseq > kMaxSeqs || d <= 0 || d % 8 || ldx < d || ldx % 8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_embed_tok_b, dim3((unsigned)nseq), dim3(256), 0, s, (const uint16_t*)emb, d, st,
                     (uint16_t*)x, ldx);
  return (int)hipGetLastError();
}

// qkv: bf16 rows [nseq, ldq] of (H + 2 KVH) hd; kc / vc: slot 0's layer cache [n_ctx, ldkv], slot b's at
// + b * seq_stride elements.  Slot b rotates at position st[b].pos and appends its k / v at that row.
int dec_rope_kv_b(void* qkv, long ldq, int nseq, int H, int KVH, int hd, const float* cos_tab, const float* sin_tab,
                  const int32_t* st, void* kc, void* vc, long ldkv, long seq_stride, hipStream_t s) {
  if (nseq < 1 || nseq > kMaxSeqs || hd % 2 || H <= 0 || KVH <= 0 || ldkv < (long)KVH * hd ||
      ldq < (long)(H + 2 * KVH) * hd)
    return (int)hipErrorInvalidValue;
  const int work = (H + KVH) * hd / 2 + KVH * hd;
  hipLaunchKernelGGL(k_rope_kv_b, dim3((unsigned)((work + 255) / 256), (unsigned)nseq), dim3(256), 0, s,
                     (uint16_t*)qkv, ldq, H, KVH, hd, cos_tab, sin_tab, st, (uint16_t*)kc, (uint16_t*)vc, ldkv,
                     seq_stride);
  return (int)hipGetLastError();
}

// RoPE + cache append for up to 16 prompt chunks in one launch (k_rope_kv_seg).  qkv: packed bf16 rows
// [T, ldq] of (H + 2 KVH) hd; segs: HOST int32 [nseg][4] = {row0, n, pos0, slot}, checked and passed by
// value as dec_attn_prefill_kv_seg does (hipErrorInvalidValue and nothing launched when a check fails);
// kc / vc: slot 0's layer cache [n_ctx, ldkv], slot b's at + b * seq_stride elements; cos / sin fp32
// [n_ctx, hd / 2].  Row row0 + r of a segment rotates its q columns in place at position pos0 + r and puts
// its rotated k and its v at cache row pos0 + r of the segment's slot: the bits of dec_rope + slice copies.
int dec_rope_kv_seg(void* qkv, long ldq, long T, const int32_t* segs, int nseg, int H, int KVH, int hd,
                    const float* cos_tab, const float* sin_tab, void* kc, void* vc, long ldkv, long seq_stride,
                    int nslots, int n_ctx, hipStream_t s) {
  PrefillSegs tb;
  if (H <= 0 || KVH <= 0 || H % KVH || (hd != 64 && hd != 128) || ldq % 8 || ldkv % 8 || seq_stride % 8 ||
      ldq < (long)(H + 2 * KVH) * hd || ldkv < (long)KVH * hd || seq_stride < (long)n_ctx * ldkv || !qkv || !kc ||
      !vc || !cos_tab || !sin_tab ||
      ((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)cos_tab | (uintptr_t)sin_tab) & 15 ||
      !prefill_segs_build(segs, nseg, T, nslots, n_ctx, seq_stride, tb))
    return (int)hipErrorInvalidValue;
  int nmax = 0;
  for (int i = 0; i < tb.nseg; ++i) nmax = tb.n[i] > nmax ? tb.n[i] : nmax;
  long g = ((long)nmax * ((H + 2 * KVH) * hd / 8) + 255) / 256;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(k_rope_kv_seg, dim3((unsigned)g, (unsigned)tb.nseg), dim3(256), 0, s, (uint16_t*)qkv, ldq, H, KVH,
                     hd, cos_tab, sin_tab, (uint16_t*)kc, (uint16_t*)vc, ldkv, tb);
  return (int)hipGetLastError();
}

// The first `rows` K / V rows of `planes` planes (one per (layer, k | v): 2 * layers) from one source to ndst
// cache slots in one launch (k_kv_rows_fanout).  Source plane j: bf16 rows [src_rows, kvd] at src + j * src_plane;
// destination i, plane j: rows [n_ctx, kvd] at dst + slots[i] * seq_stride + j * dst_plane; strides in elements.
// slots: HOST int32 [ndst], checked and passed by value.  Both directions of the shared prompt prefix: capture
// is a slot's cache -> the compact buffer (one destination, nslots 1, n_ctx the buffer's rows), restore is the
// buffer -> the held slots.  hipErrorInvalidValue and nothing launched when: ndst is not 1..16, a slot is
// outside 0..nslots-1 or listed twice, rows < 1 or past n_ctx or src_rows, kvd % 8, planes < 1, a plane or slot
// stride shorter than what it strides over, a base or stride off 16 B, or the source inside a destination.
int dec_kv_rows_fanout(const void* src, long src_plane, int src_rows, void* dst, long dst_plane, long seq_stride,
                       const int32_t* slots, int ndst, int nslots, int n_ctx, int planes, int rows, int kvd,
                       hipStream_t s) {
  if (!src || !dst || !slots || ndst < 1 || ndst > kMaxSeqs || nslots < 1 || planes < 1 || kvd < 8 || kvd % 8 ||
      rows < 1 || rows > n_ctx || rows > src_rows || src_plane % 8 || dst_plane % 8 || seq_stride % 8 ||
      src_plane < (long)src_rows * kvd || dst_plane < (long)n_ctx * kvd ||
      (nslots > 1 && seq_stride < (long)planes * dst_plane) || ((uintptr_t)src | (uintptr_t)dst) & 15)
    return (int)hipErrorInvalidValue;
  FanoutDst tb{};
  tb.ndst = ndst;
  const long span = (long)rows * kvd;  // elements of a plane that are touched
  const uint16_t *s0 = (const uint16_t*)src, *s1 = s0 + (planes - 1) * src_plane + span;
  for (int i = 0; i < ndst; ++i) {
    const int b = slots[i];
    if (b < 0 || b >= nslots) return (int)hipErrorInvalidValue;
    for (int j = 0; j < i; ++j)
      if (tb.slot[j] == b) return (int)hipErrorInvalidValue;
    const uint16_t *d0 = (const uint16_t*)dst + b * seq_stride, *d1 = d0 + (planes - 1) * dst_plane + span;
    if (s0 < d1 && d0 < s1) return (int)hipErrorInvalidValue;
    tb.slot[i] = b;
  }
  const int vec_row = kvd / 8;
  const long total = (long)planes * rows * vec_row;
  long g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(k_kv_rows_fanout, dim3((unsigned)g), dim3(256), 0, s, (const uint16_t*)src, src_plane,
                     (uint16_t*)dst, dst_plane, seq_stride, rows, vec_row, total, tb);
  return (int)hipGetLastError();
}

// floats of the workspace dec_attn_decode_b needs: nseq slots x H heads x kMaxSplits partials of hd + 2
long dec_attn_b_ws_floats(int nseq, int H, int hd) { return (long)nseq * H * kMaxSplits * (hd + 2); }

// Single-token GQA attention for every active slot in one launch.  q: bf16 rows [nseq, ldq] (row b holds the H
// query heads, RoPE applied); k / v: slot 0's cache rows [., ldkv], slot b's at + b * seq_stride; out: bf16 rows
// [nseq, ldo].  Slot b attends over its first st[b].pos + 1 rows.  L is the span the launch is sized for, as in
// dec_attn_decode_ws: up to 512 the single-workgroup kernels (every slot's length must be <= L), past that
// decode_splits(L) splits plus the combine.  ws: dec_attn_b_ws_floats(nseq, H, hd) floats, the caller's.
int dec_attn_decode_b(const void* q, long ldq, const void* k, const void* v, long ldkv, long seq_stride, int L,
                      int nseq, int H, int KVH, int hd, float scale, void* out, long ldo, const int32_t* st,
                      float* ws, hipStream_t s) {
  if (nseq < 1 || nseq > kMaxSeqs || L <= 0 || H <= 0 || KVH <= 0 || H % KVH || hd <= 0 || hd % 64 || hd > 256 ||
      ldkv % 8 || ldkv < (long)KVH * hd || ldq % 8 || ldq < (long)H * hd || ldo < (long)H * hd || seq_stride % 8 ||
      ((uintptr_t)k | (uintptr_t)v | (uintptr_t)q) % 16 || !st || !ws)
    return (int)hipErrorInvalidValue;
  const int grp = H / KVH;
  const int S = decode_splits(L);
  const bool grouped = (hd == 64 || hd == 128 || hd == 256) && (grp == 1 || grp == 2 || grp == 4 || grp == 8);
  const uint16_t *qq = (const uint16_t*)q, *kk = (const uint16_t*)k, *vv = (const uint16_t*)v;
  uint16_t* oo = (uint16_t*)out;
  const long wss = (long)H * kMaxSplits * (hd + 2);
  const unsigned ns = (unsigned)nseq;
  if (S > 1) {
    if (grouped && ((L + S - 1) / S + 63) / 64 * 64 <= kSmallL) {
      with_d_g(hd / 64, grp, [&](auto D, auto G) {
        if constexpr (D() != 3)
          hipLaunchKernelGGL((k_attn_decode_g_b<D(), G(), true>), dim3((unsigned)KVH, (unsigned)S, ns), dim3(256), 0, s,
                             qq, ldq, kk, vv, ldkv, seq_stride, scale, (uint16_t*)nullptr, 0L, st, ws, wss);
      });
    } else {
      const int wg = (grp == 2 || grp == 4 || grp == 8) ? grp : 1;
      with_d_g(hd / 64, wg, [&](auto D, auto G) {
        hipLaunchKernelGGL((k_attn_decode_split_b<D(), G()>), dim3((unsigned)(H / G()), (unsigned)S, ns),
                           dim3(kSplitWaves * 64), 0, s, qq, ldq, kk, vv, ldkv, seq_stride, grp, scale, ws, wss, st);
      });
    }
    hipLaunchKernelGGL(k_attn_combine_b, dim3((unsigned)H, 1, ns), dim3(256), 0, s, ws, wss, S, hd, oo, ldo, st);
  } else if (grouped && L <= kSmallL) {
    with_d_g(hd / 64, grp, [&](auto D, auto G) {
      if constexpr (D() != 3)
        hipLaunchKernelGGL((k_attn_decode_g_b<D(), G(), false>), dim3((unsigned)KVH, 1, ns), dim3(256), 0, s, qq, ldq,
                           kk, vv, ldkv, seq_stride, scale, oo, ldo, st, (float*)nullptr, 0L);
    });
  } else {
    with_d(hd / 64, [&](auto D) {
      hipLaunchKernelGGL(k_attn_decode_b<D()>, dim3((unsigned)H, 1, ns), dim3(kDecWaves * 64), 0, s, qq, ldq, kk, vv,
                         ldkv, seq_stride, grp, hd, scale, oo, ldo, st);
    });
  }
  return (int)hipGetLastError();
}

// floats of the workspace dec_sample_b needs (one dec_sample_ws workspace per slot)
long dec_sample_b_ws_floats(int nseq) { return (long)nseq * SB_FLOATS; }

// The device sampler for every active slot in one chain: logits fp32 rows [nseq, ldl]; slot b draws
// u = splitmix64(seed_b, step_b) from its own record and gets exactly the token dec_sample_ws draws from the
// same row, mask, top_p, temp, seed and draw index; token, pos += inc_pos and step += 1 are written back.
// host_tok: int32 [nseq] (pinned, may be null), -1 for an inactive slot.
int dec_sample_b(const float* logits, long ldl, int nseq, int V, const uint8_t* mask, float top_p, float temp,
                 int32_t* st, int inc_pos, int32_t* host_tok, float* ws, hipStream_t s) {
  if (nseq < 1 || nseq > kMaxSeqs || V <= 0 || ldl < V || !ws || !st) return (int)hipErrorInvalidValue;
  const unsigned ns = (unsigned)nseq;
  if (V <= kSampThreads * kSampRegs) {
    hipLaunchKernelGGL(k_sample_reg_b, dim3(ns), dim3(kSampThreads), 0, s, logits, ldl, V, mask, top_p, temp, st,
                       inc_pos, host_tok);
    return (int)hipGetLastError();
  }
  const dim3 g(kSbBlocks, ns), b(kSbThreads), one(1, ns);
  hipLaunchKernelGGL(k_sb_max_b, g, b, 0, s, logits, ldl, V, mask, ws, (const int32_t*)st);
  const int nucleus = top_p < 1.f;
  if (nucleus) {
    hipLaunchKernelGGL(k_sb_hist_b<0>, g, b, 0, s, logits, ldl, V, mask, ws, (const int32_t*)st);
    hipLaunchKernelGGL(k_sb_select_b<0>, one, dim3(kSbBins), 0, s, top_p, ws, (const int32_t*)st);
    hipLaunchKernelGGL(k_sb_hist_b<1>, g, b, 0, s, logits, ldl, V, mask, ws, (const int32_t*)st);
    hipLaunchKernelGGL(k_sb_select_b<1>, one, dim3(kSbBins), 0, s, top_p, ws, (const int32_t*)st);
  }
  hipLaunchKernelGGL(k_sb_part_b, g, b, 0, s, logits, ldl, V, mask, temp, nucleus, ws, (const int32_t*)st);
  hipLaunchKernelGGL(k_sb_draw_b, one, dim3(kSbBins), 0, s, logits, ldl, V, mask, temp, (const float*)ws, st, inc_pos,
                     host_tok);
  return (int)hipGetLastError();
}

}  // extern "C"
