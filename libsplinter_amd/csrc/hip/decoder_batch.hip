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
// The slot-indexed kernels are copies of the single-sequence bodies, not shared functions: folding two
// kernels' bodies into one function moved the register allocation of 8 single-sequence kernels
// (profiles/decoder_prune/README.md), and those stay exactly as they are.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <type_traits>

#include "decoder_common.hpp"

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
  const int half = hd >> 1;
  const int npairs = (H + KVH) * half;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npairs + KVH * hd; i += gridDim.x * blockDim.x) {
    if (i < npairs) {
      const int head = i / half, j = i - head * half;
      uint16_t* ptr = qkv + (long)head * hd + 2 * j;
      const float a = bf2f(ptr[0]), b = bf2f(ptr[1]);
      const float c = cs[p * half + j], s = sn[p * half + j];
      const uint16_t y0 = __builtin_bit_cast(uint16_t, (__bf16)(a * c - b * s));
      const uint16_t y1 = __builtin_bit_cast(uint16_t, (__bf16)(a * s + b * c));
      if (head < H) {
        ptr[0] = y0;
        ptr[1] = y1;
      } else {
        uint16_t* kr = kc + p * ldkv + (long)(head - H) * hd + 2 * j;
        kr[0] = y0;
        kr[1] = y1;
      }
    } else {
      const int e = i - npairs;
      vc[p * ldkv + e] = qkv[(long)(H + KVH) * hd + e];
    }
  }
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

// k_attn_decode: one 1024-thread workgroup per query head, 16 waves over interleaved 64-key chunks
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
  const int h = blockIdx.x;
  const int kvh = h / grp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __shared__ float qs[256];
  __shared__ float wm[kDecWaves], wl[kDecWaves];
  __shared__ float wacc[kDecWaves][256];
  for (int d = threadIdx.x; d < hd; d += kDecWaves * 64) qs[d] = bf2f(q[(long)h * hd + d]) * scale;
  __syncthreads();
  const uint16_t* Kb = K + (long)kvh * hd;
  const uint16_t* Vb = V + (long)kvh * hd + lane * DPL;
  float m = -INFINITY, l = 0.f, acc[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
  for (int base = wave * 64; base < L; base += kDecWaves * 64) {
    const int j = base + lane;
    float s = -INFINITY;
    if (j < L) {
      const uint16_t* kr = Kb + (long)j * ldkv;
      float dot = 0.f;
#pragma unroll 1
      for (int cb = 0; cb < DPL; ++cb) {
        uint4 kv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) kv[c] = *(const uint4*)(kr + cb * 64 + c * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          float f[8];
          unpack8(kv[c], f);
#pragma unroll
          for (int e = 0; e < 8; ++e) dot += f[e] * qs[cb * 64 + c * 8 + e];
        }
      }
      s = dot;
    }
    float cm = s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
    const float mn = fmaxf(m, cm);  // finite: lane 0 of every visited chunk holds a key
    const float corr = __expf(m - mn);
    const float p = j < L ? __expf(s - mn) : 0.f;
    float ps = p;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
    l = l * corr + ps;
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[i] *= corr;
    const int nv = min(64, L - base);
    for (int t = 0; t < nv; ++t) {
      const float pt = __shfl(p, t, 64);
      const uint16_t* vr = Vb + (long)(base + t) * ldkv;
#pragma unroll
      for (int i = 0; i < DPL; ++i) acc[i] += pt * bf2f(vr[i]);
    }
    m = mn;
  }
  if (lane == 0) { wm[wave] = m; wl[wave] = l; }
#pragma unroll
  for (int i = 0; i < DPL; ++i) wacc[wave][lane * DPL + i] = acc[i];
  __syncthreads();
  float M = wm[0];
#pragma unroll
  for (int w = 1; w < kDecWaves; ++w) M = fmaxf(M, wm[w]);
  float c[kDecWaves], den = 0.f;
#pragma unroll
  for (int w = 0; w < kDecWaves; ++w) {
    c[w] = wm[w] == -INFINITY ? 0.f : __expf(wm[w] - M);  // a wave past the slot's keys adds nothing
    den += wl[w] * c[w];
  }
  const float inv = 1.f / den;
  for (int d = threadIdx.x; d < hd; d += kDecWaves * 64) {
    float o = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) o += wacc[w][d] * c[w];
    o *= inv;
    out[(long)h * hd + d] = __builtin_bit_cast(uint16_t, (__bf16)o);
  }
}

// k_attn_decode_g: one workgroup per KV head serves its G query heads (scores, softmax, P V); SPLIT: one
// split of the flash-decoding form, partials to ws for k_attn_combine_b
template <int D, int G, bool SPLIT>
__global__ __launch_bounds__(256) void k_attn_decode_g_b(const uint16_t* __restrict__ q_, long ldq,
                                                         const uint16_t* __restrict__ K_,
                                                         const uint16_t* __restrict__ V_, long ldkv, long seq_stride,
                                                         float scale, uint16_t* __restrict__ out_, long ldo,
                                                         const int32_t* __restrict__ st, float* __restrict__ ws_,
                                                         long ws_stride) {
  constexpr int hd = 64 * D, TPK = hd / 8, KP = 256 / TPK, U = 8;
  static_assert(64 % TPK == 0, "a key row's lanes must sit in one wave");
  AttnSlot sl{q_, K_, V_, out_, ws_, 0};
  if (!attn_slot(sl, st, ldq, seq_stride, ldo, ws_stride)) return;
  const uint16_t *q = sl.q, *K = sl.K, *V = sl.V;
  uint16_t* out = sl.out;
  float* ws = sl.ws;
  const int L = sl.L;
  int k0 = 0, k1 = L < kSmallL ? L : kSmallL;
  if constexpr (SPLIT) {
    const int S = gridDim.y, chunk = ((L + S - 1) / S + 63) / 64 * 64;
    k0 = blockIdx.y * chunk;
    k1 = min(L, k0 + min(chunk, kSmallL));  // the host guarantees chunk <= kSmallL
  }
  const int n = k1 > k0 ? k1 - k0 : 0;
  const int kvh = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int sub = tid % TPK, kg = tid / TPK;
  __shared__ float sc[G][kSmallL];
  __shared__ float red[KP][G][hd];
  __shared__ float lsum[G], lmax[G];
  float qv[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float f[8];
    unpack8(*(const uint4*)(q + (long)(kvh * G + g) * hd + sub * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[g][e] = f[e] * scale;
  }
  const uint16_t* Kb = K + (long)kvh * hd + sub * 8 + (long)k0 * ldkv;
  const uint16_t* Vb = V + (long)kvh * hd + sub * 8 + (long)k0 * ldkv;
  // ---- scores
  for (int j0 = 0; j0 < n; j0 += KP * U) {
    uint4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KP + kg;
      r[u] = j < n ? *(const uint4*)(Kb + (long)j * ldkv) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KP + kg;
      float f[8], d[G];
      unpack8(r[u], f);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        d[g] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d[g] = fmaf(f[e], qv[g][e], d[g]);
#pragma unroll
        for (int o = TPK / 2; o >= 1; o >>= 1) d[g] += __shfl_xor(d[g], o, 64);
      }
      if (sub == 0 && j < n) {
#pragma unroll
        for (int g = 0; g < G; ++g) sc[g][j] = d[g];
      }
    }
  }
  __syncthreads();
  // ---- softmax, one wave per head
  for (int g = wave; g < G; g += 4) {
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) mx = fmaxf(mx, sc[g][j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) {
      const float p = __expf(sc[g][j] - mx);
      sc[g][j] = p;
      sum += p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) {
      lsum[g] = sum;
      lmax[g] = mx;
    }
  }
  __syncthreads();
  // ---- P V
  float acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  for (int j0 = 0; j0 < n; j0 += KP * U) {
    uint4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KP + kg;
      r[u] = j < n ? *(const uint4*)(Vb + (long)j * ldkv) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KP + kg;
      if (j < n) {
        float f[8];
        unpack8(r[u], f);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float p = sc[g][j];
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(p, f[e], acc[g][e]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) red[kg][g][sub * 8 + e] = acc[g][e];
  __syncthreads();
  if constexpr (SPLIT) {
    // ws[head][split][hd + 2] = (max, sum, unnormalised P V); an empty split leaves max = -inf, sum 0
    const int S = gridDim.y;
    for (int idx = tid; idx < G * (hd + 2); idx += 256) {
      const int g = idx / (hd + 2), c = idx - g * (hd + 2);
      float v;
      if (c == 0) v = n ? lmax[g] : -INFINITY;
      else if (c == 1) v = n ? lsum[g] : 0.f;
      else {
        v = 0.f;
#pragma unroll 8
        for (int k = 0; k < KP; ++k) v += red[k][g][c - 2];
      }
      ws[((long)(kvh * G + g) * S + blockIdx.y) * (hd + 2) + c] = v;
    }
  } else {
    for (int idx = tid; idx < G * hd; idx += 256) {
      const int g = idx / hd, d = idx - g * hd;
      float o = 0.f;
#pragma unroll 8
      for (int k = 0; k < KP; ++k) o += red[k][g][d];
      out[(long)(kvh * G + g) * hd + d] = __builtin_bit_cast(uint16_t, (__bf16)(o / lsum[g]));
    }
  }
}

// k_attn_decode_split: grid (H / G, S, nseq), 4 waves walk keys [j c, (j + 1) c) of the slot
template <int DPL, int G>
__global__ __launch_bounds__(kSplitWaves * 64) void k_attn_decode_split_b(
    const uint16_t* __restrict__ q_, long ldq, const uint16_t* __restrict__ K_, const uint16_t* __restrict__ V_,
    long ldkv, long seq_stride, int grp, float scale, float* __restrict__ ws_, long ws_stride,
    const int32_t* __restrict__ st) {
  constexpr int hd = 64 * DPL;
  AttnSlot sl{q_, K_, V_, nullptr, ws_, 0};
  if (!attn_slot(sl, st, ldq, seq_stride, 0, ws_stride)) return;
  const uint16_t *q = sl.q, *K = sl.K, *V = sl.V;
  float* ws = sl.ws;
  const int L = sl.L;
  const int h0 = blockIdx.x * G, S = gridDim.y, j = blockIdx.y;
  const int kvh = h0 / grp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int chunk = ((L + S - 1) / S + 63) / 64 * 64;
  const int k0 = j * chunk, k1 = min(L, k0 + chunk);
  __shared__ float qs[G][hd];
  __shared__ float wm[kSplitWaves][G], wl[kSplitWaves][G];
  __shared__ float wacc[kSplitWaves][G][hd];
  for (int d = threadIdx.x; d < G * hd; d += kSplitWaves * 64) qs[d / hd][d % hd] = bf2f(q[(long)h0 * hd + d]) * scale;
  __syncthreads();
  const uint16_t* Kb = K + (long)kvh * hd;
  const uint16_t* Vb = V + (long)kvh * hd + lane * DPL;
  float m[G], l[G], acc[G][DPL];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[g][i] = 0.f;
  }
  for (int base = k0 + wave * 64; base < k1; base += kSplitWaves * 64) {
    const int jj = base + lane;
    float sc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sc[g] = -INFINITY;
    if (jj < k1) {
      const uint16_t* kr = Kb + (long)jj * ldkv;
      float dot[G];
#pragma unroll
      for (int g = 0; g < G; ++g) dot[g] = 0.f;
#pragma unroll 1
      for (int cb = 0; cb < DPL; ++cb) {
        uint4 kv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) kv[c] = *(const uint4*)(kr + cb * 64 + c * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          float f[8];
          unpack8(kv[c], f);
#pragma unroll
          for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) dot[g] += f[e] * qs[g][cb * 64 + c * 8 + e];
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) sc[g] = dot[g];
    }
    float p[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float cm = sc[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
      const float mn = fmaxf(m[g], cm);
      const float corr = __expf(m[g] - mn);
      p[g] = jj < k1 ? __expf(sc[g] - mn) : 0.f;
      float ps = p[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
      l[g] = l[g] * corr + ps;
#pragma unroll
      for (int i = 0; i < DPL; ++i) acc[g][i] *= corr;
      m[g] = mn;
    }
    const int nv = min(64, k1 - base);
    for (int t = 0; t < nv; ++t) {
      const uint16_t* vr = Vb + (long)(base + t) * ldkv;
      float vv[DPL];
#pragma unroll
      for (int i = 0; i < DPL; ++i) vv[i] = bf2f(vr[i]);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pt = __shfl(p[g], t, 64);
#pragma unroll
        for (int i = 0; i < DPL; ++i) acc[g][i] += pt * vv[i];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (lane == 0) { wm[wave][g] = m[g]; wl[wave][g] = l[g]; }
#pragma unroll
    for (int i = 0; i < DPL; ++i) wacc[wave][g][lane * DPL + i] = acc[g][i];
  }
  __syncthreads();
  for (int g = 0; g < G; ++g) {
    float M = wm[0][g];
#pragma unroll
    for (int w = 1; w < kSplitWaves; ++w) M = fmaxf(M, wm[w][g]);
    float* o = ws + ((long)(h0 + g) * S + j) * (hd + 2);
    float c[kSplitWaves], den = 0.f;
#pragma unroll
    for (int w = 0; w < kSplitWaves; ++w) {
      c[w] = wm[w][g] == -INFINITY ? 0.f : __expf(wm[w][g] - M);  // an empty wave (or split) adds nothing
      den += wl[w][g] * c[w];
    }
    for (int d = threadIdx.x; d < hd; d += kSplitWaves * 64) {
      float a = 0.f;
#pragma unroll
      for (int w = 0; w < kSplitWaves; ++w) a += wacc[w][g][d] * c[w];
      o[2 + d] = a;
    }
    if (threadIdx.x == 0) { o[0] = M; o[1] = den; }
  }
}

// out[b][h] = sum_j acc_j e^(m_j - M) / sum_j l_j e^(m_j - M) over the S partials of head h of slot b
__global__ void k_attn_combine_b(const float* __restrict__ ws, long ws_stride, int S, int hd,
                                 uint16_t* __restrict__ out, long ldo, const int32_t* __restrict__ st) {
  const int b = blockIdx.z;
  if (!st[b * ST_WORDS + ST_ACTIVE]) return;
  const int h = blockIdx.x;
  const float* p = ws + b * ws_stride + (long)h * S * (hd + 2);
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
  if (d < hd) out[b * ldo + (long)h * hd + d] = __builtin_bit_cast(uint16_t, (__bf16)(a / den));
}

// ------------------------------------------------------------------ sampler --
// k_sample_reg and the k_sb_* chain with a slot index: slot b samples logits row b with the seed and the
// draw index of its own record and its own workspace slice; the arithmetic is the single-sequence
// kernels', statement for statement, so a slot draws the token dec_sample_ws draws from the same inputs.
__device__ __forceinline__ uint64_t slot_seed(const int32_t* sb) {
  return (uint64_t)(uint32_t)sb[ST_SEED_LO] | ((uint64_t)(uint32_t)sb[ST_SEED_HI] << 32);
}
__device__ __forceinline__ void slot_commit(int32_t* sb, int t, int inc_pos, int32_t* host_tok) {
  sb[ST_TOK] = t;
  sb[ST_POS] += inc_pos;
  sb[ST_STEP] += 1;
  if (host_tok) __hip_atomic_store(host_tok, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(kSampThreads) void k_sample_reg_b(const float* __restrict__ logits_, long ldl, int V,
                                                               const uint8_t* __restrict__ mask, float top_p,
                                                               float temp, int32_t* __restrict__ st_, int inc_pos,
                                                               int32_t* host_tok_) {
  __shared__ float sh[kSampThreads / 64];
  __shared__ float scan[kSampThreads];
  __shared__ float hist[kSampThreads];
  __shared__ float hist8[kSampThreads * 8];
  __shared__ int jstar, pick;
  const int tid = threadIdx.x;
  int32_t* st = st_ + blockIdx.x * ST_WORDS;
  int32_t* host_tok = host_tok_ ? host_tok_ + blockIdx.x : nullptr;
  if (!st[ST_ACTIVE]) {
    if (tid == 0 && host_tok) __hip_atomic_store(host_tok, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const float* logits = logits_ + blockIdx.x * ldl;
  const uint64_t seed = slot_seed(st);
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
  float lo = M - 40.f;
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
  if (tid == 0) slot_commit(st, pick, inc_pos, host_tok);
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
}

template <int LEVEL>
__global__ __launch_bounds__(kSbThreads) void k_sb_hist_b(const float* __restrict__ logits_, long ldl, int V,
                                                          const uint8_t* __restrict__ mask, float* __restrict__ ws_,
                                                          const int32_t* __restrict__ st) {
  SB_SLOT(logits_, ws_);
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
}

template <int LEVEL>
__global__ __launch_bounds__(kSbBins) void k_sb_select_b(float top_p, float* __restrict__ ws_,
                                                         const int32_t* __restrict__ st) {
  if (!st[blockIdx.y * ST_WORDS + ST_ACTIVE]) return;
  float* ws = ws_ + (long)blockIdx.y * SB_FLOATS;
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
}

__global__ __launch_bounds__(kSbThreads) void k_sb_part_b(const float* __restrict__ logits_, long ldl, int V,
                                                          const uint8_t* __restrict__ mask, float temp, int nucleus,
                                                          float* __restrict__ ws_, const int32_t* __restrict__ st) {
  SB_SLOT(logits_, ws_);
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
}

__global__ __launch_bounds__(kSbBins) void k_sb_draw_b(const float* __restrict__ logits_, long ldl, int V,
                                                       const uint8_t* __restrict__ mask, float temp,
                                                       const float* __restrict__ ws_, int32_t* __restrict__ st_,
                                                       int inc_pos, int32_t* host_tok_) {
  __shared__ float scan[kSbBins];
  __shared__ int pick;
  __shared__ float base_u;
  __shared__ int blk;
  const int tid = threadIdx.x;
  int32_t* st = st_ + blockIdx.y * ST_WORDS;
  int32_t* host_tok = host_tok_ ? host_tok_ + blockIdx.y : nullptr;
  if (!st[ST_ACTIVE]) {
    if (tid == 0 && host_tok) __hip_atomic_store(host_tok, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const float* logits = logits_ + blockIdx.y * ldl;
  const float* ws = ws_ + (long)blockIdx.y * SB_FLOATS;
  const uint64_t seed = slot_seed(st);
  const float M = ws[SB_SCAL + 0], cut = ws[SB_SCAL + 5];
  const float it = 1.f / fmaxf(temp, 1e-6f);
  if (tid == 0) {
    double total = 0.0;
    for (int b = 0; b < kSbBlocks; ++b) total += ws[SB_BPART + b];
    const double u = uniform01(seed, (uint64_t)st[ST_STEP]) * total;
    double run = 0.0;
    int bb = -1;
    for (int b = 0; b < kSbBlocks; ++b) {
      const double p = ws[SB_BPART + b];
      if (p > 0.0) {
        if (u < run + p) { bb = b; break; }
        bb = b;  // rounding at the very end: the last block with mass
      }
      run += p;
    }
    if (bb >= 0 && u >= run + ws[SB_BPART + bb]) run -= ws[SB_BPART + bb];
    blk = bb;
    base_u = (float)(u - run);
    pick = 0x7fffffff;
  }
  __syncthreads();
  const int chunk = (V + kSbBlocks - 1) / kSbBlocks;
  if (blk >= 0) {
    const int b0 = blk * chunk, b1 = min(V, b0 + chunk);
    const int per = (b1 - b0 + kSbBins - 1) / kSbBins;
    const int t0 = b0 + tid * per, t1 = min(b1, t0 + per);
    float part = 0.f;
    for (int i = t0; i < t1; ++i) {
      const float l = sb_logit(logits, mask, i);
      if (l >= cut) part += __expf((l - M) * it);
    }
    scan[tid] = part;
    __syncthreads();
    for (int off = 1; off < kSbBins; off <<= 1) {
      const float x = tid >= off ? scan[tid - off] : 0.f;
      __syncthreads();
      scan[tid] += x;
      __syncthreads();
    }
    const float u = base_u, before = tid ? scan[tid - 1] : 0.f;
    if (part > 0.f && u >= before && (u < scan[tid] || tid == kSbBins - 1 || scan[tid] >= scan[kSbBins - 1])) {
      float run = before;
      int sel = -1;
      for (int i = t0; i < t1; ++i) {
        const float l = sb_logit(logits, mask, i);
        if (l < cut) continue;
        sel = i;
        run += __expf((l - M) * it);
        if (u < run) break;
      }
      if (sel >= 0) atomicMin(&pick, sel);
    }
    __syncthreads();
  }
  if (tid == 0) {
    int t = pick;
    if (t == 0x7fffffff) {  // rounding gap: the most probable token (first block holding the max)
      for (int b = 0; b < kSbBlocks; ++b)
        if (ws[SB_BMAX + b] == M) { t = __float_as_int(ws[SB_BIDX + b]); break; }
    }
    slot_commit(st, t, inc_pos, host_tok);
  }
}
#undef SB_SLOT

// ------------------------------------------------------------------ host dispatch --
template <int V>
using ic = std::integral_constant<int, V>;

template <class F>
void with_d(int d, F f) {
  switch (d) {
    case 1: f(ic<1>{}); break;
    case 2: f(ic<2>{}); break;
    case 3: f(ic<3>{}); break;
    default: f(ic<4>{}); break;
  }
}
template <class F>
void with_d_g(int d, int g, F f) {
  with_d(d, [&](auto D) {
    switch (g) {
      case 2: f(D, ic<2>{}); break;
      case 4: f(D, ic<4>{}); break;
      case 8: f(D, ic<8>{}); break;
      default: f(D, ic<1>{}); break;
    }
  });
}

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
