// decoder_arch.hip — the fused q/k preparation step of the decoder architectures that put more than a
// rotation between the qkv projection and attention: qwen2 (a bias on q, k and v) and qwen3 (a per-head
// RMSNorm on q and k).  One launch stands where the llama path has its RoPE (+ cache append) launch:
//   dec_qk_prep          rows [T, ld] at positions pos0 + t, q / k / v transformed in place   (dec_rope)
//   dec_qk_prep_kv       one row at the device state's position, k / v appended to the cache   (dec_rope_kv)
//   dec_qk_prep_kv_b     one row per active sequence slot                                      (dec_rope_kv_b)
//   dec_qk_prep_kv_seg   the packed rows of a batched prefill pass, by-value segment table     (dec_rope_kv_seg)
// A head is one wave's work (prep_head): bf16 GEMM output -> fp32, + bias, x rsqrt(mean(x^2) + eps) x norm
// weight, the adjacent-pair rotation at the row's position, ONE rounding to bf16.  A lane owns one whole
// rotation pair (lanes 0 .. hd/2 - 1; head dim 64 leaves the upper half of the wave idle), the sum of
// squares is the wave's xor-shuffle butterfly: no LDS, no atomics.  The v columns get the bias and go to
// their place in 16-byte pieces.  All four kernels run the same prep_item on a (row, head | v piece), with
// floating-point contraction off, so the same input row, position and weights give the same bits whichever
// entry point computed them -- what batched decode, chunked prefill and the prefix cache rely on.
// The NeoX half rotation of these architectures is not a kernel concern: the loader permutes the q / k
// rows of each head (models/decoder.py), after which adjacent pairs are the file's (j, j + hd/2) pairs.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "decoder_common.hpp"

namespace {

constexpr int kPrepMaxSeqs = 16;  // sequence slots of the batched step (decoder_batch.hip kMaxSeqs)

// what every form needs beside its rows: fp32 bias [(H + 2 KVH) hd] (BIAS), fp32 norm weights [hd] for q and
// k (NORM), the fp32 cos / sin tables [n_ctx, hd / 2]
struct PrepArgs {
  const float *bias, *qn, *kn, *cs, *sn;
  float eps;
  int H, KVH;
};

// one head: src -> dst (hd bf16 each; dst may be src), bias / nw / cs / sn at the head's first element
template <int HD, bool BIAS, bool NORM>
__device__ __forceinline__ void prep_head(const uint16_t* src, const float* bias, const float* nw, float eps,
                                          const float* cs, const float* sn, uint16_t* dst, int lane) {
#pragma clang fp contract(off)
  const bool on = lane < HD / 2;
  float a = 0.f, b = 0.f;
  if (on) {
    const uint32_t v = *(const uint32_t*)(src + 2 * lane);
    a = bf2f(v & 0xffff);
    b = bf2f(v >> 16);
    if constexpr (BIAS) {
      const float2 bb = *(const float2*)(bias + 2 * lane);
      a = a + bb.x;
      b = b + bb.y;
    }
  }
  if constexpr (NORM) {
    const float ss = wave_sum(a * a + b * b);
    const float rs = rsqrtf(ss / (float)HD + eps);
    if (on) {
      const float2 w = *(const float2*)(nw + 2 * lane);
      a = a * rs * w.x;
      b = b * rs * w.y;
    }
  }
  if (on) {
    const float c = cs[lane], s = sn[lane];
    *(uint32_t*)(dst + 2 * lane) = pk2(a * c - b * s, a * s + b * c);
  }
}

// work item `item` of a row (uniform over the wave): a q head, a k head, or 64 16-byte pieces of v.
// row: the qkv row; p: its position; qdst / kdst / vdst: where its q, k and v columns go
template <int HD, bool BIAS, bool NORM>
__device__ __forceinline__ void prep_item(const PrepArgs& a, const uint16_t* row, int item, long p, uint16_t* qdst,
                                          uint16_t* kdst, uint16_t* vdst, int lane) {
#pragma clang fp contract(off)
  const int H = a.H, KVH = a.KVH;
  const float* cs = a.cs + p * (HD / 2);
  const float* sn = a.sn + p * (HD / 2);
  if (item < H) {
    prep_head<HD, BIAS, NORM>(row + item * HD, a.bias + item * HD, a.qn, a.eps, cs, sn, qdst + item * HD, lane);
  } else if (item < H + KVH) {
    prep_head<HD, BIAS, NORM>(row + item * HD, a.bias + item * HD, a.kn, a.eps, cs, sn, kdst + (item - H) * HD, lane);
  } else {
    const int e = ((item - H - KVH) * 64 + lane) * 8;
    if (e >= KVH * HD) return;
    const int col = (H + KVH) * HD + e;
    uint4 v = *(const uint4*)(row + col);
    if constexpr (BIAS) {
      float f[8];
      unpack8(v, f);
      const float4 b0 = *(const float4*)(a.bias + col), b1 = *(const float4*)(a.bias + col + 4);
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = f[i] + bb[i];
      v = pack8(f);
    }
    *(uint4*)(vdst + e) = v;
  }
}

// waves of 64 v pieces per row
__host__ __device__ inline int prep_v_waves(int KVH, int hd) { return (KVH * hd / 8 + 63) / 64; }

// rows [T, ld] in place; W work items per row (without the v waves when there is no bias: v stays as it is)
template <int HD, bool BIAS, bool NORM>
__global__ __launch_bounds__(256) void k_qk_prep(uint16_t* __restrict__ qkv, long ld, long T, int pos0, int W,
                                                 PrepArgs a) {
  const long gw = blockIdx.x * 4L + (threadIdx.x >> 6);
  const long t = gw / W;
  if (t >= T) return;
  uint16_t* row = qkv + t * ld;
  prep_item<HD, BIAS, NORM>(a, row, (int)(gw - t * W), pos0 + t, row, row + a.H * HD, row + (a.H + a.KVH) * HD,
                            threadIdx.x & 63);
}

// the step's row at position state.pos: q in place, k / v to row pos of the layer's cache
template <int HD, bool BIAS, bool NORM>
__global__ __launch_bounds__(256) void k_qk_prep_kv(uint16_t* __restrict__ qkv, const int32_t* __restrict__ st,
                                                    uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, long ldkv,
                                                    int W, PrepArgs a) {
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= W) return;
  const long p = st[ST_POS];
  prep_item<HD, BIAS, NORM>(a, qkv, item, p, qkv, kc + p * ldkv, vc + p * ldkv, threadIdx.x & 63);
}

// k_qk_prep_kv per slot (blockIdx.y): row b of qkv, the slot's cache at + b * seq_stride
template <int HD, bool BIAS, bool NORM>
__global__ __launch_bounds__(256) void k_qk_prep_kv_b(uint16_t* __restrict__ qkv, long ldq,
                                                      const int32_t* __restrict__ st, uint16_t* __restrict__ kc,
                                                      uint16_t* __restrict__ vc, long ldkv, long seq_stride, int W,
                                                      PrepArgs a) {
  const int32_t* sb = st + blockIdx.y * ST_WORDS;
  if (!sb[ST_ACTIVE]) return;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= W) return;
  const long p = sb[ST_POS];
  uint16_t* row = qkv + blockIdx.y * ldq;
  const long off = blockIdx.y * seq_stride + p * ldkv;
  prep_item<HD, BIAS, NORM>(a, row, item, p, row, kc + off, vc + off, threadIdx.x & 63);
}

// a batched prefill pass: blockIdx.y is a segment of the by-value table; row row0 + r at position pos0 + r,
// q in place, k / v to cache row pos0 + r of the segment's slot.  The k / v columns of qkv stay as they are.
template <int HD, bool BIAS, bool NORM>
__global__ __launch_bounds__(256) void k_qk_prep_kv_seg(uint16_t* __restrict__ qkv, long ld,
                                                        uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
                                                        long ldkv, int W, PrepArgs a, PrefillSegs tb) {
  const PrefillSeg sg = prefill_seg_at(tb, blockIdx.y);
  const long gw = blockIdx.x * 4L + (threadIdx.x >> 6);
  const long r = gw / W;
  if (r >= sg.n) return;
  const long p = sg.pos0 + r;
  uint16_t* row = qkv + (sg.row0 + r) * ld;
  const long off = (long)sg.slot * tb.seq_stride + p * ldkv;
  prep_item<HD, BIAS, NORM>(a, row, (int)(gw - r * W), p, row, kc + off, vc + off, threadIdx.x & 63);
}

template <bool V>
using bc = std::integral_constant<bool, V>;

// f(ic<hd>, bc<bias>, bc<norm>) for the head dim and flags of a call; the caller has checked them
template <class F>
void with_prep(int hd, bool bias, bool norm, F f) {
  auto flags = [&](auto HD) {
    if (bias && norm) f(HD, bc<true>{}, bc<true>{});
    else if (bias) f(HD, bc<true>{}, bc<false>{});
    else f(HD, bc<false>{}, bc<true>{});
  };
  if (hd == 64) flags(ic<64>{});
  else flags(ic<128>{});
}

// the checks every form shares: head dim 64 / 128, a bias or both norm weights (or all three), the tables,
// 16-byte alignment of every pointer
bool prep_ok(int H, int KVH, int hd, const float* cs, const float* sn, const float* bias, const float* qn,
             const float* kn) {
  if (H <= 0 || KVH <= 0 || H % KVH || (hd != 64 && hd != 128) || !cs || !sn) return false;
  if ((qn == nullptr) != (kn == nullptr) || (!bias && !qn)) return false;
  return !(((uintptr_t)cs | (uintptr_t)sn | (uintptr_t)bias | (uintptr_t)qn | (uintptr_t)kn) & 15);
}

}  // namespace

extern "C" {

// qkv: bf16 [T, ld] rows of (H + 2 KVH) hd; row t has position pos0 + t (the caller guarantees
// pos0 + T <= n_ctx of the cos / sin tables).  bias: fp32 [(H + 2 KVH) hd] or null; qn / kn: fp32 [hd] norm
// weights of q and k, both or neither; at least one of bias and the norms.  In place: q and k columns biased,
// normalised and rotated, v columns biased (untouched without a bias).
int dec_qk_prep(void* qkv, long ld, long T, int H, int KVH, int hd, int pos0, const float* cos_tab,
                const float* sin_tab, const float* bias, const float* qn, const float* kn, float eps, hipStream_t s) {
  if (T <= 0) return 0;
  if (!prep_ok(H, KVH, hd, cos_tab, sin_tab, bias, qn, kn) || !qkv || (uintptr_t)qkv & 15 || ld % 8 ||
      ld < (long)(H + 2 * KVH) * hd || pos0 < 0)
    return (int)hipErrorInvalidValue;
  const int W = H + KVH + (bias ? prep_v_waves(KVH, hd) : 0);
  const long g = (T * W + 3) / 4;
  if (g > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const PrepArgs a{bias, qn, kn, cos_tab, sin_tab, eps, H, KVH};
  with_prep(hd, bias != nullptr, qn != nullptr, [&](auto HD, auto B, auto N) {
    hipLaunchKernelGGL((k_qk_prep<HD(), B(), N()>), dim3((unsigned)g), dim3(256), 0, s, (uint16_t*)qkv, ld, T, pos0, W,
                       a);
  });
  return (int)hipGetLastError();
}

// qkv: bf16 [(H + 2 KVH) hd] of the step's token; kc / vc: the layer's cache [n_ctx, ldkv]; st: the device
// state (position = st[0]).  q in place, prepared k and biased v to cache row pos; the k / v columns of qkv
// stay as they are.
int dec_qk_prep_kv(void* qkv, int H, int KVH, int hd, const float* cos_tab, const float* sin_tab, const int32_t* st,
                   void* kc, void* vc, long ldkv, const float* bias, const float* qn, const float* kn, float eps,
                   hipStream_t s) {
  if (!prep_ok(H, KVH, hd, cos_tab, sin_tab, bias, qn, kn) || !qkv || !st || !kc || !vc ||
      ((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc) & 15 || ldkv % 8 || ldkv < (long)KVH * hd)
    return (int)hipErrorInvalidValue;
  const int W = H + KVH + prep_v_waves(KVH, hd);
  const PrepArgs a{bias, qn, kn, cos_tab, sin_tab, eps, H, KVH};
  with_prep(hd, bias != nullptr, qn != nullptr, [&](auto HD, auto B, auto N) {
    hipLaunchKernelGGL((k_qk_prep_kv<HD(), B(), N()>), dim3((unsigned)((W + 3) / 4)), dim3(256), 0, s, (uint16_t*)qkv,
                       st, (uint16_t*)kc, (uint16_t*)vc, ldkv, W, a);
  });
  return (int)hipGetLastError();
}

// qkv: bf16 rows [nseq, ldq]; kc / vc: slot 0's layer cache [n_ctx, ldkv], slot b's at + b * seq_stride
// elements; st: one 8-word record per slot.  Active slot b: dec_qk_prep_kv on its row at st[b].pos; an
// inactive slot's row and cache are not touched.
int dec_qk_prep_kv_b(void* qkv, long ldq, int nseq, int H, int KVH, int hd, const float* cos_tab,
                     const float* sin_tab, const int32_t* st, void* kc, void* vc, long ldkv, long seq_stride,
                     const float* bias, const float* qn, const float* kn, float eps, hipStream_t s) {
  if (!prep_ok(H, KVH, hd, cos_tab, sin_tab, bias, qn, kn) || nseq < 1 || nseq > kPrepMaxSeqs || !qkv || !st ||
      !kc || !vc || ((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc) & 15 || ldq % 8 || ldkv % 8 || seq_stride % 8 ||
      ldq < (long)(H + 2 * KVH) * hd || ldkv < (long)KVH * hd)
    return (int)hipErrorInvalidValue;
  const int W = H + KVH + prep_v_waves(KVH, hd);
  const PrepArgs a{bias, qn, kn, cos_tab, sin_tab, eps, H, KVH};
  with_prep(hd, bias != nullptr, qn != nullptr, [&](auto HD, auto B, auto N) {
    hipLaunchKernelGGL((k_qk_prep_kv_b<HD(), B(), N()>), dim3((unsigned)((W + 3) / 4), (unsigned)nseq), dim3(256), 0,
                       s, (uint16_t*)qkv, ldq, st, (uint16_t*)kc, (uint16_t*)vc, ldkv, seq_stride, W, a);
  });
  return (int)hipGetLastError();
}

// qkv: packed bf16 rows [T, ldq]; segs: HOST int32 [nseg][4] = {row0, n, pos0, slot}, checked and passed by
// value as dec_rope_kv_seg does (hipErrorInvalidValue and nothing launched when a check fails); kc / vc:
// slot 0's layer cache [n_ctx, ldkv], slot b's at + b * seq_stride elements.  Row row0 + r of a segment:
// dec_qk_prep_kv at position pos0 + r into the segment's slot.
int dec_qk_prep_kv_seg(void* qkv, long ldq, long T, const int32_t* segs, int nseg, int H, int KVH, int hd,
                       const float* cos_tab, const float* sin_tab, void* kc, void* vc, long ldkv, long seq_stride,
                       int nslots, int n_ctx, const float* bias, const float* qn, const float* kn, float eps,
                       hipStream_t s) {
  PrefillSegs tb;
  if (!prep_ok(H, KVH, hd, cos_tab, sin_tab, bias, qn, kn) || !qkv || !kc || !vc ||
      ((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc) & 15 || ldq % 8 || ldkv % 8 || seq_stride % 8 ||
      ldq < (long)(H + 2 * KVH) * hd || ldkv < (long)KVH * hd || seq_stride < (long)n_ctx * ldkv ||
      !prefill_segs_build(segs, nseg, T, nslots, n_ctx, seq_stride, tb))
    return (int)hipErrorInvalidValue;
  int nmax = 0;
  for (int i = 0; i < tb.nseg; ++i) nmax = tb.n[i] > nmax ? tb.n[i] : nmax;
  const int W = H + KVH + prep_v_waves(KVH, hd);
  const long g = ((long)nmax * W + 3) / 4;
  if (g > 0x7fffffffL) return (int)hipErrorInvalidValue;
  const PrepArgs a{bias, qn, kn, cos_tab, sin_tab, eps, H, KVH};
  with_prep(hd, bias != nullptr, qn != nullptr, [&](auto HD, auto B, auto N) {
    hipLaunchKernelGGL((k_qk_prep_kv_seg<HD(), B(), N()>), dim3((unsigned)g, (unsigned)tb.nseg), dim3(256), 0, s,
                       (uint16_t*)qkv, ldq, (uint16_t*)kc, (uint16_t*)vc, ldkv, W, a, tb);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
