// decoder_moe.hip — mixture-of-experts feed-forward for the completion decoder (qwen3moe, mixtral):
//   dec_moe_route      router logits -> top-k expert ids and their renormalised weights, on the device
//   dec_gemv_moe*      the decode step's up|gate GEMV + SwiGLU on the k experts a device-side id names
//   dec_gemv_moe_down* the k down GEMVs, weighted, summed and added to the residual in one launch
//   dec_moe_plan / dec_moe_gather / dec_moe_combine   prefill: token rows grouped by expert into 128-row
//                      aligned segments for the MFMA GEMM, and the weighted sum back
// Expert weights are stacked along rows: up|gate [E * 2F, d] (each expert's rows packed by pack_upgate on
// their own), down [E * d, F]; bf16, Q4G32 or Q8G32 (decoder_gemv.hpp).  An id is read from device memory
// by the kernel that uses it, so a captured decode step's arguments never change.  An id outside [0, E) --
// nothing here produces one -- is clamped, so that no kernel leaves the stacked matrix.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>

#include "decoder_common.hpp"
#include "decoder_gemv.hpp"

namespace {

constexpr int kMoeMaxE = 256;  // router width: 4 logits per lane
constexpr int kMoeMaxK = 8;    // experts used per token

__device__ __forceinline__ int expert_at(const int32_t* ids, int j, int E) {
  const int e = ids[j];
  return e < 0 ? 0 : (e >= E ? E - 1 : e);
}

// ------------------------------------------------------------------ router --
// One wave per row of logits [T, ldl] (columns >= E are never read), lane l holds columns l, l + 64, ..
// k rounds of wave argmax over (logit descending, index ascending): softmax is monotone, so this is the
// order of the probabilities without their rounding.  The weights are the probabilities renormalised over
// the chosen k: the softmax denominator cancels, w_j = exp(l_j - max) / sum_chosen exp(l_i - max), fp32.
__global__ __launch_bounds__(256) void k_moe_route(const float* __restrict__ logits, long ldl, int T, int E, int k,
                                                   int32_t* __restrict__ ids, float* __restrict__ w) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* l = logits + (long)row * ldl;
  constexpr int PER = kMoeMaxE / 64;
  float v[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = lane + 64 * i;
    const float t = c < E ? l[c] : -INFINITY;
    v[i] = t == t ? t : -INFINITY;  // a NaN logit ranks last
  }
  unsigned taken = 0;
  float top = 0.f, sum = 0.f, mine = 0.f;
  int mine_id = 0;
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = lane + 64 * i;
      if (c < E && !(taken >> i & 1) && (bi == 0x7fffffff || v[i] > bv)) { bv = v[i]; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
    if (j == 0) top = bv;
    const float e = top == -INFINITY ? 1.f : expf(bv - top);
    sum += e;
    if (lane == j) { mine = e; mine_id = bi; }
  }
  if (lane < k) {
    ids[(long)row * k + lane] = mine_id;
    w[(long)row * k + lane] = mine / sum;
  }
}

// ------------------------------------------------------------------ decode: up|gate --
// k_gemv<2, RMS> / k_gemv_q4<2, RMS, BITS> on expert ids[blockIdx.y]'s row block of the stacked matrix,
// into row blockIdx.y of out [k, nout]: the same loop text, so the same bits as dec_gemv* on that slice.
template <bool RMS>
__global__ __launch_bounds__(256) void k_gemv_moe(const uint16_t* __restrict__ x, const float* __restrict__ rw,
                                                  float eps, const uint16_t* __restrict__ Wall, int K, int nout,
                                                  const int32_t* __restrict__ ids, int E, uint16_t* outall) {
  constexpr int MODE = 2;
  const uint16_t* __restrict__ W = Wall + (long)expert_at(ids, blockIdx.y, E) * (2 * nout) * K;
  const uint16_t* res = nullptr;
  void* out = outall + (long)blockIdx.y * nout;
#include "decoder_body_gemv.hpp"
}

template <bool RMS, int BITS>
__global__ __launch_bounds__(256) void k_gemv_moe_q4(const uint16_t* __restrict__ x, const float* __restrict__ rw,
                                                     float eps, const uint8_t* __restrict__ Wqall,
                                                     const uint32_t* __restrict__ Wsmall, int K, int nout,
                                                     const int32_t* __restrict__ ids, int E, uint16_t* outall) {
  constexpr int MODE = 2;
  const long row0 = (long)expert_at(ids, blockIdx.y, E) * (2 * nout);
  const uint8_t* __restrict__ Wq = Wqall + row0 * ((long)K * BITS / 8);
  const uint32_t* __restrict__ Wsm = Wsmall + row0 * (K / kQ4Group);
  const uint16_t* res = nullptr;
  void* out = outall + (long)blockIdx.y * nout;
#include "decoder_body_gemv_q4.hpp"
}

// ------------------------------------------------------------------ decode: down --
// out[o] = bf16(res[o] + sum_j w[j] * dot(W[ids[j] * d + o, :], f[j, :])), j ascending, fp32, one rounding.
// A wave owns kGemvRows outputs for all k experts.  The k rows of f are one vector of k * F values against
// the wave's k row pieces: the workgroup stages as many whole rows of f as fit kGemvMaxK values in LDS (all
// 8 of a 768-wide expert, one of a 14336-wide), and a lane walks that batch in units of 16 B of weights
// (bf16) or one 32-k group (4- / 8-bit), 64 units apart, with the next unit's weights requested ahead of
// the math as in k_gemv.  A unit's dot product enters the lane's running total through w[j]; one wave
// reduction at the end.  BITS 16: bf16 weights; 4 / 8: Q4G32 / Q8G32 planes.
// LDS: bf16, 40 elements per 32 values (64 B + 16 B pad): a lane's four 16-B reads of one group start on
// distinct 4-bank quads across a 16-lane phase (stride 20 dwords), as the 36-float record of k_gemv_q4.
constexpr int kDownRec = kQ4Group + 8;

template <int BITS>
__global__ __launch_bounds__(256) void k_moe_down(const uint16_t* __restrict__ f, const void* __restrict__ Wv,
                                                  const uint32_t* __restrict__ Wsm, int d, int F,
                                                  const int32_t* __restrict__ ids, const float* __restrict__ w, int k,
                                                  int E, const uint16_t* res, uint16_t* out) {
  __shared__ __attribute__((aligned(16))) uint16_t xs[kGemvMaxK / kQ4Group * kDownRec];
  __shared__ int sid[kMoeMaxK];
  __shared__ float sw[kMoeMaxK];
  constexpr int R = kGemvRows;
  constexpr int GV = BITS == 16 ? 1 : BITS / 4;  // 16-B loads per unit and row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch = F >> 3, ng = F / kQ4Group;
  const int per = BITS == 16 ? nch : ng;  // units per expert
  const long rowbytes = (long)F * BITS / 8;
  const uint8_t* Wb = (const uint8_t*)Wv;
  const int o0 = (blockIdx.x * 4 + wave) * R;
  const bool active = o0 < d;
  long rows[R];
#pragma unroll
  for (int r = 0; r < R; ++r) rows[r] = o0 + r < d ? o0 + r : d - 1;
  if (tid < k) {  // read by the waves after the first barrier below
    sid[tid] = expert_at(ids, tid, E);
    sw[tid] = w[tid];
  }
  const int JB = F >= kGemvMaxK ? 1 : kGemvMaxK / F;  // rows of f per LDS batch
  float tot[R] = {};
  for (int j0 = 0; j0 < k; j0 += JB) {
    const int nb = k - j0 < JB ? k - j0 : JB;
    if (j0) __syncthreads();  // every wave is done with the batch before
    for (int c = tid; c < nb * nch; c += 256)
      *(uint4*)(xs + (c >> 2) * kDownRec + (c & 3) * 8) = *(const uint4*)(f + (long)j0 * F + c * 8);
    __syncthreads();
    if (!active) continue;
    const int total = nb * per;
    // unit c of the batch is unit u of expert j0 + jj
    int jj = 0, u = lane;
    while (u >= per) { u -= per; ++jj; }
    uint4 wq[R][GV];
    uint32_t sm[R] = {};
    auto fetch = [&](int jn, int un) {
      const long e0 = (long)sid[j0 + jn] * d;
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int v = 0; v < GV; ++v) wq[r][v] = *(const uint4*)(Wb + (e0 + rows[r]) * rowbytes + un * 16 * GV + v * 16);
        if constexpr (BITS != 16) sm[r] = Wsm[(e0 + rows[r]) * ng + un];
      }
    };
    if (lane < total) fetch(jj, u);
    for (int c = lane; c < total; c += 64) {
      uint4 cq[R][GV];
      uint32_t csm[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int v = 0; v < GV; ++v) cq[r][v] = wq[r][v];
        csm[r] = sm[r];
      }
      const float wj = sw[j0 + jj];
      u += 64;
      while (u >= per) { u -= per; ++jj; }
      if (c + 64 < total) fetch(jj, u);  // one unit of look-ahead per row
      float dotp[R];
      if constexpr (BITS == 16) {
        float xf[8];
        unpack8(*(const uint4*)(xs + (c >> 2) * kDownRec + (c & 3) * 8), xf);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float wf[8];
          unpack8(cq[r][0], wf);
          dotp[r] = 0.f;
#pragma unroll
          for (int q = 0; q < 8; ++q) dotp[r] += wf[q] * xf[q];
        }
      } else {
        float xg[kQ4Group];
        float gs = 0.f;
#pragma unroll
        for (int q = 0; q < kQ4Group; q += 8) {
          unpack8(*(const uint4*)(xs + c * kDownRec + q), xg + q);
#pragma unroll
          for (int t = 0; t < 8; ++t) gs += xg[q + t];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float dot;
          if constexpr (BITS == 4) {
            dot = q4dot8(cq[r][0].x, xg);
            dot += q4dot8(cq[r][0].y, xg + 8);
            dot += q4dot8(cq[r][0].z, xg + 16);
            dot += q4dot8(cq[r][0].w, xg + 24);
          } else {
            dot = q8dot4(cq[r][0].x, xg);
            dot += q8dot4(cq[r][0].y, xg + 4);
            dot += q8dot4(cq[r][0].z, xg + 8);
            dot += q8dot4(cq[r][0].w, xg + 12);
            dot += q8dot4(cq[r][GV - 1].x, xg + 16);
            dot += q8dot4(cq[r][GV - 1].y, xg + 20);
            dot += q8dot4(cq[r][GV - 1].z, xg + 24);
            dot += q8dot4(cq[r][GV - 1].w, xg + 28);
          }
          dotp[r] = fmaf(bf2f(csm[r] & 0xffff), dot, bf2f(csm[r] >> 16) * gs);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) tot[r] = fmaf(wj, dotp[r], tot[r]);
    }
  }
  if (!active) return;
#pragma unroll
  for (int r = 0; r < R; ++r) tot[r] = wave_sum(tot[r]);
  if (lane < R && o0 + lane < d) {
    float y = tot[0];
#pragma unroll
    for (int r = 1; r < R; ++r)
      if (r == lane) y = tot[r];
    y += bf2f(res[o0 + lane]);
    out[o0 + lane] = __builtin_bit_cast(uint16_t, (__bf16)y);
  }
}

// ------------------------------------------------------------------ prefill grouping --
// One workgroup, thread e owns expert e: it counts its entries of ids [n] (n = T * k, (t, j) order), the
// starts are the running sum of the counts rounded up to `align`, and a second walk hands out the slots
// in entry order.  No atomics: counts, starts and ranks are the same on every run.
__global__ __launch_bounds__(kMoeMaxE) void k_moe_plan(const int32_t* __restrict__ ids, int n, int E, int align,
                                                       int32_t* __restrict__ counts, int32_t* __restrict__ base,
                                                       int32_t* __restrict__ slot) {
  __shared__ int cnt[kMoeMaxE], start[kMoeMaxE];
  const int e = threadIdx.x;
  int c = 0;
  for (int i = 0; i < n; ++i) c += ids[i] == e;
  cnt[e] = c;
  __syncthreads();
  if (e == 0) {
    int run = 0;
    for (int i = 0; i < E; ++i) {
      start[i] = run;
      run += (cnt[i] + align - 1) / align * align;
    }
  }
  __syncthreads();
  if (e >= E) return;
  counts[e] = c;
  base[e] = start[e];
  int r = start[e];
  for (int i = 0; i < n; ++i)
    if (ids[i] == e) slot[i] = r++;
}

// xg[slot[i]] = x[i / k] for the n = T * k entries, in 16-byte pieces; a slot outside [0, rows) is skipped
__global__ __launch_bounds__(256) void k_moe_gather(const uint16_t* __restrict__ x, long ldx, int k, int d,
                                                    const int32_t* __restrict__ slot, int rows,
                                                    uint16_t* __restrict__ xg) {
  const int i = blockIdx.x, s = slot[i];
  if (s < 0 || s >= rows) return;
  const uint16_t* src = x + (long)(i / k) * ldx;
  uint16_t* dst = xg + (long)s * d;
  for (int c = threadIdx.x; c < d / 8; c += 256) *(uint4*)(dst + c * 8) = *(const uint4*)(src + c * 8);
}

// out[t] = bf16(res[t] + sum_j w[t, j] * y[slot[t, j]]), j ascending, fp32, one rounding; 4 columns a thread
__global__ __launch_bounds__(256) void k_moe_combine(const float* __restrict__ y, int rows, int k, int d,
                                                     const int32_t* __restrict__ slot, const float* __restrict__ w,
                                                     const uint16_t* res, long ldres, uint16_t* out, long ldo) {
  const int t = blockIdx.x;
  for (int c = threadIdx.x * 4; c < d; c += 1024) {
    float a[4] = {};
    for (int j = 0; j < k; ++j) {
      const int s = slot[t * k + j];
      if (s < 0 || s >= rows) continue;
      const float wj = w[t * k + j];
      const float4 v = *(const float4*)(y + (long)s * d + c);
      a[0] = fmaf(wj, v.x, a[0]);
      a[1] = fmaf(wj, v.y, a[1]);
      a[2] = fmaf(wj, v.z, a[2]);
      a[3] = fmaf(wj, v.w, a[3]);
    }
    const uint2 r = *(const uint2*)(res + (long)t * ldres + c);
    const uint16_t rr[4] = {(uint16_t)(r.x & 0xffff), (uint16_t)(r.x >> 16), (uint16_t)(r.y & 0xffff),
                            (uint16_t)(r.y >> 16)};
    uint16_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = __builtin_bit_cast(uint16_t, (__bf16)(bf2f(rr[q]) + a[q]));
    *(uint2*)(out + (long)t * ldo + c) = make_uint2(o[0] | (uint32_t)o[1] << 16, o[2] | (uint32_t)o[3] << 16);
  }
}

// ------------------------------------------------------------------ host --
bool moe_shape_ok(int E, int k) { return E >= 1 && E <= kMoeMaxE && k >= 1 && k <= kMoeMaxK && k <= E; }

template <int BITS>
int moe_upgate_qn(const void* x, const float* rms_w, float eps, const void* Wq, const void* Wsm, int N, int K,
                  const int32_t* ids, int k, int E, void* out, hipStream_t s) {
  if (K <= 0 || K % kQ4Group || K > kGemvQ4MaxK || N <= 0 || N % 32 || !moe_shape_ok(E, k) || !ids || !out ||
      ((uintptr_t)Wq | (uintptr_t)x) % 16 || (uintptr_t)Wsm % 4 || (rms_w && (uintptr_t)rms_w % 16) ||
      ((long)N * K * BITS / 8) % 16)
    return (int)hipErrorInvalidValue;
  const int nout = N / 2, per_block = 4 * (kGemvRows / 2);
  const dim3 g((unsigned)((nout + per_block - 1) / per_block), (unsigned)k), b(256);
  const size_t lds = (size_t)(K / kQ4Group) * kQ4Rec * sizeof(float);
  if (rms_w)
    hipLaunchKernelGGL((k_gemv_moe_q4<true, BITS>), g, b, lds, s, (const uint16_t*)x, rms_w, eps, (const uint8_t*)Wq,
                       (const uint32_t*)Wsm, K, nout, ids, E, (uint16_t*)out);
  else
    hipLaunchKernelGGL((k_gemv_moe_q4<false, BITS>), g, b, lds, s, (const uint16_t*)x, rms_w, eps, (const uint8_t*)Wq,
                       (const uint32_t*)Wsm, K, nout, ids, E, (uint16_t*)out);
  return (int)hipGetLastError();
}

template <int BITS>
int moe_down(const void* f, const void* W, const void* Wsm, int d, int F, const int32_t* ids, const float* w, int k,
             int E, const void* res, void* out, hipStream_t s) {
  const int mult = BITS == 16 ? 8 : kQ4Group;
  if (d <= 0 || F <= 0 || F % mult || F > kGemvMaxK || !moe_shape_ok(E, k) || !ids || !w || !res || !out ||
      ((uintptr_t)W | (uintptr_t)f) % 16 || (BITS != 16 && (!Wsm || (uintptr_t)Wsm % 4)) ||
      ((long)d * F * (BITS == 16 ? 16 : BITS) / 8) % 16)
    return (int)hipErrorInvalidValue;
  const dim3 g((unsigned)((d + 4 * kGemvRows - 1) / (4 * kGemvRows))), b(256);
  hipLaunchKernelGGL((k_moe_down<BITS>), g, b, 0, s, (const uint16_t*)f, W, (const uint32_t*)Wsm, d, F, ids, w, k, E,
                     (const uint16_t*)res, (uint16_t*)out);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// logits fp32 [T, ldl] -> ids int32 [T, k] (chosen experts, best first; ties to the lowest index) and
// w fp32 [T, k] (their softmax probabilities renormalised to sum 1).  E <= 256, k <= 8, k <= E.
int dec_moe_route(const float* logits, long ldl, int T, int E, int k, int32_t* ids, float* w, hipStream_t s) {
  if (!logits || !ids || !w || T <= 0 || !moe_shape_ok(E, k) || ldl < E) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_moe_route, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, logits, ldl, T, E, k, ids, w);
  return (int)hipGetLastError();
}

// dec_gemv mode 2 (RMSNorm with rms_w when non-null, up|gate, SwiGLU) on each of the k experts ids names:
// W bf16 [E * N, K] stacked, N = 2F packed rows per expert, out bf16 [k, F].  Limits of dec_gemv.
int dec_gemv_moe(const void* x, const float* rms_w, float eps, const void* W, int N, int K, const int32_t* ids, int k,
                 int E, void* out, hipStream_t s) {
  if (K <= 0 || K % 8 || K > kGemvMaxK || N <= 0 || N % 32 || !moe_shape_ok(E, k) || !ids || !out ||
      ((uintptr_t)W | (uintptr_t)x) % 16)
    return (int)hipErrorInvalidValue;
  const int nout = N / 2, per_block = 4 * (kGemvRows / 2);
  const dim3 g((unsigned)((nout + per_block - 1) / per_block), (unsigned)k), b(256);
  if (rms_w)
    hipLaunchKernelGGL((k_gemv_moe<true>), g, b, 0, s, (const uint16_t*)x, rms_w, eps, (const uint16_t*)W, K, nout,
                       ids, E, (uint16_t*)out);
  else
    hipLaunchKernelGGL((k_gemv_moe<false>), g, b, 0, s, (const uint16_t*)x, rms_w, eps, (const uint16_t*)W, K, nout,
                       ids, E, (uint16_t*)out);
  return (int)hipGetLastError();
}

// the same over Q4G32 / Q8G32 planes Wq [E * N, K * bits / 8], Wsm [E * N, K / 32].  Limits of dec_gemv_q4.
int dec_gemv_moe_q4(const void* x, const float* rms_w, float eps, const void* Wq, const void* Wsm, int N, int K,
                    const int32_t* ids, int k, int E, void* out, hipStream_t s) {
  return moe_upgate_qn<4>(x, rms_w, eps, Wq, Wsm, N, K, ids, k, E, out, s);
}
int dec_gemv_moe_q8(const void* x, const float* rms_w, float eps, const void* Wq, const void* Wsm, int N, int K,
                    const int32_t* ids, int k, int E, void* out, hipStream_t s) {
  return moe_upgate_qn<8>(x, rms_w, eps, Wq, Wsm, N, K, ids, k, E, out, s);
}

// f bf16 [k, F], W [E * d, F] stacked (bf16, or Q4G32 / Q8G32 planes), ids / w [k], res / out bf16 [d]
// (may alias).  F % 8 (bf16) or % 32, F <= 16384.
int dec_gemv_moe_down(const void* f, const void* W, int d, int F, const int32_t* ids, const float* w, int k, int E,
                      const void* res, void* out, hipStream_t s) {
  return moe_down<16>(f, W, nullptr, d, F, ids, w, k, E, res, out, s);
}
int dec_gemv_moe_down_q4(const void* f, const void* Wq, const void* Wsm, int d, int F, const int32_t* ids,
                         const float* w, int k, int E, const void* res, void* out, hipStream_t s) {
  return moe_down<4>(f, Wq, Wsm, d, F, ids, w, k, E, res, out, s);
}
int dec_gemv_moe_down_q8(const void* f, const void* Wq, const void* Wsm, int d, int F, const int32_t* ids,
                         const float* w, int k, int E, const void* res, void* out, hipStream_t s) {
  return moe_down<8>(f, Wq, Wsm, d, F, ids, w, k, E, res, out, s);
}

// ids int32 [T, k] -> counts [E] (entries per expert), base [E] (each expert's first slot: the running sum
// of the counts, every start rounded up to `align`), slot [T, k] (base[e] + the entry's rank among e's
// entries in (t, j) order).  An entry whose id is outside [0, E) keeps what slot held (the caller's -1).
int dec_moe_plan(const int32_t* ids, int T, int k, int E, int align, int32_t* counts, int32_t* base, int32_t* slot,
                 hipStream_t s) {
  if (!ids || !counts || !base || !slot || T <= 0 || !moe_shape_ok(E, k) || align < 1 ||
      (long)T * k + (long)E * align > 0x7fffffffL)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_moe_plan, dim3(1), dim3(kMoeMaxE), 0, s, ids, T * k, E, align, counts, base, slot);
  return (int)hipGetLastError();
}

// xg bf16 [rows, d]: row slot[t, j] = x[t] (x bf16 [T, ldx]); rows no slot names are not written
int dec_moe_gather(const void* x, long ldx, int T, int k, int d, const int32_t* slot, int rows, void* xg,
                   hipStream_t s) {
  if (!x || !slot || !xg || T <= 0 || k < 1 || k > kMoeMaxK || d <= 0 || d % 8 || ldx < d || ldx % 8 || rows <= 0 ||
      ((uintptr_t)x | (uintptr_t)xg) % 16)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_moe_gather, dim3((unsigned)(T * k)), dim3(256), 0, s, (const uint16_t*)x, ldx, k, d, slot, rows,
                     (uint16_t*)xg);
  return (int)hipGetLastError();
}

// out[t] = bf16(res[t] + sum_j w[t, j] y[slot[t, j]]): y fp32 [rows, d], res / out bf16 rows (may alias)
int dec_moe_combine(const float* y, int rows, int T, int k, int d, const int32_t* slot, const float* w,
                    const void* res, long ldres, void* out, long ldo, hipStream_t s) {
  if (!y || !slot || !w || !res || !out || T <= 0 || k < 1 || k > kMoeMaxK || d <= 0 || d % 4 || rows <= 0 ||
      ldres < d || ldo < d || ldres % 4 || ldo % 4 || (uintptr_t)y % 16 || ((uintptr_t)res | (uintptr_t)out) % 8)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_moe_combine, dim3((unsigned)T), dim3(256), 0, s, y, rows, k, d, slot, w, (const uint16_t*)res,
                     ldres, (uint16_t*)out, ldo);
  return (int)hipGetLastError();
}

}  // extern "C"
