// gemm_rln.hip — residual projection + post-LayerNorm in one kernel (K15 / K16-down of SURVEY
// §2.10): the o-proj and FFN-down GEMMs of the Nomic-BERT encoder, whose output width is the model
// width (N = 768), so ONE workgroup owns whole output rows and finishes the LayerNorm in registers:
//
//   out[m, :] = LN( A[m, :] . W^T + res[m, :] ) * gamma + beta        (out may alias res)
//
// This replaces the reference daemon's llama.cpp decode of these layers
// (/root/reference/splinference.cpp:236-251) and the round-2 pairing of a library GEMM with a
// separate LayerNorm pass (one extra read + write of the [M, 768] activations per projection).
//
// Geometry (gfx950, 256 CUs): workgroup tile 128 rows x 768 columns, 512 threads = 8 waves as
// 2 (rows) x 4 (columns); each wave owns 64 rows x 192 columns = 4 x 12 tiles of
// v_mfma_f32_16x16x32_bf16 (192 fp32 accumulators per lane).  At M = 32768 tokens the grid is
// exactly 256 workgroups: one per CU, no tail wave.  The MFMA operands are swapped (the W fragment
// is the A operand), so a lane's accumulator holds four CONSECUTIVE output columns of one row:
// residual loads, LayerNorm and the bf16 stores work on 8-byte row pieces straight from registers
// (16-byte pieces in the default form, after lanes l and l ^ 16 exchange halves: EPI 4 below).
//
// K loop: BK = 32 (one MFMA k-step), LDS rings of three W stages (768 x 32 bf16, 48 KB each) and
// two A stages (128 x 32, 8 KB each), filled by global_load_lds_dwordx4 (LDS-DMA; 7
// wave-instructions per wave per stage) two and one stages ahead of the MFMAs and issued between
// them, counted vmcnt + raw s_barrier (no vmcnt(0) drain in the loop): the ring loop shared with
// k_gemm384's 32-wide arm, one text in gemm_ring32_issue.hpp + gemm_ring32_body.hpp.  The
// LDS image has 64-byte rows; the 16-byte chunk c of row r is stored at chunk c ^ ((r >> 1) & 3),
// which makes every ds_read_b128 lane group (16 lanes) hit 16 distinct bank slots (brute-forced
// over the gfx950 b128 lane groups); glds writes lane-linearly, so the XOR is applied to the
// global source address and to the read address (guide rule 21).
//
// Epilogue: v = acc + res (fp32), row sums over the wave's 48 values per row, then across the 4
// lanes that share the row (xor 16 / 32) and the 4 column waves (LDS), two passes (mean, then
// centred variance), then (v - mean) * rstd * gamma + beta -> bf16.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>

#include "bf16_util.hpp"
#include "gemm_tile.hpp"
#include "nomic_api.h"

namespace {

constexpr int kBM = 128;          // rows per workgroup
constexpr int kN = 768;           // output width (= model width)
constexpr int kBK = 32;           // K per stage
constexpr int kWN = kN / 4;       // columns per wave (192)
constexpr int kNT = kWN / 16;     // 16-wide n-tiles per wave (12)
constexpr int kThreads = 512;
constexpr int kRowBytes = kBK * 2;                   // 64
constexpr int kABytes = kBM * kRowBytes;             // 8 KB per A stage
constexpr int kWBytes = kN * kRowBytes;              // 48 KB per W stage
constexpr int kEpiLds = 4 * kBM * 4;                 // epilogue: [4 column waves][128 rows] fp32 row sums

// K pipeline: LDS rings of kNW W stages and kNA A stages, one barrier per stage; the loop and its
// explanation are in gemm_ring32_body.hpp.
constexpr int kNW = 3, kNA = 2;
constexpr int kLdsBytes = kNW * kWBytes + kNA * kABytes;  // 160 KB: [W ring | A ring]
static_assert(kLdsBytes <= 160 * 1024 && kLdsBytes >= kEpiLds, "LDS budget");

__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {  // wave-uniform: a scalar branch to an immediate count
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// EPI 0: residual added in the epilogue (8-B loads).  3 (K = 768, the o-proj): the residual is
// added during the K loop -- stage t loads the lane's residual pieces of two of its 48 (m-tile,
// n-tile) accumulator tiles, stage t + 1 adds them -- so the epilogue only normalises and stores:
// the residual's 50 MB at M = 32768 no longer arrive while every workgroup sits in its epilogue
// (o-proj 62.6 -> 56.3 us; the down projection, K = 3072, gains nothing from it: 146.3 vs 147.1 us,
// profiles/r4aq).  4: EPI 0 with 16-B residual loads and output stores from registers (24 of each
// per lane instead of 48 8-B ones; lane pairs l, l ^ 16 exchange halves, see the epilogue): o-proj
// 64.0 -> 51.4 us, down 149.8 -> 138.0 us, the same bits (profiles/encoder_tails).  It needs 16-B
// aligned residual and output rows; the entry point runs EPI 0 where they are not.
//
// Measured and removed (each was a template parameter of this kernel; o-proj / down at M = 32768;
// variant numbers are round 3's -- 2, ring, DMAs per MFMA pair -- not today's NOMIC_RLN values):
//   - all of a stage's DMAs issued right after the barrier (ILV 0, variant 220): 67.6 / 152.0 us
//     against 59.1 / 144.7 with two DMAs ahead of each MFMA pair (222); three per pair (ILV 3, on
//     the PIPE 1 and 4 rings: 213, 243): 66.2 / 156.4 and 66.7 / 157.2 (profiles/r3_rln_ab.jsonl)
//   - rings of 2 W + 4 A stages and 2 W + 6 A stages (PIPE 1, 4: variants 212, 242 of that file):
//     59.7 / 146.4 and 60.2 / 147.7 against 59.1 / 144.7; 2 W + 2 A (PIPE 3): the first form,
//     from before the A/B files
//   - the residual as the first K step, an MFMA against an identity operand (EPI 2), and W
//     fragments read two pairs ahead (PF 2): within +-1 % or slower (profiles/r3_pmc_encoder.md,
//     r3_rln_variants_ab.jsonl)
//   - the K loop's DMAs from inline asm (AS): o-proj 61.4 against 62.6, down 150.1 against 147.1,
//     embed step 9.28-9.34 against 9.20 ms (profiles/r3_gemm_asm_dma.md)
//   - block b starting its K walk at step b mod nk (ROT): equal at K 128 / 768, +7 % at K 3072
//     (profiles/r3_rln_rot_ab.jsonl)
//   - 4 waves of 128 rows x 192 columns (WM 1): built for the A/B harness, no measurement kept
//   - 16-B stores on EPI 3: o-proj 57.9 us, no better than EPI 3 itself; an LDS-staged 16-B
//     epilogue: 109 registers spilled into the K loop, 420 us on the down shape
//     (profiles/encoder_tails/rln_ab.jsonl)
template <int EPI>
__global__ __launch_bounds__(kThreads, 1) void k_gemm_rln(const uint16_t* __restrict__ A, long lda,
                                                          const uint16_t* __restrict__ W, long ldw, int K, long M,
                                                          const uint16_t* res, long ldr,
                                                          const uint16_t* __restrict__ gamma,
                                                          const uint16_t* __restrict__ beta, float eps,
                                                          uint16_t* out, long ldo) {
  constexpr int LW = kNW - 1, LA = kNA - 1;            // stages of lead
  constexpr int kABase = kNW * kWBytes;                // LDS: [W ring | A ring]
  constexpr int kWaves = kThreads / 64;                // 8 waves: 2 (rows) x 4 (columns)
  constexpr int RW = kBM / 2, MT = RW / 16;            // rows and m-tiles per wave
  constexpr int GA = 8 / kWaves, GW = 48 / kWaves;     // LDS-DMA wave-instructions per wave per stage
  constexpr bool KRES = EPI == 3;  // residual added during the K loop
  constexpr bool WIDE = EPI == 4;  // 16-B epilogue I/O from registers
  static_assert(EPI == 0 || EPI == 3 || EPI == 4, "epilogue forms");
  static_assert(!KRES || MT * kNT == 48, "EPI 3 spreads 48 accumulator tiles over 24 stages");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wn = wave & 3;
  // W is read by every block and A rows by one block only: no reuse for an XCD remap to exploit
  const long m0 = (long)blockIdx.x * kBM;

  // ---- per-lane LDS-DMA sources: a wave-instruction covers 16 rows x 64 B, lane -> (row, chunk)
  const int drow = lane >> 2, dpc = lane & 3;
  uint32_t offA[GA];
#pragma unroll
  for (int i = 0; i < GA; ++i) {
    const int r = (wave + kWaves * i) * 16 + drow;
    const long gr = (m0 + r < M) ? m0 + r : M - 1;       // tail rows re-read row M-1, never stored
    offA[i] = (uint32_t)(gr * lda + swz(r, dpc) * 8);
  }
  uint32_t offW[GW];
#pragma unroll
  for (int i = 0; i < GW; ++i) {
    const int r = (wave + kWaves * i) * 16 + drow;
    offW[i] = (uint32_t)(r * ldw + swz(r, dpc) * 8);
  }
#include "gemm_ring32_issue.hpp"
  // the accumulators and the EPI 3 state are declared here, between the two halves of the ring text:
  // declared ahead of the DMA lambdas they change the register allocation of all three forms
  f32x4 acc[MT][kNT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < kNT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // EPI 3: residual pieces of accumulator tile u = (u / kNT, u % kNT), two tiles per stage
  const long rmb = m0 + wr * RW + (lane & 15);
  const int rcq = (lane >> 4) * 4;
  uint2 rq[2] = {make_uint2(0, 0), make_uint2(0, 0)};
  auto res_load = [&](int u, uint2& d) {
    const int i = u / kNT, j = u % kNT;
    const long m = rmb + 16 * i < M ? rmb + 16 * i : M - 1;
    d = *(const uint2*)(res + m * ldr + wn * kWN + j * 16 + rcq);
  };
  auto res_add = [&](int u, const uint2& rr) {
    const int i = u / kNT, j = u % kNT;
    acc[i][j][0] += bf2f(rr.x & 0xffff);
    acc[i][j][1] += bf2f(rr.x >> 16);
    acc[i][j][2] += bf2f(rr.y & 0xffff);
    acc[i][j][3] += bf2f(rr.y >> 16);
  };
  // stage t, between its barrier and its MFMAs: the pieces are loaded one stage ahead of their add,
  // issued before this stage's DMAs (older than them: the counted waits stay exact); a chain of
  // uniform branches keeps the tile indices static.  Text, not a lambda: as a lambda it changes the
  // register allocation of all three forms.
#define GEMM_RING32_STAGE_HOOK(t)                      \
  if (KRES && t < 24) {                                \
    _Pragma("unroll") for (int k = 0; k < 24; ++k) {   \
      if (t == k) {                                    \
        if (k > 0) {                                   \
          res_add(2 * (k - 1), rq[0]);                 \
          res_add(2 * (k - 1) + 1, rq[1]);             \
        }                                              \
        res_load(2 * k, rq[0]);                        \
        res_load(2 * k + 1, rq[1]);                    \
      }                                                \
    }                                                  \
  }
#include "gemm_ring32_body.hpp"
#undef GEMM_RING32_STAGE_HOOK
  if constexpr (KRES) {  // the last pair (loaded at stage 23)
    res_add(46, rq[0]);
    res_add(47, rq[1]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  raw_barrier();  // every wave is done with the rings: the LDS is the epilogue's

  // ---- epilogue -------------------------------------------------------------------------
  // lane: rows m_i = m0 + wr*64 + i*16 + (lane & 15); columns n_j = wn*192 + j*16 + (lane>>4)*4 + 0..3
  const int rl = lane & 15, cq = (lane >> 4) * 4;
  {
    // residual loads (EPI 0 / 4; EPI 3 has it in the accumulators) and stores from registers, in
    // 8-B (EPI 0, 3) or 16-B (EPI 4) row pieces
    float* red = (float*)smem;  // [4 column waves][128 rows]
    const long mb = m0 + wr * RW + rl;  // row of m-tile i: mb + 16 i
    float s[MT] = {};
    // WIDE: lanes l and l ^ 16 hold adjacent 4-column groups of one row.  For the n-tile pair
    // (2p, 2p + 1) the even 16-lane group takes the pair's 8 consecutive columns of tile 2p and the
    // odd group those of tile 2p + 1: one 16-B access per lane and pair, and the half that belongs
    // to the partner lane changes hands by ds_swizzle (lane ^ 16, no LDS memory).  Every value is
    // added and summed in the order of the 8-B form (per row: n-tiles ascending), so the bits match.
    const bool odd = (lane >> 4) & 1;
    const int c8 = wn * kWN + (odd ? 16 : 0) + (lane >> 5) * 8;  // + 32 p: the lane's 8 columns of pair p
    (void)odd, (void)c8;
    if constexpr (EPI == 4) {
#pragma unroll
      for (int p = 0; p < kNT / 2; ++p) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const long m = mb + 16 * i < M ? mb + 16 * i : M - 1;
          const uint4 rr = *(const uint4*)(res + m * ldr + c8 + 32 * p);
          const uint32_t lo[2] = {rr.x, rr.y}, hi[2] = {rr.z, rr.w};
          const uint4 rv = exchange16(odd, lo, hi);
          const uint32_t r0[2] = {rv.x, rv.y};  // tile 2p
          const uint32_t r1[2] = {rv.z, rv.w};  // tile 2p + 1
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int j = 2 * p + h;
            const uint32_t x = h ? r1[0] : r0[0], y = h ? r1[1] : r0[1];
            acc[i][j][0] += bf2f(x & 0xffff);
            acc[i][j][1] += bf2f(x >> 16);
            acc[i][j][2] += bf2f(y & 0xffff);
            acc[i][j][3] += bf2f(y >> 16);
            s[i] += (acc[i][j][0] + acc[i][j][1]) + (acc[i][j][2] + acc[i][j][3]);
          }
        }
      }
    } else {
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      const int n = wn * kWN + j * 16 + cq;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if constexpr (EPI == 0) {
          const long m = mb + 16 * i < M ? mb + 16 * i : M - 1;
          const uint2 rr = *(const uint2*)(res + m * ldr + n);
          acc[i][j][0] += bf2f(rr.x & 0xffff);
          acc[i][j][1] += bf2f(rr.x >> 16);
          acc[i][j][2] += bf2f(rr.y & 0xffff);
          acc[i][j][3] += bf2f(rr.y >> 16);
        }
        (void)n;
        s[i] += (acc[i][j][0] + acc[i][j][1]) + (acc[i][j][2] + acc[i][j][3]);
      }
    }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      s[i] += __shfl_xor(s[i], 16);
      s[i] += __shfl_xor(s[i], 32);
    }
    if (lane < 16) {
#pragma unroll
      for (int i = 0; i < MT; ++i) red[wn * kBM + wr * RW + i * 16 + rl] = s[i];
    }
    __syncthreads();
    float mean[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int r = wr * RW + i * 16 + rl;
      mean[i] = (red[r] + red[kBM + r] + red[2 * kBM + r] + red[3 * kBM + r]) * (1.f / kN);
      s[i] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < kNT; ++j)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = acc[i][j][e] - mean[i];
          s[i] += d * d;
        }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      s[i] += __shfl_xor(s[i], 16);
      s[i] += __shfl_xor(s[i], 32);
    }
    __syncthreads();  // every wave has read the row sums
    if (lane < 16) {
#pragma unroll
      for (int i = 0; i < MT; ++i) red[wn * kBM + wr * RW + i * 16 + rl] = s[i];
    }
    __syncthreads();
    float rstd[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int r = wr * RW + i * 16 + rl;
      const float var = (red[r] + red[kBM + r] + red[2 * kBM + r] + red[3 * kBM + r]) * (1.f / kN);
      rstd[i] = rsqrtf(var + eps);
    }
    if constexpr (WIDE) {
#pragma unroll
      for (int p = 0; p < kNT / 2; ++p) {
        float g[2][4], be[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int n = wn * kWN + (2 * p + h) * 16 + cq;
          const uint2 gg = *(const uint2*)(gamma + n), bb = *(const uint2*)(beta + n);
          g[h][0] = bf2f(gg.x & 0xffff), g[h][1] = bf2f(gg.x >> 16), g[h][2] = bf2f(gg.y & 0xffff), g[h][3] = bf2f(gg.y >> 16);
          be[h][0] = bf2f(bb.x & 0xffff), be[h][1] = bf2f(bb.x >> 16), be[h][2] = bf2f(bb.y & 0xffff), be[h][3] = bf2f(bb.y >> 16);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const long m = mb + 16 * i;
          uint32_t pk[2][2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (acc[i][2 * p + h][e] - mean[i]) * rstd[i] * g[h][e] + be[h][e];
            pk[h][0] = pk2(o[0], o[1]);
            pk[h][1] = pk2(o[2], o[3]);
          }
          // the even group keeps tile 2p and gets the partner's four columns of it, the odd group 2p + 1
          const uint4 v = exchange16(odd, pk[0], pk[1]);
          if (m < M) *(uint4*)(out + m * ldo + c8 + 32 * p) = v;
        }
      }
    } else {
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      const int n = wn * kWN + j * 16 + cq;
      const uint2 gg = *(const uint2*)(gamma + n), bb = *(const uint2*)(beta + n);
      const float g[4] = {bf2f(gg.x & 0xffff), bf2f(gg.x >> 16), bf2f(gg.y & 0xffff), bf2f(gg.y >> 16)};
      const float be[4] = {bf2f(bb.x & 0xffff), bf2f(bb.x >> 16), bf2f(bb.y & 0xffff), bf2f(bb.y >> 16)};
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const long m = mb + 16 * i;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (acc[i][j][e] - mean[i]) * rstd[i] * g[e] + be[e];
        if (m < M) *(uint2*)(out + m * ldo + n) = make_uint2(pk2(o[0], o[1]), pk2(o[2], o[3]));
      }
    }
    }
  }
}

// Selectable forms (NOMIC_RLN): 242 (default) = residual added in the epilogue, 16-B residual
// loads and output stores (EPI 4); 222 = the same with 8-B loads and stores (EPI 0; the default
// until the 16-B form: mixed step 11.89-11.92 -> 11.69-11.74 ms, profiles/encoder_tails); 232 = 222
// with the residual added during the K loop at K = 768 (EPI 3): 10 % faster on the o-proj with a
// cold residual (profiles/r4aq), but in the encoder the residual was just written by the previous
// layer and is warm, and the mixed step measured 12.452 (222) vs 12.500 ms (232) over three
// alternating runs each (profiles/r4ax).
int g_rln_variant = -1;
int rln_pick(int v) { return v == 222 || v == 232 ? v : 242; }
int rln_variant() {
  if (g_rln_variant < 0) {
    const char* e = getenv("NOMIC_RLN");
    g_rln_variant = rln_pick(e && *e ? atoi(e) : 242);
  }
  return g_rln_variant;
}

template <int EPI>
void launch_rln(unsigned blocks, hipStream_t s, const uint16_t* A, long lda, const uint16_t* W, long ldw, int K, long M,
                const uint16_t* res, long ldr, const uint16_t* gamma, const uint16_t* beta, float eps, uint16_t* out,
                long ldo) {
  spl::allow_lds<k_gemm_rln<EPI>>(kLdsBytes);
  hipLaunchKernelGGL(k_gemm_rln<EPI>, dim3(blocks), dim3(kThreads), kLdsBytes, s, A, lda, W, ldw, K, M, res, ldr, gamma,
                     beta, eps, out, ldo);
}

}  // namespace

extern "C" int nomic_gemm_res_ln(const void* A, long lda, const void* W, long ldw, long M, int N, int K,
                                 const void* res, long ldr, const void* gamma, const void* beta, float eps, void* out,
                                 long ldo, hipStream_t s) {
  // shapes the kernel and its grid assume: row-complete 768-wide tiles, whole K stages, 16-B
  // aligned rows, 32-bit DMA offsets
  if (N != kN || K < kBK || K % kBK || M <= 0 || !A || !W || !res || !gamma || !beta || !out)
    return (int)hipErrorInvalidValue;
  if (lda % 8 || ldw % 8 || ldr % 4 || ldo % 4 || lda < K || ldw < K || ldr < N || ldo < N)
    return (int)hipErrorInvalidValue;
  if ((M - 1) * lda + K >= (1L << 32) || (long)kN * ldw >= (1L << 32)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((M + kBM - 1) / kBM);
  const auto* a = (const uint16_t*)A;
  const auto* w = (const uint16_t*)W;
  const auto* r = (const uint16_t*)res;
  const auto* g = (const uint16_t*)gamma;
  const auto* b = (const uint16_t*)beta;
  auto* o = (uint16_t*)out;
  // 16-B epilogue accesses need 16-B aligned rows; where they are not, the 8-B form runs
  const bool wide_ok = ldr % 8 == 0 && ldo % 8 == 0 && ((uintptr_t)res | (uintptr_t)out) % 16 == 0;
  int v = rln_variant();
  if (v == 232 && !(K / kBK >= 24 && K <= 768)) v = 222;
  if (v == 242 && !wide_ok) v = 222;
  if (v == 232) launch_rln<3>(blocks, s, a, lda, w, ldw, K, M, r, ldr, g, b, eps, o, ldo);
  else if (v == 242) launch_rln<4>(blocks, s, a, lda, w, ldw, K, M, r, ldr, g, b, eps, o, ldo);
  else launch_rln<0>(blocks, s, a, lda, w, ldw, K, M, r, ldr, g, b, eps, o, ldo);
  return (int)hipGetLastError();
}

extern "C" int nomic_gemm_res_ln_set_variant(int variant) {
  const int prev = rln_variant();
  g_rln_variant = rln_pick(variant);
  return prev;
}
