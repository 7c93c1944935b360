// gemm384.hip — 256x384-tile bf16 GEMM with register epilogues (STORE, SwiGLU, RoPE): the encoder's
// qkv projection (N = 2304 = 6 x 384) and up|gate projection (N = 6144 = 16 x 384).
//
//   C[M, N] = A[M, K] . W[N, K]^T      (A activations, W = packed weight rows)
//
// Why this tile: every GEMM here is co-limited by the per-CU L2 -> LDS fill rate.  A 256x384 tile
// moves 40 KB per 32-wide K step for 48 MFMAs per wave: 154 FLOP per fill byte and 5 LDS-DMA
// wave-instructions per wave per step, against 128 and 6 (per 48 MFMAs) for the 256^2 tile and 110
// and 7 for k_gemm_rln's 128x768.  384 KB of fp32 accumulators (192 per lane at 512 threads) is the
// largest tile a CU holds.  At 32768 tokens both shapes are whole rounds of 256 CUs: 2048 tiles = 8
// rounds (12 on the 256^2 tile) and 768 tiles = 3 rounds (4.5).
//
// Geometry: 512 threads = 8 waves as 4 (rows) x 2 (columns); each wave owns 64 rows x 192 columns =
// 4 x 12 tiles of v_mfma_f32_16x16x32_bf16 with swapped operands (the W fragment is the A operand),
// so a lane's accumulator holds four CONSECUTIVE output columns of one row: k_gemm_rln's per-wave
// layout and fragment read order.
//
// K loop, 32-wide stages (BK = 32; K % 64 != 0, or NOMIC_GEMM384_BK=32): the ring loop it shares with
// k_gemm_rln, one text in gemm_ring32_issue.hpp + gemm_ring32_body.hpp, where the pipeline is explained.
// Here: LDS rings of three W stages (384 x 32 bf16, 24 KB) and two A stages (256 x 32, 16 KB), 104 KB;
// 2 A + 3 W LDS-DMA wave-instructions per wave per stage; 64-B rows with the 16-B chunk c of row r
// stored at c ^ ((r >> 1) & 3), applied to the global source address and to the read address.
//
// K loop, 64-wide stages (BK = 64, the default where K % 64 == 0): two slots of [W 384 rows x 128 B |
// A 256 rows x 128 B], 2 x 80 KB = 160 KB, so one s_waitcnt and one s_barrier per TWO MFMA K-steps (12
// per tile at K = 768 instead of 24) and whole 128-B lines per DMA row piece.  A DMA wave-instruction
// covers 8 rows x 128 B (lane -> row lane >> 3, chunk lane & 7), 4 A + 6 W per wave per stage, LDS
// destination lane-linear 1 KB; chunk c of row r is stored at c ^ ((r >> 1) & 7) (16 distinct bank quads
// in each ds_read_b128 lane group for both K-steps; & 3 gives 8).  A stage is two passes of the 32-wide
// loop's six-pair body, K-step 2T then 2T + 1, so every accumulator sees ascending k in steps of 32
// and the output has the bits of the 32-wide loop.  Ring discipline: iteration T waits vmcnt(0)
// (everything in flight is stage T, issued during iteration T - 1), then one raw barrier; stage T + 1's
// ten pieces then enter the other slot, whose last readers all passed this barrier, two ahead of each
// of the first five MFMA pairs; no barrier follows the last stage.
// Measured (profiles/gemm384_bk64/README.md), 32768 tokens, forms interleaved in one process:
// SwiGLU 268.9 -> 247.9 us, qkv + RoPE 124.6 -> 116.3 us; mixed step 11.22-11.31 -> 10.92-10.97 ms.
// Measured and removed: one piece ahead of each of the first ten pairs: equal on the SwiGLU shape
// (254.1 against 252.9 us), slower on the qkv shape (118.9 against 115.0 us).
//
// Epilogues run from registers, no LDS image.  pack_upgate and pack_qkv place up / gate and the NEOX
// pair (d, d + 32) in n-tiles 2p and 2p + 1 at the same in-tile column, so SwiGLU and RoPE are
// lane-local; lanes l and l ^ 16 hold adjacent 4-column groups of a row and exchange halves
// (exchange16 in bf16_util.hpp: ds_swizzle, no LDS memory), so every store is one 16-B row piece.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>

#include "bf16_util.hpp"
#include "gemm_tile.hpp"
#include "nomic_api.h"

namespace {

constexpr int kBM = spl::kGemm384BM;  // rows per workgroup
constexpr int kBN = spl::kGemm384BN;  // columns per workgroup
constexpr int kBK = 32;               // K per stage
constexpr int kWN = kBN / 2;          // columns per wave (192)
constexpr int kNT = kWN / 16;         // 16-wide n-tiles per wave (12)
constexpr int kThreads = 512;
constexpr int kRowBytes = kBK * 2;            // 64
constexpr int kABytes = kBM * kRowBytes;      // 16 KB per A stage
constexpr int kWBytes = kBN * kRowBytes;      // 24 KB per W stage

__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {  // wave-uniform: a scalar branch to an immediate count
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// NEOX rotation of one pair.  k_gemm256 / k_gemm_nt rotate 8 consecutive d per thread, and hipcc
// contracts six of the eight: x1 = fma(a, c, -(b s)), x2 = fma(b, c, a s); the elements d = 6, 7
// (mod 8) keep every product rounded.  `plain` selects that form, so the three kernels write the
// same bits (profiles/gemm384/README.md).
__device__ __forceinline__ void rotate(float a, float b, float c, float s, bool plain, float& x1, float& x2) {
  float p1, p2;
  {
#pragma clang fp contract(off)
    p1 = a * c - b * s;
    p2 = b * c + a * s;
  }
  float bs, as;
  {
#pragma clang fp contract(off)
    bs = b * s;
    as = a * s;
  }
  const float f1 = __builtin_fmaf(a, c, -bs), f2 = __builtin_fmaf(b, c, as);
  x1 = plain ? p1 : f1;
  x2 = plain ? p2 : f2;
}

struct Epi384 {
  uint16_t* out;
  long ldo;
  const float* rope;   // [max_pos, 32] x {cos, sin} interleaved (ROPE)
  const int32_t* pos;  // [M] position of each row (ROPE)
  int rope_cols;       // columns (from 0) that get RoPE
  long M;
  int gn;              // n-tiles per band of the tile order (spl::remap_tile)
};

// K pipeline: LDS rings of kNW W stages and kNA A stages, one barrier per stage (gemm_ring32_body.hpp).
// Measured and removed: rings of 4 W + 3 A stages (144 KB, counted waits 8 / 5 / 0): 280.6 against
// 267.2 us on the SwiGLU shape, 122.0 against 114.2 us on the qkv shape (profiles/gemm384).
constexpr int kNW = 3, kNA = 2;
constexpr int kLdsBytes = kNW * kWBytes + kNA * kABytes;  // 104 KB: [W ring | A ring]
static_assert(kLdsBytes <= 160 * 1024, "LDS budget");

// 64-wide stages (BK = 64): two slots of [W | A] with 128-B rows, the 16-B chunk c of row r stored at
// c ^ ((r >> 1) & 7) (k_attn3's K image: 16 distinct bank quads in every ds_read_b128 lane group, for
// both K-steps of a stage; (r >> 1) & 3 on 128-B rows does not give that).
constexpr int kWBytes2 = kBN * 128, kABytes2 = kBM * 128;  // 48 KB + 32 KB
constexpr int kSlotBytes = kWBytes2 + kABytes2;
constexpr int kLdsBytes2 = 2 * kSlotBytes;                 // 160 KB
static_assert(kLdsBytes2 <= 160 * 1024, "LDS budget");

template <int MODE, int BK>
__global__ __launch_bounds__(kThreads, 1) void k_gemm384(const uint16_t* __restrict__ A, long lda,
                                                         const uint16_t* __restrict__ W, long ldw, int K,
                                                         int mtiles, int ntiles, Epi384 ep) {
  constexpr int LW = kNW - 1, LA = kNA - 1;            // stages of lead
  constexpr int kABase = kNW * kWBytes;                // LDS: [W ring | A ring]
  constexpr int kWaves = kThreads / 64;                // 8 waves: 4 (rows) x 2 (columns)
  constexpr int RW = kBM / 4, MT = RW / 16;            // rows and m-tiles per wave
  constexpr int GA = kBM / 16 / kWaves, GW = kBN / 16 / kWaves;  // LDS-DMA wave-instructions per wave per stage
  static_assert(GA == 2 && GW == 3 && MT == 4, "wait_vm's cases and the epilogues assume this split");
  static_assert(MODE == NOMIC_EPI_STORE || MODE == NOMIC_EPI_SWIGLU || MODE == NOMIC_EPI_ROPE, "epilogues");
  static_assert(BK == 32 || BK == 64, "K per stage");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wn = wave & 1;
  int mt, nt;
  spl::remap_tile(blockIdx.x, mtiles * ntiles, ntiles, ep.gn, mt, nt);
  const long m0 = (long)mt * kBM, n0 = (long)nt * kBN;
  A += m0 * lda;
  W += n0 * ldw;

  f32x4 acc[MT][kNT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < kNT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (BK == 32) {
    // ---- per-lane LDS-DMA sources: a wave-instruction covers 16 rows x 64 B, lane -> (row, chunk)
    const int drow = lane >> 2, dpc = lane & 3;
    uint32_t offA[GA];
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      const int r = (wave + kWaves * i) * 16 + drow;
      const long gr = (m0 + r < ep.M) ? r : ep.M - 1 - m0;  // tail rows re-read row M-1, never stored
      offA[i] = (uint32_t)(gr * lda + swz(r, dpc) * 8);
    }
    uint32_t offW[GW];
#pragma unroll
    for (int i = 0; i < GW; ++i) {
      const int r = (wave + kWaves * i) * 16 + drow;
      offW[i] = (uint32_t)(r * ldw + swz(r, dpc) * 8);
    }
#define GEMM_RING32_STAGE_HOOK(t)
#include "gemm_ring32_issue.hpp"
#include "gemm_ring32_body.hpp"
#undef GEMM_RING32_STAGE_HOOK
  } else {
    // ---- 64-wide stages: two slots of [W 384 rows x 128 B | A 256 rows x 128 B], one vmcnt(0) and one
    // barrier per two MFMA K-steps.  A DMA wave-instruction covers 8 rows x 128 B (whole lines), lane ->
    // (row lane >> 3, chunk lane & 7); piece p = wave + 8 i holds rows 8 p .. 8 p + 7 at byte 1024 p.
    constexpr int GA2 = kBM / 8 / kWaves, GW2 = kBN / 8 / kWaves, kOps2 = GA2 + GW2;  // 4 A + 6 W pieces
    static_assert(kOps2 <= kNT, "two pieces ahead of each of the first MFMA pairs cover a stage's loads");
    const int drow = lane >> 3, dpc = lane & 7;
    // the XOR term of row 8 (wave + 8 i) + drow is ((wave & 1) << 2) | (drow >> 1) for every i
    const int dsw = swz128(wave * 8 + drow, dpc) * 8;
    uint32_t offA[GA2];
#pragma unroll
    for (int i = 0; i < GA2; ++i) {
      const int r = (wave + kWaves * i) * 8 + drow;
      const long gr = (m0 + r < ep.M) ? r : ep.M - 1 - m0;  // tail rows re-read row M-1, never stored
      offA[i] = (uint32_t)(gr * lda + dsw);
    }
    const uint32_t offW = (uint32_t)((wave * 8 + drow) * ldw + dsw);  // piece i: + 64 i rows, wave-uniform
    const int nk = K / 64;
    // piece u (A pieces, then W pieces) of stage t, into slot t & 1
    auto issue_op = [&](int t, int u) {
      char* slot = smem + (t & 1) * kSlotBytes;
      if (u < GA2)
        __builtin_amdgcn_global_load_lds((gbl_void*)(A + (long)t * 64 + offA[u]),
                                         (lds_void*)(slot + kWBytes2 + (wave + kWaves * u) * 1024), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((gbl_void*)(W + (long)t * 64 + (long)(u - GA2) * (kWaves * 8) * ldw + offW),
                                         (lds_void*)(slot + (wave + kWaves * (u - GA2)) * 1024), 16, 0, 0);
    };
    // fragment read of K-step h: row = base16 + (lane & 15), logical chunk 4 h + (lane >> 4); the
    // h = 1 address is the h = 0 address ^ 64
    const int fl = (lane & 15) * 128 + (swz128(lane & 15, lane >> 4) << 4);
    const int aoff = kWBytes2 + (wr * RW) * 128 + fl;
    const int woff = (wn * kWN) * 128 + fl;

#pragma unroll
    for (int u = 0; u < kOps2; ++u) issue_op(0, u);
    for (int t = 0; t < nk; ++t) {
      // everything in flight is stage t (issued during iteration t - 1); past the barrier stage t is
      // visible to every wave and every wave is done with stage t - 1's slot, which stage t + 1 enters
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      raw_barrier();
      const char* bw = smem + (t & 1) * kSlotBytes;
      // two passes of the 32-wide loop's six-pair body (K-step 2 t, then 2 t + 1): every accumulator
      // sees ascending k.  The A fragments of the second pass replace the first pass's, each behind
      // its last MFMAs in the sixth pair; stage t + 1's pieces go ahead of the first pairs.
      bf16x8 af[MT], w0, w1, x0, x1;
#pragma unroll
      for (int i = 0; i < MT; ++i) af[i] = *(const bf16x8*)(bw + aoff + i * 16 * 128);
      w0 = *(const bf16x8*)(bw + woff);
      w1 = *(const bf16x8*)(bw + woff + 16 * 128);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int q = 0; q < kNT; ++q) {
        const int jp = q % (kNT / 2);
        if (t + 1 < nk) {
#pragma unroll
          for (int u = 2 * q; u < 2 * q + 2; ++u)
            if (u < kOps2) issue_op(t + 1, u);
        }
        if (q + 1 < kNT) {
          const int h1 = (q + 1) / (kNT / 2), j1 = (q + 1) % (kNT / 2);
          x0 = *(const bf16x8*)(bw + (woff ^ (h1 * 64)) + (2 * j1) * 16 * 128);
          x1 = *(const bf16x8*)(bw + (woff ^ (h1 * 64)) + (2 * j1 + 1) * 16 * 128);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          acc[i][2 * jp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, af[i], acc[i][2 * jp], 0, 0, 0);
          acc[i][2 * jp + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, af[i], acc[i][2 * jp + 1], 0, 0, 0);
          if (q == kNT / 2 - 1) af[i] = *(const bf16x8*)(bw + (aoff ^ 64) + i * 16 * 128);
        }
        __builtin_amdgcn_sched_barrier(0);
        w0 = x0;
        w1 = x1;
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }

  // ---- epilogue, from registers ---------------------------------------------------------
  // lane: rows m_i = m0 + wr*64 + i*16 + (lane & 15); columns of n-tile j: wn*192 + j*16 + (lane>>4)*4 + 0..3.
  // For an n-tile pair (x, y) the even 16-lane group takes 8 consecutive columns of x and the odd
  // group those of y: one 16-B store per lane, the half that belongs to the partner lane l ^ 16
  // changes hands by ds_swizzle.
  const int rl = lane & 15, cq = (lane >> 4) * 4;
  const bool odd = (lane >> 4) & 1;
  const int h8 = (lane >> 5) * 8;          // the lane's 8 columns inside a 16-wide n-tile
  const long mb = m0 + wr * RW + rl;       // row of m-tile i: mb + 16 i
  // through a lambda that captures `odd`: called directly, exchange16 changes the code of this kernel
  // (the lane-group test becomes a 32-bit compare and registers move)
  auto exchange = [&](const uint32_t (&x)[2], const uint32_t (&y)[2]) -> uint4 { return exchange16(odd, x, y); };
  if constexpr (MODE == NOMIC_EPI_STORE) {
    uint16_t* o = ep.out + n0 + wn * kWN + (odd ? 16 : 0) + h8;  // + 32 p: n-tiles 2p, 2p + 1
#pragma unroll
    for (int p = 0; p < kNT / 2; ++p)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const long m = mb + 16 * i;
        const uint32_t x[2] = {pk2(acc[i][2 * p][0], acc[i][2 * p][1]), pk2(acc[i][2 * p][2], acc[i][2 * p][3])};
        const uint32_t y[2] = {pk2(acc[i][2 * p + 1][0], acc[i][2 * p + 1][1]),
                               pk2(acc[i][2 * p + 1][2], acc[i][2 * p + 1][3])};
        const uint4 v = exchange(x, y);
        if (m < ep.M) *(uint4*)(o + m * ep.ldo + 32 * p) = v;
      }
  } else if constexpr (MODE == NOMIC_EPI_SWIGLU) {
    // n-tiles [up16 | gate16] x 6 (pack_upgate) -> hidden units (n0 + wn*192) / 2 + 16 p + 0..15;
    // pairs of n-tile pairs (2 q, 2 q + 1) share the exchange
    uint16_t* o = ep.out + (n0 + wn * kWN) / 2 + (odd ? 16 : 0) + h8;  // + 32 q
#pragma unroll
    for (int q = 0; q < kNT / 4; ++q)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const long m = mb + 16 * i;
        uint32_t hk[2][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int p = 2 * q + h;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = spl::swiglu(acc[i][2 * p][e], acc[i][2 * p + 1][e]);
          hk[h][0] = pk2(v[0], v[1]);
          hk[h][1] = pk2(v[2], v[3]);
        }
        const uint4 v = exchange(hk[0], hk[1]);
        if (m < ep.M) *(uint4*)(o + m * ep.ldo + 32 * q) = v;
      }
  } else {
    // three 64-wide heads per wave, n-tiles [d0-15 | d32-47 | d16-31 | d48-63] (pack_qkv): n-tile
    // pair p = 2 head + half holds x1 = d and x2 = d + 32 for d = 16 half + (lane>>4)*4 + 0..3.
    // The even group stores x1's 8 columns at d, the odd group x2's at d + 32 (natural head order).
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const long m = mb + 16 * i;
      const long mr = m < ep.M ? m : ep.M - 1;
      const bool rot = n0 + wn * kWN < ep.rope_cols;  // wave-uniform: a wave past rope_cols reads no table
      const float* cs0 = ep.rope + (rot ? (long)ep.pos[mr] * 64 : 0) + cq * 2;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float4 ca = {}, cb = {};
        if (rot) ca = *(const float4*)(cs0 + half * 32), cb = *(const float4*)(cs0 + half * 32 + 4);
        const float cs[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};  // (cos, sin) of d .. d + 3
#pragma unroll
        for (int head = 0; head < kWN / 64; ++head) {
          const int p = 2 * head + half;
          const long gcol = n0 + wn * kWN + head * 64;
          float x1[4], x2[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            x1[e] = acc[i][2 * p][e];
            x2[e] = acc[i][2 * p + 1][e];
          }
          if (gcol < ep.rope_cols) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              // d mod 8 = (cq & 4) + e: 6, 7 are e = 2, 3 of the odd 16-lane groups
              rotate(x1[e], x2[e], cs[2 * e], cs[2 * e + 1], e >= 2 && odd, x1[e], x2[e]);
            }
          }
          const uint32_t x[2] = {pk2(x1[0], x1[1]), pk2(x1[2], x1[3])};
          const uint32_t y[2] = {pk2(x2[0], x2[1]), pk2(x2[2], x2[3])};
          const uint4 v = exchange(x, y);
          if (m < ep.M) *(uint4*)(ep.out + m * ep.ldo + gcol + (odd ? 32 : 0) + half * 16 + h8) = v;
        }
      }
    }
  }
}

// K per stage (NOMIC_GEMM384_BK): 64 where K is a multiple of 64, else and with 32 the 32-wide loop
int g_bk = -1;
int gemm384_bk() {
  if (g_bk < 0) {
    const char* e = getenv("NOMIC_GEMM384_BK");
    g_bk = e && atoi(e) == 32 ? 32 : 64;
  }
  return g_bk;
}

template <int MODE, int BK>
int launch384_bk(const uint16_t* A, long lda, const uint16_t* W, long ldw, long M, int N, int K, const Epi384& ep,
              hipStream_t s) {
  constexpr int lds = BK == 64 ? kLdsBytes2 : kLdsBytes;
  spl::allow_lds<k_gemm384<MODE, BK>>(lds);
  const int mtiles = (int)((M + kBM - 1) / kBM), ntiles = N / kBN;
  hipLaunchKernelGGL((k_gemm384<MODE, BK>), dim3(mtiles * ntiles), dim3(kThreads), lds, s, A, lda, W, ldw, K, mtiles,
                     ntiles, ep);
  return (int)hipGetLastError();
}

template <int MODE>
int launch384(const uint16_t* A, long lda, const uint16_t* W, long ldw, long M, int N, int K, const Epi384& ep,
              hipStream_t s) {
  if (gemm384_bk() == 64 && K % 64 == 0) return launch384_bk<MODE, 64>(A, lda, W, ldw, M, N, K, ep, s);
  return launch384_bk<MODE, 32>(A, lda, W, ldw, M, N, K, ep, s);
}

}  // namespace

namespace spl {

bool gemm384_ok(int mode, const void* out, long ldo, long lda, long ldw, long M, int N, int K, const float* rope) {
  if (mode != NOMIC_EPI_STORE && mode != NOMIC_EPI_SWIGLU && mode != NOMIC_EPI_ROPE) return false;
  if (M <= 0 || N <= 0 || N % kBN || K % kBK || K < 2 * kBK) return false;
  // 16-B DMA sources and 16-B output row pieces
  if (lda % 8 || ldw % 8 || ldo % 8 || (uintptr_t)out % 16 || lda < K || ldw < K) return false;
  if (mode == NOMIC_EPI_ROPE && (uintptr_t)rope % 16) return false;  // 16-B (cos, sin) loads
  // 32-bit DMA offsets inside a tile, int tile counts
  const long mtiles = (M + kBM - 1) / kBM;
  return (long)kBM * lda < (1L << 31) && (long)kBN * ldw < (1L << 31) && mtiles * (N / kBN) < (1L << 31);
}

int gemm384_launch(int mode, const uint16_t* A, long lda, const uint16_t* W, long ldw, long M, int N, int K,
                   uint16_t* out, long ldo, const float* rope, const int32_t* pos, int rope_cols, int gn,
                   hipStream_t s) {
  const Epi384 ep{out, ldo, rope, pos, rope_cols, M, gn};
  switch (mode) {
    case NOMIC_EPI_STORE: return launch384<NOMIC_EPI_STORE>(A, lda, W, ldw, M, N, K, ep, s);
    case NOMIC_EPI_SWIGLU: return launch384<NOMIC_EPI_SWIGLU>(A, lda, W, ldw, M, N, K, ep, s);
    case NOMIC_EPI_ROPE: return launch384<NOMIC_EPI_ROPE>(A, lda, W, ldw, M, N, K, ep, s);
    default: return (int)hipErrorInvalidValue;
  }
}

}  // namespace spl

extern "C" int nomic_gemm384_set_bk(int bk) {
  const int prev = gemm384_bk();
  g_bk = bk == 32 ? 32 : 64;
  return prev;
}
