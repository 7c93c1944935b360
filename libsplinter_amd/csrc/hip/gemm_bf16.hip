// gemm_bf16.hip — MFMA bf16 GEMM with fused epilogues for the Nomic-BERT
// encoder (kernels K12/K13/K15/K16 of SURVEY §2.10).
//
//   C[M, N] = A[M, K] . W[N, K]^T      (A activations, W = GGUF weight rows)
//
// Geometry (gfx950): 256 threads = 4 waves in a 2x2 arrangement, block tile
// 128x128, BK = 64; each wave owns a 64x64 sub-tile = 4x4 tiles of
// v_mfma_f32_16x16x32_bf16 with fp32 accumulators.  Both operands are
// K-contiguous, so every MFMA fragment is one 16-B ds_read_b128.
// Staging: global_load_lds_dwordx4 (LDS-DMA) into a double-buffered LDS
// image; the image is lane-linear, so the XOR swizzle (chunk ^= row & 7,
// conflict-free for the ds_read_b128 lane groups) is applied to the GLOBAL
// source address and to the LDS read address (guide rule 21).
// Block -> tile mapping is XCD-aware (bijective remap, guide §5 T1): the tiles
// that share A rows run on one XCD and reuse its L2.
// Epilogue: accumulators go through LDS in fp32, then each thread owns
// 16-B output chunks, so every fused epilogue (residual add, SwiGLU, RoPE)
// works on whole rows with vector loads/stores.  The image -> output step is one
// text for this kernel and the 256x256 one (gemm_epilogue128_body.hpp).
// Shared with gemm384.hip and gemm_rln.hip: the bf16 and lane helpers (bf16_util.hpp), the tile order,
// SwiGLU and allow_lds (gemm_tile.hpp).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "bf16_util.hpp"
#include "gemm_tile.hpp"
#include "glds_asm.hpp"
#include "nomic_api.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kTileBytes = BM * BK * 2;            // 16 KB per operand tile
constexpr int kEpiStride = BN + 4;                 // fp32 epilogue row stride (floats)
constexpr int kLdsBytes = (BM * kEpiStride * 4 > 4 * kTileBytes) ? BM * kEpiStride * 4 : 4 * kTileBytes;

// Stage one BMxBK tile of a K-contiguous matrix (row stride ld elements)
// starting at (row0, k0) into the lane-linear LDS image at `dst`.
__device__ __forceinline__ void stage_tile(const uint16_t* __restrict__ src, long ld, long row0, int k0,
                                           char* dst, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int blk = wave * 4 + i;          // 8-row block of this wave instruction
    const int r = blk * 8 + (lane >> 3);   // row in tile
    const int pc = lane & 7;               // physical 16-B chunk in the 128-B row
    const int c = pc ^ (r & 7);            // logical chunk stored there
    const uint16_t* g = src + (row0 + r) * ld + k0 + c * 8;
    __builtin_amdgcn_global_load_lds((gbl_void*)g, (lds_void*)(dst + blk * 1024), 16, 0, 0);
  }
}

__device__ __forceinline__ bf16x8 lds_frag(const char* tile, int r, int c) {
  return *(const bf16x8*)(tile + r * 128 + ((c ^ (r & 7)) << 4));
}

using spl::remap_tile;  // gemm_tile.hpp

struct EpiArgs {
  uint16_t* out;
  long ldo;
  const uint16_t* res;   // residual [M, N] (mode 1)
  long ldr;
  const float* rope;     // [max_pos, 32] x {cos, sin} interleaved (mode 3)
  const int32_t* pos;    // [M] position of each row (mode 3)
  int rope_cols;         // columns (from 0) that get RoPE (q|k = 1536)
  long M;
  int gn;                // n-tiles per band of the tile order (remap_tile)
  int nsplit;            // k_gemm256: tiles at the end of the dispatch order run as two half-tile blocks
};

using spl::swiglu;  // gemm_tile.hpp

template <int MODE>
__global__ __launch_bounds__(kThreads, 2) void k_gemm_nt(const uint16_t* __restrict__ A, long lda,
                                                         const uint16_t* __restrict__ W, long ldw, int K,
                                                         int mtiles, int ntiles, EpiArgs ep) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int mt, nt;
  remap_tile(blockIdx.x, mtiles * ntiles, ntiles, ep.gn, mt, nt);
  const long m0 = (long)mt * BM, n0 = (long)nt * BN;
  const int wm = wave >> 1, wn = wave & 1;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / BK;
  // LDS: [A0 | B0 | A1 | B1], 16 KB each
  stage_tile(A, lda, m0, 0, smem, wave, lane);
  stage_tile(W, ldw, n0, 0, smem + kTileBytes, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      char* nb = smem + (cur ^ 1) * 2 * kTileBytes;
      stage_tile(A, lda, m0, (kt + 1) * BK, nb, wave, lane);
      stage_tile(W, ldw, n0, (kt + 1) * BK, nb + kTileBytes, wave, lane);
    }
    const char* ta = smem + cur * 2 * kTileBytes;
    const char* tb = ta + kTileBytes;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = lds_frag(ta, wm * 64 + i * 16 + fr, kk * 4 + fq);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = lds_frag(tb, wn * 64 + j * 16 + fr, kk * 4 + fq);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: accumulators -> LDS (fp32) -> 16-B output chunks --------
  float* E = (float*)smem;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        E[(wm * 64 + i * 16 + fq * 4 + r) * kEpiStride + wn * 64 + j * 16 + fr] = acc[i][j][r];
  __syncthreads();

  constexpr int kEpiCols = BN, kEpiThreads = kThreads;
  const long mh = m0;
#include "gemm_epilogue128_body.hpp"  // image rows -> output rows mh .., every mode
}

// ===========================================================================
// 256x256 tile, 8 waves (2M x 4N), 4 phases per K-tile, LDS-DMA prefetch kept
// in flight ACROSS barriers (counted vmcnt, raw s_barrier): the structure of
// the guide's 8-phase template (cdna_hip_programming.md §5 "The 256² 8-phase
// template"), with this kernel's own phase/stage schedule:
//
//   LDS = 2 buffers x [A0 | A1 | B0 | B1] half-tiles (128 rows x BK=64 bf16,
//   16 KB each; XOR-swizzled on the global source address).  Wave (wr, wn)
//   owns rows {qm*128 + wr*64 + 0..63} and cols {qn*128 + wn*32 + 0..31} for
//   quadrants qm, qn in {0,1}, so quadrant (qm, qn) reads only half-tiles
//   A<qm>, B<qn>.  Per K-tile t (buffer t&1):
//     phase 1: read A0,B0 -> MFMA (0,0); stage A1(t+1)
//     phase 2: read B1    -> MFMA (0,1); stage A0(t+2)
//     phase 3: read A1    -> MFMA (1,0); stage B0(t+2)
//     phase 4:               MFMA (1,1); stage B1(t+2)
//   Every half-tile is staged >= 1 phase after its previous contents were
//   read (WAR, separated by a barrier) and read >= 6 phases after it was
//   staged (RAW: the reading phase first waits vmcnt(#glds issued after it),
//   then the barrier).  Up to 6 half-tiles (12 DMA per lane) stay in flight.
// Epilogue: two 128-row halves through one fp32 LDS image (128 x 260).
// Tail split (EpiArgs::nsplit > 0): a grid whose last round would fill at most half the CUs runs
// that round's tiles as two half-tile workgroups each (one 128-row half, 3 half-tiles of DMA and
// 2 quadrant phases per K-tile on a 3-stage LDS ring with its own counted waits: see the half-tile
// branch of the kernel), so the round takes about half a tile time on twice the CUs.
// ===========================================================================
constexpr int kThreads2 = 512;
constexpr int kHalfBytes = 128 * BK * 2;           // 16 KB
constexpr int kBufBytes = 4 * kHalfBytes;          // 64 KB
constexpr int kEpi2Stride = 256 + 4;
constexpr int kLds2Bytes = (128 * kEpi2Stride * 4 > 2 * kBufBytes) ? 128 * kEpi2Stride * 4 : 2 * kBufBytes;
constexpr int kLds2SplitBytes = 9 * kHalfBytes;    // 144 KB: the half-tile blocks' 3-stage ring
static_assert(kLds2SplitBytes >= kLds2Bytes && kLds2SplitBytes <= 160 * 1024, "LDS budget");

__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {  // wave-uniform: scalar branch to an immediate count
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// The LDS-DMAs are issued from inline asm (glds_asm.hpp): with the builtin, hipcc put lgkmcnt(0)
// before every MFMA group of the loop.  Both K loops are peeled (the steady-state K-tiles carry no
// staging branches) and issue their fragment reads in the order the MFMAs consume them (k-step
// 0's B and A fragments first), pinned there, so the first MFMAs wait only for their own operands
// (counted lgkmcnt) instead of the whole phase's reads.
template <int MODE>
__global__ __launch_bounds__(kThreads2, 1) void k_gemm256(const uint16_t* __restrict__ A, long lda,
                                                          const uint16_t* __restrict__ W, long ldw, int K,
                                                          int mtiles, int ntiles, EpiArgs ep) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wn = wave & 3;
  int mt, nt;
  // Tail split: blocks [0, T - nsplit) are whole tiles; the last nsplit tiles of the dispatch order
  // are each computed by two half-tile blocks (qh = their 128-row half) with the highest block
  // indices, so they are dispatched last.  Whole tiles keep remap_tile's XCD banding.  Half block h
  // runs on XCD h & 7 (T - nsplit is a multiple of the CU count, hence of 8), so in every whole
  // group of 16 half blocks, block 8 qh + x takes half qh of the group's tile x: both halves of a
  // tile run on the XCD whose band the tile belongs to.  The < 16 half blocks left over pair up
  // (2 u, 2 u + 1) on neighbouring XCDs; they only lose the band's L2 reuse.
  int bid = blockIdx.x, qh = -1;
  {
    const int nw = mtiles * ntiles - ep.nsplit;
    if (bid >= nw) {
      const int h = bid - nw, full = (ep.nsplit >> 3) << 4;
      if (h < full) {
        bid = nw + ((h >> 4) << 3) + (h & 7);
        qh = (h >> 3) & 1;
      } else {
        bid = nw + (full >> 1) + ((h - full) >> 1);
        qh = (h - full) & 1;
      }
    }
  }
  remap_tile(bid, mtiles * ntiles, ntiles, ep.gn, mt, nt);
  const long m0 = (long)mt * 256, n0 = (long)nt * 256;
  if (qh >= 0 && m0 + qh * 128 >= ep.M) return;  // a half wholly in the row tail (block-uniform)

  // per-lane DMA source offsets (elements): half h, instruction i -> 8-row block (i*8 + wave)
  const int srow = lane >> 3, schunk = ((lane & 7) ^ srow) * 8;
  uint32_t offA[2][2], offB[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = h * 128 + (i * 8 + wave) * 8 + srow;
      const long gr = (m0 + r < ep.M) ? m0 + r : ep.M - 1;  // clamp: tail rows re-read row M-1, never stored
      offA[h][i] = (uint32_t)(gr * lda + schunk);
      offB[h][i] = (uint32_t)((n0 + r) * ldw + schunk);
    }
  auto stage_one = [&](int which, int t, int buf, int i) {  // which: 0 A0, 1 A1, 2 B0, 3 B1
    const uint16_t* base = (which < 2 ? A : W) + (long)t * BK;
    char* dst = smem + buf * kBufBytes + which * kHalfBytes;
    const uint32_t off = which == 0 ? offA[0][i] : which == 1 ? offA[1][i] : which == 2 ? offB[0][i] : offB[1][i];
    spl::glds16_asm(base + off, dst + (i * 8 + wave) * 1024);  // counted LDS waits (glds_asm.hpp)
  };
  auto stage = [&](int which, int t, int buf) {
    stage_one(which, t, buf, 0);
    stage_one(which, t, buf, 1);
  };

  // fragment read addressing: row-in-half R = base16 + (lane&15), chunk kk*4 + (lane>>4), swizzled by R&7 = lane&7
  const int frow = (lane & 15) * 128;
  const int fsw0 = ((0 * 4 + (lane >> 4)) ^ (lane & 7)) << 4;
  const int fsw1 = ((1 * 4 + (lane >> 4)) ^ (lane & 7)) << 4;

  f32x4 acc[2][2][4][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / BK;
  bf16x8 af[4][2], b0[2][2], b1[2][2];
  // one fragment read, pinned where it is written; one k-step of a quadrant's 8 MFMAs
  auto rd = [](bf16x8& dst, const char* p) {
    dst = *(const bf16x8*)p;
    __builtin_amdgcn_sched_barrier(0);
  };
  auto mm = [&](f32x4 (&ac)[4][2], bf16x8 (&bf)[2][2], int kk) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        ac[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][kk], bf[j][kk], ac[i][j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  if (qh >= 0) {
    // ---- half-tile workgroup: rows qh*128 .. +127 of the tile, all 256 columns ----------------
    // LDS = ring of 3 stages x [A<qh> | B0 | B1] half-tiles (48 KB each, 144 KB).  K-tile t lives
    // in slot t % 3 and is staged, in the order A B0 B1 (6 DMA per lane), during K-tile t - 2.
    // Per K-tile t: vmcnt(6) (all but K-tile t + 1's six DMAs have landed: K-tile t is in), ONE
    // barrier, then quadrant (qh, 0) from A, B0 and quadrant (qh, 1) from B1 -- the same K order
    // and MFMA order per output element as the whole tile, so the bits are the same.
    //   RAW: K-tile t is read >= one whole K-tile (2 quadrant phases) after its last DMA was
    //        issued, behind the counted wait and the barrier.
    //   WAR: slot (t + 2) % 3 held K-tile t - 1, whose last reads every wave finished before it
    //        reached K-tile t's barrier; the DMAs into it are issued after that barrier.
    // At most 12 DMA per lane stay in flight.  The accumulators are acc[0][*] for either half.
    constexpr int kStage3 = 3 * kHalfBytes;
    const uint32_t oA[2] = {qh ? offA[1][0] : offA[0][0], qh ? offA[1][1] : offA[0][1]};
    auto hstage = [&](int which, int t, int slot) {  // which: 0 A<qh>, 1 B0, 2 B1
      const uint16_t* base = (which == 0 ? A : W) + (long)t * BK;
      char* dst = smem + slot * kStage3 + which * kHalfBytes;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t off = which == 0 ? oA[i] : which == 1 ? offB[0][i] : offB[1][i];
        spl::glds16_asm(base + off, dst + (i * 8 + wave) * 1024);
      }
    };
    hstage(0, 0, 0); hstage(1, 0, 0); hstage(2, 0, 0);
    if (nk > 1) { hstage(0, 1, 1); hstage(1, 1, 1); hstage(2, 1, 1); }
    int slot = 0, sslot = 2;  // t % 3, (t + 2) % 3
    auto h_kt = [&](int t, auto n1c, auto n2c) {
      constexpr bool n1 = decltype(n1c)::value, n2 = decltype(n2c)::value;
      const char* hA = smem + slot * kStage3;
      const char* pa = hA + (wr * 64) * 128 + frow;
      const char* pb0 = hA + kHalfBytes + (wn * 32) * 128 + frow;
      const char* pb1 = hA + 2 * kHalfBytes + (wn * 32) * 128 + frow;
      wait_vm(n1 ? 6 : 0);
      raw_barrier();
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int fs = kk ? fsw1 : fsw0;
        rd(b0[0][kk], pb0 + fs);
        rd(b0[1][kk], pb0 + 16 * 128 + fs);
#pragma unroll
        for (int i = 0; i < 4; ++i) rd(af[i][kk], pa + i * 16 * 128 + fs);
      }
      if constexpr (n2) hstage(0, t + 2, sslot);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      mm(acc[0][0], b0, 0);
      mm(acc[0][0], b0, 1);
      __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int fs = kk ? fsw1 : fsw0;
        rd(b1[0][kk], pb1 + fs);
        rd(b1[1][kk], pb1 + 16 * 128 + fs);
      }
      if constexpr (n2) hstage(1, t + 2, sslot);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      mm(acc[0][1], b1, 0);
      __builtin_amdgcn_s_setprio(0);
      if constexpr (n2) hstage(2, t + 2, sslot);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      mm(acc[0][1], b1, 1);
      __builtin_amdgcn_s_setprio(0);
      slot = slot == 2 ? 0 : slot + 1;
      sslot = sslot == 2 ? 0 : sslot + 1;
    };
    int t = 0;
    for (; t + 2 < nk; ++t) h_kt(t, std::true_type{}, std::true_type{});
    if (t + 1 < nk) h_kt(t++, std::true_type{}, std::false_type{});
    if (t < nk) h_kt(t, std::false_type{}, std::false_type{});
  } else {
  // prologue, in the steady-state issue order: A0 B0 B1 A1 (t=0), A0 B0 B1 (t=1)
  stage(0, 0, 0); stage(2, 0, 0); stage(3, 0, 0); stage(1, 0, 0);
  if (nk > 1) { stage(0, 1, 1); stage(2, 1, 1); stage(3, 1, 1); }

  auto ls_kt = [&](int t, auto n1c, auto n2c) {
    constexpr bool n1 = decltype(n1c)::value, n2 = decltype(n2c)::value;
    const int buf = t & 1;
    const char* hA0 = smem + buf * kBufBytes;
    const char* hA1 = hA0 + kHalfBytes;
    const char* hB0 = hA0 + 2 * kHalfBytes;
    const char* hB1 = hA0 + 3 * kHalfBytes;
    const char* pb0 = hB0 + (wn * 32) * 128 + frow;
    const char* pb1 = hB1 + (wn * 32) * 128 + frow;
    const char* pa0 = hA0 + (wr * 64) * 128 + frow;
    const char* pa1 = hA1 + (wr * 64) * 128 + frow;
    // ---- phase 1: quadrant (0,0)
    wait_vm(n1 ? 10 : 4);
    raw_barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int fs = kk ? fsw1 : fsw0;
      rd(b0[0][kk], pb0 + fs);
      rd(b0[1][kk], pb0 + 16 * 128 + fs);
#pragma unroll
      for (int i = 0; i < 4; ++i) rd(af[i][kk], pa0 + i * 16 * 128 + fs);
    }
    if constexpr (n1) stage(1, t + 1, buf ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mm(acc[0][0], b0, 0);
    mm(acc[0][0], b0, 1);
    __builtin_amdgcn_s_setprio(0);
    // ---- phase 2: quadrant (0,1)
    wait_vm(n1 ? 10 : 2);
    raw_barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int fs = kk ? fsw1 : fsw0;
      rd(b1[0][kk], pb1 + fs);
      rd(b1[1][kk], pb1 + 16 * 128 + fs);
    }
    if constexpr (n2) stage(0, t + 2, buf);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mm(acc[0][1], b1, 0);
    mm(acc[0][1], b1, 1);
    __builtin_amdgcn_s_setprio(0);
    // ---- phase 3: quadrant (1,0)
    wait_vm(n2 ? 10 : (n1 ? 8 : 0));
    raw_barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int fs = kk ? fsw1 : fsw0;
#pragma unroll
      for (int i = 0; i < 4; ++i) rd(af[i][kk], pa1 + i * 16 * 128 + fs);
    }
    if constexpr (n2) stage(2, t + 2, buf);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mm(acc[1][0], b0, 0);
    mm(acc[1][0], b0, 1);
    __builtin_amdgcn_s_setprio(0);
    // ---- phase 4: quadrant (1,1), registers only (B1's last read was phase 2: a barrier ago)
    if constexpr (n2) stage(3, t + 2, buf);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mm(acc[1][1], b1, 0);
    mm(acc[1][1], b1, 1);
    __builtin_amdgcn_s_setprio(0);
  };
  int t = 0;
  for (; t + 2 < nk; ++t) ls_kt(t, std::true_type{}, std::true_type{});
  if (t + 1 < nk) ls_kt(t++, std::true_type{}, std::false_type{});
  if (t < nk) ls_kt(t, std::false_type{}, std::false_type{});
  }  // whole tile
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue: two 128-row halves through the fp32 LDS image ------------
  // (a half-tile block holds its one half in acc[0] and runs the first pass only, on rows of qh)
  float* E = (float*)smem;
  constexpr int kEpiCols = 256, kEpiThreads = kThreads2;
  const int fq = lane >> 4, fr = lane & 15;
  const long mbase = m0 + (qh > 0 ? 128 : 0);
#pragma unroll
  for (int qm = 0; qm < 2; ++qm) {
    if (qm == 1 && qh >= 0) break;
    __syncthreads();
#pragma unroll
    for (int qn = 0; qn < 2; ++qn)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            E[(wr * 64 + i * 16 + fq * 4 + r) * kEpi2Stride + qn * 128 + wn * 32 + j * 16 + fr] = acc[qm][qn][i][j][r];
    __syncthreads();
    const long mh = mbase + qm * 128;
#include "gemm_epilogue128_body.hpp"  // the same text as k_gemm_nt's, on a 256-column image
  }
}

}  // namespace

namespace {

int g_num_cus = 0;  // MI355X: 256 CUs in 8 XCDs; read from the device on first use
int num_cus() {
  if (g_num_cus <= 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    g_num_cus = n;
  }
  return g_num_cus;
}

// Tail split of the 256^2 kernel (NOMIC_GEMM_TAIL_SPLIT, nomic_gemm_set_tail_split): 1 = a last
// round of R <= CUs / 2 tiles runs as 2 R half-tile blocks of the same launch; 0 = one block per tile
int g_tail_split = -1;
int tail_split() {
  if (g_tail_split < 0) {
    const char* e = getenv("NOMIC_GEMM_TAIL_SPLIT");
    g_tail_split = e && *e ? atoi(e) != 0 : 1;
  }
  return g_tail_split;
}
// tiles of a T-tile grid that run as two half-tile blocks
int split_tiles(long T) {
  const int cus = num_cus(), R = (int)(T % cus);
  return tail_split() && R > 0 && R <= cus / 2 ? R : 0;
}

// Kernel choice (NOMIC_GEMM): 0 = auto, 128 = the 128^2 kernel, 256 = the 256^2 kernel, 384 = the
// 256x384 register-epilogue kernel (gemm384.hip; STORE / SWIGLU / ROPE with N % 384 == 0).
//
// Measured and removed (SwiGLU shape, M = 32768, unless said otherwise):
//   - persistent / stream-K 256^2 kernel (512-515) and the persistent register-epilogue kernel
//     (300, gemm_pt.hip, round 5): slower or equal (profiles/r1_gemm_persistent_ab.jsonl,
//     r2_gemm_streamk_ab.jsonl, r5/gemm_pt_ab_r5c.jsonl)
//   - the lockstep K loop with builtin LDS-DMA and all of a phase's reads before its MFMAs (PP 0):
//     296.5 us against 285.2 for the peeled asm-DMA loop that stayed, qkv 146.9 against 137.4
//     (profiles/r3_gemm_asm_dma.md, r3_gemm_pp2_ab.jsonl)
//   - the staggered ping-pong loop (PP 1: waves 4-7 one barrier behind, a load and an MFMA section
//     per phase): 310.2 against 314.2 us, +1 %, issue stalls turned into barrier waits
//     (profiles/r3_gemm_pp_ab.jsonl)
//   - a phase's two DMAs issued between its MFMA groups (ILV 1-3): -1 % on this kernel, +3 % on the
//     persistent one (profiles/r3_gemm_ilv_ab.jsonl)
//   - SwiGLU applied in registers with a lane-paired bf16 LDS image (EPI 1): 295.7 us, neutral,
//     the epilogue is not the limiter (profiles/r3_gemm_asm_dma.md)
//   - asm DMA in the 128^2 kernel (AS128): 144 against 140 us on the qkv shape
//     (profiles/r3_gemm_asm_dma.md, r3_gemm_asm_dma_rln_128_ab.jsonl)
int g_variant = -1;
int gemm_variant() {
  if (g_variant < 0) {
    const char* e = getenv("NOMIC_GEMM");
    const int v = e ? atoi(e) : 0;
    g_variant = v == 128 || v == 256 || v == 384 ? v : 0;
  }
  return g_variant;
}

// band width of the tile order: the largest divisor of ntiles <= cap (NOMIC_GEMM_GN overrides;
// 0 = row-major)
int band_width(int ntiles, int cap) {
  static const int env = [] {
    const char* v = getenv("NOMIC_GEMM_GN");
    return v && *v ? atoi(v) : -1;
  }();
  if (env == 0) return ntiles;
  if (env > 0) cap = env;
  for (int g = cap < ntiles ? cap : ntiles; g > 1; --g)
    if (ntiles % g == 0) return g;
  return 1;
}

// The 256x384 kernel (gemm384.hip).  n-band of its tile order: 4 (3 at 6 n-tiles); the sweep is flat,
// SwiGLU 269.6 / 266.6 / 265.9 / 266.5 / 268.2 us at 1 / 2 / 4 / 8 / 16, qkv 121.8 / 120.6 / 120.6 /
// 120.2 us at 1 / 2 / 3 / 6 (profiles/gemm384).  Auto rule: the SwiGLU and RoPE modes (the two shapes
// measured) from one whole round of tiles on.  us on 384 / 256^2 / 128^2, K = 768:
//   tokens   SwiGLU (N 6144)            tiles   qkv (N 2304)               tiles
//   32768    267.2 / 300.2 /   -        2048    114.2 / 132.0 /   -         768
//   25000    214.0 / 237.6 / 248.1      1568    110.8 / 109.5 / 111.1       588   (auto ran 128^2: equal)
//    8192     70.2 /  84.1 /  89.2       512     41.5 /  48.7 /  43.4       192   (below a round: stays)
//    4096     40.6 /  44.9 /  49.0       256     36.1 /  30.7 /  28.6        96
//    2048     32.3 /  27.3 /  25.9       128     33.9 /  17.8 /  17.1        48
// Measured and removed: a ring of 4 W + 3 A stages (144 KB) ran 280.6 against 267.2 us (SwiGLU) and
// 122.0 against 114.2 us (qkv) at 32768 tokens.
constexpr int kBand384 = 4;
bool auto384(int mode, long M, int N) {
  if ((mode != NOMIC_EPI_SWIGLU && mode != NOMIC_EPI_ROPE) || N % spl::kGemm384BN) return false;
  return (M + spl::kGemm384BM - 1) / spl::kGemm384BM * (N / spl::kGemm384BN) >= num_cus();
}

template <int MODE>
int launch(const uint16_t* A, long lda, const uint16_t* W, long ldw, long M, int N, int K, EpiArgs ep,
           hipStream_t s) {
  // the 256x384 kernel (K in steps of 32): forced by 384; auto takes it per shape (auto384)
  const int var = gemm_variant();
  if constexpr (MODE == NOMIC_EPI_STORE || MODE == NOMIC_EPI_SWIGLU || MODE == NOMIC_EPI_ROPE) {
    const int nt384 = N / spl::kGemm384BN;
    if ((var == 384 || (var == 0 && auto384(MODE, M, N))) &&
        spl::gemm384_ok(MODE, ep.out, ep.ldo, lda, ldw, M, N, K, ep.rope))
      return spl::gemm384_launch(MODE, A, lda, W, ldw, M, N, K, ep.out, ep.ldo, ep.rope, ep.pos, ep.rope_cols,
                                 band_width(nt384, kBand384), s);
  }
  if (K % BK || N % BN || M <= 0) return (int)hipErrorInvalidValue;
  const long mpad = (M + 255) / 256 * 256;
  const bool fits = N % 256 == 0 && mpad * lda < (1L << 31) && (long)N * ldw < (1L << 31);
  // the 256^2 kernel runs 1 block/CU with a serial prologue / epilogue per tile: it wins once there
  // are several waves of tiles.  From 1024 tiles: the qkv projection at 32768 tokens (1152 tiles)
  // measured 137.4 us on it against 144.5 us on the 128^2 kernel (round-3 trace); the SwiGLU GEMM
  // has 3072.
  const long tiles256 = fits ? (mpad / 256) * (N / 256) : 0;
  static const long min_tiles = [] {  // NOMIC_GEMM256_MIN_TILES (A/B knob)
    const char* e = getenv("NOMIC_GEMM256_MIN_TILES");
    return e && atol(e) > 0 ? atol(e) : 1024L;
  }();
  if (fits && (var == 256 || (var == 0 && tiles256 >= min_tiles))) {
    spl::allow_lds<k_gemm256<MODE>>(kLds2SplitBytes);
    const int mtiles = (int)(mpad / 256), ntiles = N / 256;
    ep.gn = band_width(ntiles, 4);
    ep.nsplit = split_tiles(tiles256);
    // a launch without half-tile blocks is what it was: same grid, same LDS size
    hipLaunchKernelGGL((k_gemm256<MODE>), dim3(mtiles * ntiles + ep.nsplit), dim3(kThreads2),
                       ep.nsplit ? kLds2SplitBytes : kLds2Bytes, s, A, lda, W, ldw, K, mtiles, ntiles, ep);
    return (int)hipGetLastError();
  }
  const int mtiles = (int)((M + BM - 1) / BM), ntiles = N / BN;
  ep.gn = band_width(ntiles, 8);
  hipLaunchKernelGGL(k_gemm_nt<MODE>, dim3(mtiles * ntiles), dim3(kThreads), kLdsBytes, s, A, lda, W, ldw, K, mtiles,
                     ntiles, ep);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int nomic_gemm_set_variant(int variant) {
  const int prev = gemm_variant();
  g_variant = variant == 128 || variant == 256 || variant == 384 ? variant : 0;
  return prev;
}

extern "C" int nomic_gemm_set_tail_split(int on) {
  const int prev = tail_split();
  g_tail_split = on != 0;
  return prev;
}

extern "C" long nomic_gemm256_grid(long M, int N) {
  if (M <= 0 || N <= 0 || N % 256) return 0;
  const long T = (M + 255) / 256 * (N / 256);
  return T + split_tiles(T);
}

extern "C" int nomic_gemm(int mode, const void* A, long lda, const void* W, long ldw, long M, int N, int K, void* out,
                          long ldo, const void* res, long ldr, const float* rope, const int32_t* pos, int rope_cols,
                          hipStream_t s) {
  EpiArgs ep{(uint16_t*)out, ldo, (const uint16_t*)res, ldr, rope, pos, rope_cols, M, 1, 0};
  // operands each mode reads must be there (a launch without them would fault)
  if ((mode == NOMIC_EPI_RESIDUAL && !res) || (mode == NOMIC_EPI_ROPE && (!rope || !pos)))
    return (int)hipErrorInvalidValue;
  const auto* a = (const uint16_t*)A;
  const auto* w = (const uint16_t*)W;
  switch (mode) {
    case NOMIC_EPI_STORE: return launch<NOMIC_EPI_STORE>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_RESIDUAL: return launch<NOMIC_EPI_RESIDUAL>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_SWIGLU: return launch<NOMIC_EPI_SWIGLU>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_ROPE: return launch<NOMIC_EPI_ROPE>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_F32: return launch<NOMIC_EPI_F32>(a, lda, w, ldw, M, N, K, ep, s);
    default: return (int)hipErrorInvalidValue;
  }
}
