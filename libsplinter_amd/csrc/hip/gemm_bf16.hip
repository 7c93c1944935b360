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
// works on whole rows with vector loads/stores.
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
  // LayerNorm fold (nomic_api.h NOMIC_EPI_*_FOLD / RES_*STATS)
  const float2* pin;     // [M][np] (mean, M2) 128-column partials of the rows of A (fold) or of
  int np;                //   res (RES_LN_STATS), as a stats-mode producer wrote them
  float eps;
  const float* c1;       // [N] W' 1       (fold)
  const float* c2;       // [N] W b        (fold)
  const uint16_t* lng;   // [N] LN gamma / beta of res (RES_LN_STATS)
  const uint16_t* lnb;
  float2* part;          // [M][N/128] (mean, M2) of out's rows per 128 columns (RES_*STATS)
  int nsplit;            // k_gemm256: tiles at the end of the dispatch order run as two half-tile blocks
};

constexpr bool is_fold(int m) { return m == NOMIC_EPI_ROPE_FOLD || m == NOMIC_EPI_SWIGLU_FOLD; }
constexpr bool is_stats(int m) { return m == NOMIC_EPI_RES_STATS || m == NOMIC_EPI_RES_LN_STATS; }
constexpr bool is_rope(int m) { return m == NOMIC_EPI_ROPE || m == NOMIC_EPI_ROPE_FOLD; }
constexpr bool is_swiglu(int m) { return m == NOMIC_EPI_SWIGLU || m == NOMIC_EPI_SWIGLU_FOLD; }
constexpr bool is_rowstore(int m) { return m == NOMIC_EPI_STORE || m == NOMIC_EPI_RESIDUAL || is_stats(m); }
constexpr bool needs_rowstats(int m) { return is_fold(m) || m == NOMIC_EPI_RES_LN_STATS; }

// LN fold of one GEMM output: rstd (acc - mean c1[n]) + c2[n]  (== LN(a) . w for the unfolded w)
__device__ __forceinline__ float fold(float acc, float2 st, float c1, float c2) {
  return st.y * (acc - st.x * c1) + c2;
}

// sum over the 16 lanes of a row group (lanes 16k .. 16k+15) on the DPP crossbar (no LDS
// traffic, unlike ds_bpermute): quad_perm [1,0,3,2] and [2,3,0,1] give every lane its quad's sum,
// row_half_mirror (lane i <-> 7-i) the 8-lane sum, row_mirror (i <-> 15-i) the 16-lane sum
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float sum16(float v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  return dpp_add<0x140>(v);
}

__device__ __forceinline__ void load8f(const float* p, float (&o)[8]) {  // p: 32-B aligned
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

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
  // LN modes: the epilogue's per-column vectors are fixed per thread (its column group does not
  // change with the row iteration), so they are loaded here, ahead of the main loop, and the
  // block's 128 row statistics are combined from the producer's partials into LDS behind the
  // main loop (one float2 per row, past the staging / epilogue image: same __shared__ array)
  float cv1[8], cv2[8], cv3[8], cv4[8];
  uint4 lg = {}, lb = {};
  float2 pr[8];
  float2* S = (float2*)(smem + kLdsBytes);
  if constexpr (needs_rowstats(MODE)) {
    const long m = m0 + (tid & 127);
    const long mr = m < ep.M ? m : ep.M - 1;
    if (tid < 128) {
#pragma unroll
      for (int i = 0; i < 8; ++i) pr[i] = i < ep.np ? ep.pin[mr * ep.np + i] : make_float2(0.f, 0.f);
    }
  }
  if constexpr (is_rope(MODE) && is_fold(MODE)) {
    const int head = (tid >> 2) & 1, d0 = (tid & 3) * 8;
    const int pc = d0 < 16 ? d0 : d0 + 16;
    const float* c1 = ep.c1 + n0 + head * 64 + pc;
    const float* c2 = ep.c2 + n0 + head * 64 + pc;
    load8f(c1, cv1); load8f(c2, cv2); load8f(c1 + 16, cv3); load8f(c2 + 16, cv4);
  } else if constexpr (is_swiglu(MODE) && is_fold(MODE)) {
    const int c8 = (tid & 7) * 8, uc = 32 * (c8 >> 4) + (c8 & 15);
    load8f(ep.c1 + n0 + uc, cv1); load8f(ep.c2 + n0 + uc, cv2);
    load8f(ep.c1 + n0 + uc + 16, cv3); load8f(ep.c2 + n0 + uc + 16, cv4);
  } else if constexpr (MODE == NOMIC_EPI_RES_LN_STATS) {
    const int c8 = (tid & 15) * 8;
    lg = *(const uint4*)(ep.lng + n0 + c8);
    lb = *(const uint4*)(ep.lnb + n0 + c8);
  }
  // LDS: [A0 | B0 | A1 | B1], 16 KB each
  stage_tile(A, lda, m0, 0, smem, wave, lane);
  stage_tile(W, ldw, n0, 0, smem + kTileBytes, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (needs_rowstats(MODE)) {
    if (tid < 128) {  // Chan's combination of equal-size partials (as k_row_stats)
      float mean = 0.f, m2 = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) mean += pr[i].x;  // absent partials are zero
      mean /= (float)ep.np;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = pr[i].x - mean;
        if (i < ep.np) m2 += pr[i].y + (float)BN * d * d;
      }
      S[tid] = make_float2(mean, rsqrtf(m2 / ((float)BN * (float)ep.np) + ep.eps));
    }
  }
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

  if constexpr (is_rowstore(MODE)) {
#pragma unroll
    for (int it = 0; it < (BM * BN / 8) / kThreads; ++it) {
      const int q = tid + it * kThreads;
      const int row = q >> 4, c8 = (q & 15) * 8;  // 16 consecutive lanes share a row
      const long gm = m0 + row;
      const bool ok = gm < ep.M;
      if (!is_stats(MODE) && !ok) continue;      // stats modes keep every lane for the shuffles
      const float4 v0 = *(const float4*)&E[row * kEpiStride + c8];
      const float4 v1 = *(const float4*)&E[row * kEpiStride + c8 + 4];
      float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      if constexpr (MODE != NOMIC_EPI_STORE) {
        const long gr = ok ? gm : ep.M - 1;
        const uint4 rr = *(const uint4*)(ep.res + gr * ep.ldr + n0 + c8);
        const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
        float r[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          r[2 * e] = bf2f((uint16_t)(rw[e] & 0xffff));
          r[2 * e + 1] = bf2f((uint16_t)(rw[e] >> 16));
        }
        if constexpr (MODE == NOMIC_EPI_RES_LN_STATS) {
          const float2 st = S[row];
          const uint32_t gw[4] = {lg.x, lg.y, lg.z, lg.w}, bw[4] = {lb.x, lb.y, lb.z, lb.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const uint32_t g2 = gw[e >> 1], b2 = bw[e >> 1];
            const float gf = bf2f((uint16_t)(e & 1 ? g2 >> 16 : g2 & 0xffff));
            const float bf = bf2f((uint16_t)(e & 1 ? b2 >> 16 : b2 & 0xffff));
            r[e] = (r[e] - st.x) * st.y * gf + bf;
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += r[e];
      }
      uint4 o;
      o.x = pk2(v[0], v[1]);
      o.y = pk2(v[2], v[3]);
      o.z = pk2(v[4], v[5]);
      o.w = pk2(v[6], v[7]);
      if (ok) *(uint4*)(ep.out + gm * ep.ldo + n0 + c8) = o;
      if constexpr (is_stats(MODE)) {
        // statistics of the stored (bf16-rounded) values: the consumer folds against exactly them
        const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
        float vr[8], sm = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          vr[e] = bf2f((uint16_t)(e & 1 ? ow[e >> 1] >> 16 : ow[e >> 1] & 0xffff));
          sm += vr[e];
        }
        const float mean = sum16(sm) * (1.f / BN);
        float m2 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) m2 += (vr[e] - mean) * (vr[e] - mean);
        m2 = sum16(m2);
        if (ok && (lane & 15) == 0) ep.part[gm * ntiles + nt] = make_float2(mean, m2);
      }
    }
  } else if constexpr (is_swiglu(MODE)) {
    // block columns: [up16 | gate16] x 4 (pack_upgate) of output columns nt*64 + 0..63
#pragma unroll
    for (int it = 0; it < (BM * 64 / 8) / kThreads; ++it) {
      const int q = tid + it * kThreads;
      const int row = q >> 3, c8 = (q & 7) * 8;
      const long gm = m0 + row;
      if (gm >= ep.M) continue;
      const int uc = 32 * (c8 >> 4) + (c8 & 15);
      float o[8];
      float2 st;
      if constexpr (is_fold(MODE)) st = S[row];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float up = E[row * kEpiStride + uc + e];
        float g = E[row * kEpiStride + uc + 16 + e];
        if constexpr (is_fold(MODE)) {
          up = fold(up, st, cv1[e], cv2[e]);
          g = fold(g, st, cv3[e], cv4[e]);
        }
        o[e] = swiglu(up, g);
      }
      uint4 w;
      w.x = pk2(o[0], o[1]);
      w.y = pk2(o[2], o[3]);
      w.z = pk2(o[4], o[5]);
      w.w = pk2(o[6], o[7]);
      *(uint4*)(ep.out + gm * ep.ldo + (long)nt * 64 + c8) = w;
    }
  } else if constexpr (is_rope(MODE)) {
    // two 64-wide heads per block; NEOX rotation pairs (d, d + 32)
#pragma unroll
    for (int it = 0; it < (BM * 2 * 4) / kThreads; ++it) {
      const int q = tid + it * kThreads;
      const int row = q >> 3, head = (q >> 2) & 1, d0 = (q & 3) * 8;
      const long gm = m0 + row;
      if (gm >= ep.M) continue;
      const int cb = head * 64;
      const long gcol = n0 + cb;
      const int pc = d0 < 16 ? d0 : d0 + 16;  // pack_qkv: [d0-15 | d32-47 | d16-31 | d48-63]
      float x1[8], x2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x1[e] = E[row * kEpiStride + cb + pc + e];
        x2[e] = E[row * kEpiStride + cb + pc + 16 + e];
      }
      if constexpr (is_fold(MODE)) {
        const float2 st = S[row];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          x1[e] = fold(x1[e], st, cv1[e], cv2[e]);
          x2[e] = fold(x2[e], st, cv3[e], cv4[e]);
        }
      }
      if (gcol < ep.rope_cols) {
        const float* cs = ep.rope + (long)ep.pos[gm] * 64 + d0 * 2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float c = cs[2 * e], s = cs[2 * e + 1];
          const float a = x1[e], b = x2[e];
          x1[e] = a * c - b * s;
          x2[e] = b * c + a * s;
        }
      }
      uint4 w1, w2;
      w1.x = pk2(x1[0], x1[1]);
      w1.y = pk2(x1[2], x1[3]);
      w1.z = pk2(x1[4], x1[5]);
      w1.w = pk2(x1[6], x1[7]);
      w2.x = pk2(x2[0], x2[1]);
      w2.y = pk2(x2[2], x2[3]);
      w2.z = pk2(x2[4], x2[5]);
      w2.w = pk2(x2[6], x2[7]);
      *(uint4*)(ep.out + gm * ep.ldo + gcol + d0) = w1;
      *(uint4*)(ep.out + gm * ep.ldo + gcol + d0 + 32) = w2;
    }
  } else if constexpr (MODE == NOMIC_EPI_F32) {
    float* outf = (float*)ep.out;
#pragma unroll
    for (int it = 0; it < (BM * BN / 4) / kThreads; ++it) {
      const int q = tid + it * kThreads;
      const int row = q >> 5, c4 = (q & 31) * 4;
      const long gm = m0 + row;
      if (gm >= ep.M) continue;
      *(float4*)(outf + gm * ep.ldo + n0 + c4) = *(const float4*)&E[row * kEpiStride + c4];
    }
  }
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
    if constexpr (MODE == NOMIC_EPI_STORE || MODE == NOMIC_EPI_RESIDUAL) {
#pragma unroll
      for (int it = 0; it < (128 * 256 / 8) / kThreads2; ++it) {
        const int q = tid + it * kThreads2;
        const int row = q >> 5, c8 = (q & 31) * 8;
        const long gm = mh + row;
        if (gm >= ep.M) continue;
        const float4 v0 = *(const float4*)&E[row * kEpi2Stride + c8];
        const float4 v1 = *(const float4*)&E[row * kEpi2Stride + c8 + 4];
        float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        if constexpr (MODE == NOMIC_EPI_RESIDUAL) {
          const uint4 rr = *(const uint4*)(ep.res + gm * ep.ldr + n0 + c8);
          const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[2 * e] += bf2f((uint16_t)(rw[e] & 0xffff));
            v[2 * e + 1] += bf2f((uint16_t)(rw[e] >> 16));
          }
        }
        *(uint4*)(ep.out + gm * ep.ldo + n0 + c8) = pack8(v);
      }
    } else if constexpr (MODE == NOMIC_EPI_SWIGLU) {
      // block columns [up16 | gate16] x 8 (pack_upgate) -> output columns nt*128 + 0..127
#pragma unroll
      for (int it = 0; it < (128 * 128 / 8) / kThreads2; ++it) {
        const int q = tid + it * kThreads2;
        const int row = q >> 4, oc = (q & 15) * 8;
        const long gm = mh + row;
        if (gm >= ep.M) continue;
        const int uc = 32 * (oc >> 4) + (oc & 15);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float up = E[row * kEpi2Stride + uc + e];
          const float g = E[row * kEpi2Stride + uc + 16 + e];
          o[e] = swiglu(up, g);
        }
        *(uint4*)(ep.out + gm * ep.ldo + (long)nt * 128 + oc) = pack8(o);
      }
    } else if constexpr (MODE == NOMIC_EPI_ROPE) {
      // four 64-wide heads per block; NEOX rotation pairs (d, d + 32)
#pragma unroll
      for (int it = 0; it < (128 * 4 * 4) / kThreads2; ++it) {
        const int q = tid + it * kThreads2;
        const int row = q >> 4, head = (q >> 2) & 3, d0 = (q & 3) * 8;
        const long gm = mh + row;
        if (gm >= ep.M) continue;
        const int cb = head * 64;
        const long gcol = n0 + cb;
        const int pc = d0 < 16 ? d0 : d0 + 16;  // pack_qkv layout
        float x1[8], x2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          x1[e] = E[row * kEpi2Stride + cb + pc + e];
          x2[e] = E[row * kEpi2Stride + cb + pc + 16 + e];
        }
        if (gcol < ep.rope_cols) {
          const float* cs = ep.rope + (long)ep.pos[gm] * 64 + d0 * 2;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float c = cs[2 * e], s = cs[2 * e + 1];
            const float a = x1[e], b = x2[e];
            x1[e] = a * c - b * s;
            x2[e] = b * c + a * s;
          }
        }
        *(uint4*)(ep.out + gm * ep.ldo + gcol + d0) = pack8(x1);
        *(uint4*)(ep.out + gm * ep.ldo + gcol + d0 + 32) = pack8(x2);
      }
    } else if constexpr (MODE == NOMIC_EPI_F32) {
      float* outf = (float*)ep.out;
#pragma unroll
      for (int it = 0; it < (128 * 256 / 4) / kThreads2; ++it) {
        const int q = tid + it * kThreads2;
        const int row = q >> 6, c4 = (q & 63) * 4;
        const long gm = mh + row;
        if (gm >= ep.M) continue;
        *(float4*)(outf + gm * ep.ldo + n0 + c4) = *(const float4*)&E[row * kEpi2Stride + c4];
      }
    }
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
  // has 3072.  The statistics epilogues exist in the 128^2 kernel only.
  constexpr bool k256_ok = MODE <= NOMIC_EPI_F32;
  const long tiles256 = fits ? (mpad / 256) * (N / 256) : 0;
  static const long min_tiles = [] {  // NOMIC_GEMM256_MIN_TILES (A/B knob)
    const char* e = getenv("NOMIC_GEMM256_MIN_TILES");
    return e && atol(e) > 0 ? atol(e) : 1024L;
  }();
  if (k256_ok && fits && (var == 256 || (var == 0 && tiles256 >= min_tiles))) {
    spl::allow_lds<k_gemm256<MODE>>(kLds2SplitBytes);
    const int mtiles = (int)(mpad / 256), ntiles = N / 256;
    ep.gn = band_width(ntiles, 4);
    ep.nsplit = split_tiles(tiles256);
    // a launch without half-tile blocks is what it was: same grid, same LDS size
    if constexpr (k256_ok)
      hipLaunchKernelGGL((k_gemm256<MODE>), dim3(mtiles * ntiles + ep.nsplit), dim3(kThreads2),
                         ep.nsplit ? kLds2SplitBytes : kLds2Bytes, s, A, lda, W, ldw, K, mtiles, ntiles, ep);
    return (int)hipGetLastError();
  }
  const int mtiles = (int)((M + BM - 1) / BM), ntiles = N / BN;
  ep.gn = band_width(ntiles, 8);
  constexpr int lds = kLdsBytes + (needs_rowstats(MODE) ? BM * 8 : 0);
  hipLaunchKernelGGL(k_gemm_nt<MODE>, dim3(mtiles * ntiles), dim3(kThreads), lds, s, A, lda, W, ldw, K, mtiles, ntiles,
                     ep);
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

extern "C" int nomic_gemm_ln(int mode, const void* A, long lda, const void* W, long ldw, long M, int N, int K,
                             void* out, long ldo, const void* res, long ldr, const float* rope, const int32_t* pos,
                             int rope_cols, const float* part_in, int nparts, float eps, const float* c1,
                             const float* c2, const void* ln_g, const void* ln_b, float* part, hipStream_t s) {
  EpiArgs ep{(uint16_t*)out, ldo, (const uint16_t*)res, ldr, rope, pos, rope_cols, M, 1, (const float2*)part_in,
             nparts, eps, c1, c2, (const uint16_t*)ln_g, (const uint16_t*)ln_b, (float2*)part};
  // operands each mode reads must be there (a fold / stats launch without them would fault)
  if ((needs_rowstats(mode) && (!part_in || nparts < 1 || nparts > 8)) || (is_fold(mode) && (!c1 || !c2)) ||
      (is_stats(mode) && (!part || !res || N % BN)) || (mode == NOMIC_EPI_RES_LN_STATS && (!ln_g || !ln_b)) ||
      (mode == NOMIC_EPI_RESIDUAL && !res) || (is_rope(mode) && (!rope || !pos)))
    return (int)hipErrorInvalidValue;
  const auto* a = (const uint16_t*)A;
  const auto* w = (const uint16_t*)W;
  switch (mode) {
    case NOMIC_EPI_STORE: return launch<NOMIC_EPI_STORE>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_RESIDUAL: return launch<NOMIC_EPI_RESIDUAL>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_SWIGLU: return launch<NOMIC_EPI_SWIGLU>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_ROPE: return launch<NOMIC_EPI_ROPE>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_F32: return launch<NOMIC_EPI_F32>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_ROPE_FOLD: return launch<NOMIC_EPI_ROPE_FOLD>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_SWIGLU_FOLD: return launch<NOMIC_EPI_SWIGLU_FOLD>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_RES_STATS: return launch<NOMIC_EPI_RES_STATS>(a, lda, w, ldw, M, N, K, ep, s);
    case NOMIC_EPI_RES_LN_STATS: return launch<NOMIC_EPI_RES_LN_STATS>(a, lda, w, ldw, M, N, K, ep, s);
    default: return (int)hipErrorInvalidValue;
  }
}

extern "C" int nomic_gemm(int mode, const void* A, long lda, const void* W, long ldw, long M, int N, int K, void* out,
                          long ldo, const void* res, long ldr, const float* rope, const int32_t* pos, int rope_cols,
                          hipStream_t s) {
  if (mode > NOMIC_EPI_F32) return (int)hipErrorInvalidValue;  // the LN modes go through nomic_gemm_ln
  return nomic_gemm_ln(mode, A, lda, W, ldw, M, N, K, out, ldo, res, ldr, rope, pos, rope_cols, nullptr, 0, 0.f,
                       nullptr, nullptr, nullptr, nullptr, nullptr, s);
}

namespace {
// one thread per row: Chan's combination of equal-size (128-column) partials
__global__ void k_row_stats(const float2* __restrict__ part, int np, long M, float eps, float2* __restrict__ st) {
  const long m = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const float2* p = part + m * np;
  float mean = 0.f;
  for (int i = 0; i < np; ++i) mean += p[i].x;
  mean /= (float)np;
  float m2 = 0.f;
  for (int i = 0; i < np; ++i) {
    const float d = p[i].x - mean;
    m2 += p[i].y + (float)BN * d * d;
  }
  const float var = m2 / ((float)BN * (float)np);
  st[m] = make_float2(mean, rsqrtf(var + eps));
}
}  // namespace

extern "C" int nomic_row_stats(const float* part, int nparts, long M, float eps, float* st, hipStream_t s) {
  if (nparts <= 0 || M <= 0 || !part || !st) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_row_stats, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, (const float2*)part, nparts, M,
                     eps, (float2*)st);
  return (int)hipGetLastError();
}
