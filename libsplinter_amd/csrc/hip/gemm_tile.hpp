// gemm_tile.hpp — what the encoder GEMM files share: the block -> tile order, the SwiGLU formula,
// the dynamic-LDS limit of a kernel, and the entry of the 256x384 register-epilogue kernel
// (gemm384.hip) that gemm_bf16.hip's launcher dispatches to.  The bf16 and lane helpers are in
// bf16_util.hpp, the 32-wide ring K loop of k_gemm_rln and k_gemm384 in gemm_ring32_body.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace spl {

__device__ __forceinline__ void remap_tile(int bid, int nb, int nt, int gn, int& mt, int& ntile) {
  // bijective XCD remap: blocks b and b+8 share an XCD; give each XCD a
  // contiguous range of the linear tile order.  The linear order is
  // band-major: bands of `gn` n-tiles, m-major inside a band, so the ~32
  // tiles an XCD runs at once cover (32/gn) A row-blocks x gn W column-blocks
  // and both fit its 4 MB L2 (gn = nt: plain row-major).
  const int xcd = bid & 7, q = nb >> 3, r = nb & 7;
  const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int per_band = (nb / nt) * gn;
  const int band = wg / per_band, rem = wg - band * per_band;
  mt = rem / gn;
  ntile = band * gn + (rem - mt * gn);
}

// up * silu(g) with a hardware reciprocal and exp2 (v_rcp_f32 + v_exp_f32: no IEEE division
// sequence in the epilogue; ~1 ulp, far below the bf16 output rounding)
__device__ __forceinline__ float swiglu(float up, float g) {
  return up * g * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-g * 1.4426950408889634f));
}

// host: raise kernel F's dynamic-LDS limit to `bytes`, once per kernel
template <auto F>
void allow_lds(int bytes) {
  static const bool once = [bytes] {
    (void)hipFuncSetAttribute((const void*)F, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return true;
  }();
  (void)once;
}

// 256x384 kernel (gemm384.hip).  gemm384_ok: the shapes, strides and alignments it takes (mode is a
// NOMIC_EPI_* value); gemm384_launch assumes them.  gn = n-tiles per band of the tile order.
constexpr int kGemm384BM = 256, kGemm384BN = 384;
bool gemm384_ok(int mode, const void* out, long ldo, long lda, long ldw, long M, int N, int K,
                const float* rope);
int gemm384_launch(int mode, const uint16_t* A, long lda, const uint16_t* W, long ldw, long M, int N, int K,
                   uint16_t* out, long ldo, const float* rope, const int32_t* pos, int rope_cols, int gn,
                   hipStream_t s);

}  // namespace spl
