// bf16_util.hpp — the bf16 and lane helpers every kernel file of the encoder and decoder uses: the
// vector and address-space typedefs, bf16 <-> fp32 on packed words, the raw barrier, the lane ^ 16
// move with the 16-B half exchange built on it, and the LDS chunk swizzles of the GEMM images.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

// bf16 bits -> fp32: of a 16-bit value, and of the low half of a word whose high half is clear
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ float bf2f(uint32_t h16) { return __uint_as_float(h16 << 16); }
// fp32 -> bf16, round-to-nearest-even, on the hardware converter (v_cvt_pk_bf16_f32: one
// instruction per PAIR via pk2, instead of a 5-op integer rounding sequence per value)
__device__ __forceinline__ uint32_t f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
__device__ __forceinline__ uint32_t pk2(float a, float b) {
  const bf16x2_t v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ void unpack8(uint4 v, float* f) {
  f[0] = bf2f(v.x & 0xffff); f[1] = bf2f(v.x >> 16);
  f[2] = bf2f(v.y & 0xffff); f[3] = bf2f(v.y >> 16);
  f[4] = bf2f(v.z & 0xffff); f[5] = bf2f(v.z >> 16);
  f[6] = bf2f(v.w & 0xffff); f[7] = bf2f(v.w >> 16);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  return make_uint4(pk2(f[0], f[1]), pk2(f[2], f[3]), pk2(f[4], f[5]), pk2(f[6], f[7]));
}

// s_barrier without the vmcnt(0) / lgkmcnt(0) drain of __syncthreads: the caller's own counted
// waits order its loads
__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// the value of lane ^ 16 (ds_swizzle bit mode: and 0x1f, or 0, xor 0x10 -- a cross-lane move
// on the LDS crossbar that touches no LDS memory)
__device__ __forceinline__ uint32_t xor16(uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F); }

// Lanes l and l ^ 16 (`odd` = bit 4 of the lane) each hold an 8-B piece x and an 8-B piece y.  The
// even lane returns (its x, the partner's x), the odd lane (the partner's y, its y): two 8-B pieces
// per lane become one 16-B piece.  Run on a loaded 16-B piece (x = low half, y = high half) it is
// its own inverse.
__device__ __forceinline__ uint4 exchange16(bool odd, const uint32_t (&x)[2], const uint32_t (&y)[2]) {
  const uint32_t gx = xor16(odd ? x[0] : y[0]), gy = xor16(odd ? x[1] : y[1]);
  return odd ? make_uint4(gx, gy, y[0], y[1]) : make_uint4(x[0], x[1], gx, gy);
}

// physical 16-B chunk of logical chunk c in row r of an LDS image with 64-B rows (swz) and with
// 128-B rows (swz128): 16 distinct bank quads in every ds_read_b128 lane group
__device__ __forceinline__ int swz(int r, int c) { return c ^ ((r >> 1) & 3); }
__device__ __forceinline__ int swz128(int r, int c) { return c ^ ((r >> 1) & 7); }

}  // namespace
