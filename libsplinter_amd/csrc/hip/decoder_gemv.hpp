// decoder_gemv.hpp — what the one-token GEMV kernels of decoder_kernels.hip (k_gemv, k_gemv_q4) and their
// per-expert forms in decoder_moe.hip (k_gemv_moe, k_gemv_moe_q4) share besides the loop text itself
// (decoder_body_gemv.hpp, decoder_body_gemv_q4.hpp): the geometry, the row map, the store epilogue and
// the 4- / 8-bit dot products.
#pragma once
#include "decoder_common.hpp"

namespace {

// y[n] = x . W[n, :] for one token.  x (bf16 [K], optionally RMS-normalised in LDS first: the
// dec_rmsnorm + GEMV pair of a layer in one launch) is staged in LDS; each wave owns 4 weight rows
// and streams them with 16-B loads, 4 independent accumulators in flight.  MODE 0: bf16 out,
// 1: + residual (bf16, may alias out: each element is read and written by the same lane),
// 2: SwiGLU over pack_upgate rows (out[o] = up * silu(gate), o -> rows 32(o/16) + o%16 and +16),
// 4: fp32 out (logits).
constexpr int kGemvRows = 4;
constexpr int kGemvMaxK = 16384;

// The row map and the store epilogue shared by k_gemv and k_gemv_q4.  A wave's R weight rows serve
// outputs o0, o0 + 1, ..: row r is output o0 + r, or with MODE 2 the up (r even) / gate (r odd) row
// of output o0 + r / 2 in pack_upgate's 32-row blocks.
template <int MODE, int R>
__device__ __forceinline__ void gemv_rows(int o0, int nout, long (&rows)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int o = o0 + (MODE == 2 ? r / 2 : r);
    if (o >= nout) o = nout - 1;  // tail: recompute the last output, never stored twice
    rows[r] = MODE == 2 ? (long)(32 * (o / 16) + (o % 16) + (r & 1) * 16) : (long)o;
  }
}
// acc: the rows' wave-reduced dot products; lane i stores output o0 + i
template <int MODE, int R>
__device__ __forceinline__ void gemv_store(const float (&acc)[R], int o0, int nout, int lane, const uint16_t* res,
                                           void* out) {
  constexpr int outs = MODE == 2 ? R / 2 : R;
  if (lane < outs) {
    const int o = o0 + lane;
    if (o < nout) {
      float a0 = acc[0], a1 = acc[1];
#pragma unroll
      for (int r = 0; r < R; ++r)
        if ((MODE == 2 ? r / 2 : r) == lane) {
          if (MODE == 2) { if (r & 1) a1 = acc[r]; else a0 = acc[r]; }
          else a0 = acc[r];
        }
      if constexpr (MODE == 4) {
        ((float*)out)[o] = a0;
      } else {
        float y = a0;
        if constexpr (MODE == 1) y += bf2f(res[o]);
        if constexpr (MODE == 2) y = a0 * a1 / (1.f + __expf(-a1));
        ((uint16_t*)out)[o] = __builtin_bit_cast(uint16_t, (__bf16)y);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 4-bit weights (Q4G32): W [N, K] resident in HBM at 0.625 B per weight instead of 2.
//   q  : uint8 [N, K/2]  -- k = 2j in the low nibble of byte j, k = 2j + 1 in the high nibble
//   sm : uint32 [N, K/32] -- per 32-k group, bf16 pair (d low, m high): w = d * q + m
// The decode step is weight-bandwidth bound (every weight read once per token), so the GEMV reads
// 3.2x fewer bytes than the bf16 one.  GGUF Q4_0 / Q4_1 / Q4_K blocks are all affine 4-bit grids
// over 32-weight (sub)blocks, which is the layout this format keeps (reference: llama.cpp reads
// its Q4 weights directly in llama_decode, splainference.cpp:272-330).
// ---------------------------------------------------------------------------
constexpr int kQ4Group = 32;

// nibble pairs -> floats: for one dword of 8 nibbles (k = 0..7), lo bytes hold k = 0,2,4,6 and hi
// bytes k = 1,3,5,7; each byte converts with a single v_cvt_f32_ubyteN
__device__ __forceinline__ float q4dot8(uint32_t w, const float* x) {
  const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;
  float s = (float)(lo & 0xff) * x[0];
  s = fmaf((float)(hi & 0xff), x[1], s);
  s = fmaf((float)((lo >> 8) & 0xff), x[2], s);
  s = fmaf((float)((hi >> 8) & 0xff), x[3], s);
  s = fmaf((float)((lo >> 16) & 0xff), x[4], s);
  s = fmaf((float)((hi >> 16) & 0xff), x[5], s);
  s = fmaf((float)(lo >> 24), x[6], s);
  return fmaf((float)(hi >> 24), x[7], s);
}

constexpr int kGemvQ4MaxK = 16384;
constexpr int kQ4Rec = kQ4Group + 4;  // LDS floats per group record

// 8-bit bytes -> floats, one v_cvt_f32_ubyteN each (Q8G32: k = 4j .. 4j+3 in dword j)
__device__ __forceinline__ float q8dot4(uint32_t w, const float* x) {
  float s = (float)(w & 0xff) * x[0];
  s = fmaf((float)((w >> 8) & 0xff), x[1], s);
  s = fmaf((float)((w >> 16) & 0xff), x[2], s);
  return fmaf((float)(w >> 24), x[3], s);
}

}  // namespace
