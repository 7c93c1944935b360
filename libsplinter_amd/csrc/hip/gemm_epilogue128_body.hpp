// No include guard: the epilogue that k_gemm_nt and k_gemm256 (gemm_bf16.hip) share, as text: 128 rows of
// the fp32 LDS image -> 16-B output chunks, every mode.  k_gemm_nt includes it once, k_gemm256 once per
// 128-row half.  As text and not as a function: through a function template (EpiArgs by reference or by
// value) hipcc allocated the scalar registers of every kernel differently and reordered the epilogues;
// as text all ten kernels keep their instructions (profiles/gemm_epilogue/README.md).
//
// The including kernel has defined:
//   constants   MODE (NOMIC_EPI_*), kEpiCols (columns of the image and of an n-tile: 128 or 256),
//               kEpiThreads (threads of the workgroup)
//   values      E (the image, row stride kEpiCols + 4 floats, complete: a barrier has been passed), tid,
//               mh (output row of image row 0), nt and n0 = nt * kEpiCols (the n-tile and its first GEMM
//               column), ep (EpiArgs)
// Every thread owns 16-B chunks of whole rows, consecutive lanes share a row; rows from ep.M on are not
// written (the row tail).
{
  constexpr int kStride = kEpiCols + 4, kLog = kEpiCols == 256 ? 8 : 7;
  static_assert(kEpiCols == 1 << kLog, "image width");
  if constexpr (MODE == NOMIC_EPI_STORE || MODE == NOMIC_EPI_RESIDUAL) {
#pragma unroll
    for (int it = 0; it < (128 * kEpiCols / 8) / kEpiThreads; ++it) {
      const int q = tid + it * kEpiThreads;
      const int row = q >> (kLog - 3), c8 = (q & (kEpiCols / 8 - 1)) * 8;
      const long gm = mh + row;
      if (gm >= ep.M) continue;
      const float4 v0 = *(const float4*)&E[row * kStride + c8];
      const float4 v1 = *(const float4*)&E[row * kStride + c8 + 4];
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
    // image columns: [up16 | gate16] x kEpiCols / 32 (pack_upgate); they become the kEpiCols / 2 output
    // columns from nt * kEpiCols / 2 on
#pragma unroll
    for (int it = 0; it < (128 * (kEpiCols / 2) / 8) / kEpiThreads; ++it) {
      const int q = tid + it * kEpiThreads;
      const int row = q >> (kLog - 4), oc = (q & (kEpiCols / 16 - 1)) * 8;
      const long gm = mh + row;
      if (gm >= ep.M) continue;
      const int uc = 32 * (oc >> 4) + (oc & 15);
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float up = E[row * kStride + uc + e];
        const float g = E[row * kStride + uc + 16 + e];
        o[e] = swiglu(up, g);
      }
      *(uint4*)(ep.out + gm * ep.ldo + (long)nt * (kEpiCols / 2) + oc) = pack8(o);
    }
  } else if constexpr (MODE == NOMIC_EPI_ROPE) {
    // kEpiCols / 64 heads of 64 columns per image row; NEOX rotation pairs (d, d + 32), which pack_qkv
    // put 16 image columns apart: a head's image columns are [d0-15 | d32-47 | d16-31 | d48-63], the
    // output is in natural order
    constexpr int kHeads = kEpiCols / 64;
#pragma unroll
    for (int it = 0; it < (128 * kHeads * 4) / kEpiThreads; ++it) {
      const int q = tid + it * kEpiThreads;
      const int row = q >> (kLog - 4), head = (q >> 2) & (kHeads - 1), d0 = (q & 3) * 8;
      const long gm = mh + row;
      if (gm >= ep.M) continue;
      const int cb = head * 64;
      const long gcol = n0 + cb;
      const int pc = d0 < 16 ? d0 : d0 + 16;
      float x1[8], x2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x1[e] = E[row * kStride + cb + pc + e];
        x2[e] = E[row * kStride + cb + pc + 16 + e];
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
    for (int it = 0; it < (128 * kEpiCols / 4) / kEpiThreads; ++it) {
      const int q = tid + it * kEpiThreads;
      const int row = q >> (kLog - 2), c4 = (q & (kEpiCols / 4 - 1)) * 4;
      const long gm = mh + row;
      if (gm >= ep.M) continue;
      *(float4*)(outf + gm * ep.ldo + n0 + c4) = *(const float4*)&E[row * kStride + c4];
    }
  }
}
