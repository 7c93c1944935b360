// decoder_body_gemv.hpp — the body of k_gemv (decoder_kernels.hip) and k_gemv_moe (decoder_moe.hip).
// In scope: constexpr MODE, RMS; x, rw, eps, W (the [N, K] matrix whose rows this launch reads), K, nout,
// res, out.
  __shared__ __attribute__((aligned(16))) uint16_t xs[kGemvMaxK];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch = K >> 3;
  // this wave's outputs and their weight rows; the first chunk of every row is requested BEFORE x
  // is staged, so its HBM latency overlaps the staging and the barriers (as k_gemv_q4)
  constexpr int outs = MODE == 2 ? kGemvRows / 2 : kGemvRows;
  const int o0 = (blockIdx.x * 4 + wave) * outs;
  const bool active = o0 < nout;
  long rows[kGemvRows];
  gemv_rows<MODE>(o0, nout, rows);
  uint4 wv[kGemvRows];
  if (active && lane < nch) {
#pragma unroll
    for (int r = 0; r < kGemvRows; ++r) wv[r] = *(const uint4*)(W + rows[r] * K + lane * 8);
  }
  float ss = 0.f;
  for (int c = tid; c < nch; c += 256) {
    const uint4 v = *(const uint4*)(x + c * 8);
    *(uint4*)(xs + c * 8) = v;
    if constexpr (RMS) {
      float f[8];
      unpack8(v, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss += f[e] * f[e];
    }
  }
  if constexpr (RMS) {
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float rs = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + eps);
    for (int c = tid; c < nch; c += 256) {  // each thread rewrites the chunks it staged
      float f[8];
      unpack8(*(const uint4*)(xs + c * 8), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = f[e] * rs * rw[c * 8 + e];
      *(uint4*)(xs + c * 8) = pack8(f);
    }
  }
  __syncthreads();
  if (!active) return;
  float acc[kGemvRows] = {};
  for (int c = lane; c < nch; c += 64) {
    uint4 cw[kGemvRows];
#pragma unroll
    for (int r = 0; r < kGemvRows; ++r) cw[r] = wv[r];
    if (c + 64 < nch) {  // one chunk of look-ahead per row
#pragma unroll
      for (int r = 0; r < kGemvRows; ++r) wv[r] = *(const uint4*)(W + rows[r] * K + (c + 64) * 8);
    }
    float xf[8];
    unpack8(*(const uint4*)(xs + c * 8), xf);
#pragma unroll
    for (int r = 0; r < kGemvRows; ++r) {
      float wf[8];
      unpack8(cw[r], wf);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[r] += wf[e] * xf[e];
    }
  }
#pragma unroll
  for (int r = 0; r < kGemvRows; ++r) acc[r] = wave_sum(acc[r]);
  gemv_store<MODE>(acc, o0, nout, lane, res, out);
