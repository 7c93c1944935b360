// decoder_body_gemv_q4.hpp — the body of k_gemv_q4 (decoder_kernels.hip) and k_gemv_moe_q4 (decoder_moe.hip).
// In scope: constexpr MODE, RMS, BITS; x, rw, eps, Wq / Wsm (the planes of the [N, K] matrix whose rows this
// launch reads), K, nout, res, out.
  // dynamic LDS, fp32, one 36-float record per 32-k group: x[32], the group sum, 3 pad.  The
  // 144-B record stride keeps the main loop's per-lane ds_read_b128 of consecutive groups
  // conflict-free (16-lane phases start on 16 distinct 4-bank quads).
  extern __shared__ __attribute__((aligned(16))) float xs[];
  __shared__ float red[4];
  constexpr int R = kGemvRows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch = K >> 3, ng = K / kQ4Group;
  // this wave's weight rows, and its first group's weights requested BEFORE x is staged: the HBM
  // latency of the first loads overlaps the staging and its barriers
  constexpr int outs = MODE == 2 ? R / 2 : R;
  const int o0 = (blockIdx.x * 4 + wave) * outs;
  const bool active = o0 < nout;
  long rows[R];
  gemv_rows<MODE>(o0, nout, rows);
  constexpr int GV = BITS / 4;  // 16-B loads per group and row
  const long qrow = (long)K * BITS / 8;
  uint4 wq[R][GV];
  uint32_t sm[R];
  if (active && lane < ng) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int v = 0; v < GV; ++v) wq[r][v] = *(const uint4*)(Wq + rows[r] * qrow + lane * 16 * GV + v * 16);
      sm[r] = Wsm[rows[r] * ng + lane];
    }
  }
  float ss = 0.f;
  for (int c = tid; c < nch; c += 256) {
    float f[8];
    unpack8(*(const uint4*)(x + c * 8), f);
    float* px = xs + (c >> 2) * kQ4Rec + (c & 3) * 8;
    *(float4*)px = make_float4(f[0], f[1], f[2], f[3]);
    *(float4*)(px + 4) = make_float4(f[4], f[5], f[6], f[7]);
    if constexpr (RMS) {
#pragma unroll
      for (int e = 0; e < 8; ++e) ss += f[e] * f[e];
    }
  }
  float rs = 1.f;
  if constexpr (RMS) {
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    rs = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + eps);
  }
  // each thread revisits the chunks it staged: RMS scaling (x * rs * w rounded to bf16, as the bf16
  // path feeds its GEMV) and the 32-group sums over the 4 consecutive lanes holding a group's chunks
  // (nch % 4 == 0 and the stride 256 keep a group's 4 lanes active together)
  for (int c = tid; c < nch; c += 256) {
    float* px = xs + (c >> 2) * kQ4Rec + (c & 3) * 8;
    float4 a = *(const float4*)px, b = *(const float4*)(px + 4);
    if constexpr (RMS) {
      const float4 wa = *(const float4*)(rw + c * 8), wb = *(const float4*)(rw + c * 8 + 4);
      a = make_float4((float)(__bf16)(a.x * rs * wa.x), (float)(__bf16)(a.y * rs * wa.y),
                      (float)(__bf16)(a.z * rs * wa.z), (float)(__bf16)(a.w * rs * wa.w));
      b = make_float4((float)(__bf16)(b.x * rs * wb.x), (float)(__bf16)(b.y * rs * wb.y),
                      (float)(__bf16)(b.z * rs * wb.z), (float)(__bf16)(b.w * rs * wb.w));
      *(float4*)px = a;
      *(float4*)(px + 4) = b;
    }
    float s = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if ((c & 3) == 0) xs[(c >> 2) * kQ4Rec + kQ4Group] = s;
  }
  __syncthreads();
  if (!active) return;
  float acc[R] = {};
  for (int g = lane; g < ng; g += 64) {
    // the group's weights are in registers; request the next group's before the math (one group
    // of look-ahead per lane: 2 x 4 x 20 B in flight)
    uint4 cq[R][GV];
    uint32_t csm[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int v = 0; v < GV; ++v) cq[r][v] = wq[r][v];
      csm[r] = sm[r];
    }
    if (g + 64 < ng) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int v = 0; v < GV; ++v) wq[r][v] = *(const uint4*)(Wq + rows[r] * qrow + (g + 64) * 16 * GV + v * 16);
        sm[r] = Wsm[rows[r] * ng + g + 64];
      }
    }
    float xg[kQ4Group];
#pragma unroll
    for (int e = 0; e < kQ4Group; e += 4) *(float4*)(xg + e) = *(const float4*)(xs + g * kQ4Rec + e);
    const float gs = xs[g * kQ4Rec + kQ4Group];
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
      acc[r] = fmaf(bf2f(csm[r] & 0xffff), dot, fmaf(bf2f(csm[r] >> 16), gs, acc[r]));
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
  gemv_store<MODE>(acc, o0, nout, lane, res, out);
