// No include guard: the body of k_attn_decode_split (decoder_kernels.hip) and k_attn_decode_split_b
// (decoder_batch.hip), included once by each after its own signature and prologue.  The prologue leaves
// q, K, V, ws (this sequence's query row, cache and partials) and L (its key count); DPL, G, ldkv, grp,
// scale are kernel parameters.
//
// Split-L decode attention (flash-decoding) for long caches: grid (H / G, S), workgroup (h, j) of 4 waves
// scores keys [j c, (j + 1) c) with c = ceil(L / S) rounded up to 64 and writes its unnormalised
// partial (m, l, acc[hd]) to ws; k_attn_combine merges the S partials of a head.  One workgroup per
// head streams the whole cache through one CU (164 GB/s at L = 8192, profiles/r2_decode_q4.md).
// The chunk walk is k_attn_decode's, written out again on purpose: moved into one inlined function,
// even word for word, it allocates other registers in 8 of the 20 kernels
// (profiles/decoder_prune/README.md).
  // G query heads of one kv group per workgroup (grouped-query attention): every key and value row
  // is loaded once for all G heads instead of once per head
  constexpr int hd = 64 * DPL;
  const int h0 = blockIdx.x * G, S = gridDim.y, j = blockIdx.y;
  const int kvh = h0 / grp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int chunk = ((L + S - 1) / S + 63) / 64 * 64;
  const int k0 = j * chunk, k1 = min(L, k0 + chunk);
  __shared__ float qs[G][hd];
  __shared__ float wm[kSplitWaves][G], wl[kSplitWaves][G];
  __shared__ float wacc[kSplitWaves][G][hd];
  for (int d = threadIdx.x; d < G * hd; d += kSplitWaves * 64) qs[d / hd][d % hd] = bf2f(q[(long)h0 * hd + d]) * scale;
  __syncthreads();
  const uint16_t* Kb = K + (long)kvh * hd;
  const uint16_t* Vb = V + (long)kvh * hd + lane * DPL;
  float m[G], l[G], acc[G][DPL];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[g][i] = 0.f;
  }
  for (int base = k0 + wave * 64; base < k1; base += kSplitWaves * 64) {
    const int jj = base + lane;
    float sc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sc[g] = -INFINITY;
    if (jj < k1) {
      const uint16_t* kr = Kb + (long)jj * ldkv;
      float dot[G];
#pragma unroll
      for (int g = 0; g < G; ++g) dot[g] = 0.f;
#pragma unroll 1
      for (int cb = 0; cb < DPL; ++cb) {
        uint4 kv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) kv[c] = *(const uint4*)(kr + cb * 64 + c * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          float f[8];
          unpack8(kv[c], f);
#pragma unroll
          for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) dot[g] += f[e] * qs[g][cb * 64 + c * 8 + e];
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) sc[g] = dot[g];
    }
    float p[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float cm = sc[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
      const float mn = fmaxf(m[g], cm);
      const float corr = __expf(m[g] - mn);
      p[g] = jj < k1 ? __expf(sc[g] - mn) : 0.f;
      float ps = p[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
      l[g] = l[g] * corr + ps;
#pragma unroll
      for (int i = 0; i < DPL; ++i) acc[g][i] *= corr;
      m[g] = mn;
    }
    const int nv = min(64, k1 - base);
    for (int t = 0; t < nv; ++t) {
      const uint16_t* vr = Vb + (long)(base + t) * ldkv;
      float vv[DPL];
#pragma unroll
      for (int i = 0; i < DPL; ++i) vv[i] = bf2f(vr[i]);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pt = __shfl(p[g], t, 64);
#pragma unroll
        for (int i = 0; i < DPL; ++i) acc[g][i] += pt * vv[i];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (lane == 0) { wm[wave][g] = m[g]; wl[wave][g] = l[g]; }
#pragma unroll
    for (int i = 0; i < DPL; ++i) wacc[wave][g][lane * DPL + i] = acc[g][i];
  }
  __syncthreads();
  for (int g = 0; g < G; ++g) {
    float M = wm[0][g];
#pragma unroll
    for (int w = 1; w < kSplitWaves; ++w) M = fmaxf(M, wm[w][g]);
    float* o = ws + ((long)(h0 + g) * S + j) * (hd + 2);
    float c[kSplitWaves], den = 0.f;
#pragma unroll
    for (int w = 0; w < kSplitWaves; ++w) {
      c[w] = wm[w][g] == -INFINITY ? 0.f : __expf(wm[w][g] - M);  // an empty wave (or split) adds nothing
      den += wl[w][g] * c[w];
    }
    for (int d = threadIdx.x; d < hd; d += kSplitWaves * 64) {
      float a = 0.f;
#pragma unroll
      for (int w = 0; w < kSplitWaves; ++w) a += wacc[w][g][d] * c[w];
      o[2 + d] = a;
    }
    if (threadIdx.x == 0) { o[0] = M; o[1] = den; }
  }
