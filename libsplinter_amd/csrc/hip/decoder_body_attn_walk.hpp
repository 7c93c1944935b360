// No include guard: the body of k_attn_decode (decoder_kernels.hip) and k_attn_decode_b (decoder_batch.hip),
// included once by each after its own signature and prologue.  The prologue leaves q, K, V, out (this
// sequence's query row, cache and output row) and L (its key count); DPL, ldkv, grp, hd, scale are kernel
// parameters.  DEC_SLOTS is defined by decoder_batch.hip.
//
// Single-token decode attention over the KV cache (GQA): one 1024-thread workgroup per
// query head h (kv head h / (H/KVH)); its 16 waves take interleaved 64-key chunks (a decode
// step launches only H workgroups, so the split-L width lives inside the workgroup).  Inside a
// chunk each lane scores one key (16-B loads along its cache row against the LDS-resident,
// pre-scaled q), the wave keeps an online softmax (max/sum via __shfl_xor), and the V rows
// are accumulated with p broadcast by __shfl, each lane owning DPL = hd/64 contiguous
// output dims.  The 16 partial (m, l, acc) states merge in LDS.  K/V are [L, ldkv] rows
// (ldkv = KVH*hd elements) starting at the kv head's column.
  const int h = blockIdx.x;
  const int kvh = h / grp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __shared__ float qs[256];
  __shared__ float wm[kDecWaves], wl[kDecWaves];
  __shared__ float wacc[kDecWaves][256];
  for (int d = threadIdx.x; d < hd; d += kDecWaves * 64) qs[d] = bf2f(q[(long)h * hd + d]) * scale;
  __syncthreads();
  const uint16_t* Kb = K + (long)kvh * hd;
  const uint16_t* Vb = V + (long)kvh * hd + lane * DPL;
  float m = -INFINITY, l = 0.f, acc[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
  for (int base = wave * 64; base < L; base += kDecWaves * 64) {
    const int j = base + lane;
    float s = -INFINITY;
    if (j < L) {
      const uint16_t* kr = Kb + (long)j * ldkv;
      // hd == 64 * DPL: the key row in batches of 8 16-B loads issued before their FMAs (a
      // runtime-bound loop issued them one latency at a time: 28 us per step at 32 heads); one batch
      // in flight keeps the 1024-thread block inside its 128 VGPRs
      float dot = 0.f;
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
          for (int e = 0; e < 8; ++e) dot += f[e] * qs[cb * 64 + c * 8 + e];
        }
      }
      s = dot;
    }
    float cm = s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
    const float mn = fmaxf(m, cm);  // finite: lane 0 of every visited chunk holds a key
    const float corr = __expf(m - mn);
    const float p = j < L ? __expf(s - mn) : 0.f;
    float ps = p;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
    l = l * corr + ps;
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[i] *= corr;
    const int nv = min(64, L - base);
    for (int t = 0; t < nv; ++t) {
      const float pt = __shfl(p, t, 64);
      const uint16_t* vr = Vb + (long)(base + t) * ldkv;
#pragma unroll
      for (int i = 0; i < DPL; ++i) acc[i] += pt * bf2f(vr[i]);
    }
    m = mn;
  }
  if (lane == 0) { wm[wave] = m; wl[wave] = l; }
#pragma unroll
  for (int i = 0; i < DPL; ++i) wacc[wave][lane * DPL + i] = acc[i];
  __syncthreads();
  float M = wm[0];
#pragma unroll
  for (int w = 1; w < kDecWaves; ++w) M = fmaxf(M, wm[w]);
  float c[kDecWaves], den = 0.f;
#pragma unroll
  for (int w = 0; w < kDecWaves; ++w) {
#ifdef DEC_SLOTS
    c[w] = wm[w] == -INFINITY ? 0.f : __expf(wm[w] - M);  // a wave past the slot's keys adds nothing
#else
    c[w] = __expf(wm[w] - M);  // no guard here since the kernel was written; adding it changes its instructions
#endif
    den += wl[w] * c[w];
  }
  const float inv = 1.f / den;
  for (int d = threadIdx.x; d < hd; d += kDecWaves * 64) {
    float o = 0.f;
#pragma unroll
    for (int w = 0; w < kDecWaves; ++w) o += wacc[w][d] * c[w];
    o *= inv;
    out[(long)h * hd + d] = __builtin_bit_cast(uint16_t, (__bf16)o);
  }
