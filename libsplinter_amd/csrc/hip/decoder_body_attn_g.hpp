// No include guard: the body of k_attn_decode_g (decoder_kernels.hip) and k_attn_decode_g_b
// (decoder_batch.hip), included once by each after its own signature and prologue.  The prologue leaves
// q, K, V, out, ws (this sequence's query row, cache, output row and partials) and L (its key count);
// D, G, SPLIT, ldkv, scale are kernel parameters.
//
// k_attn_decode_g: decode attention for caches of at most kSmallL keys (the single-workgroup regime).
// One workgroup per KV head serves its G query heads, so every K / V row is read once for the group
// instead of once per head, and no phase walks the keys one at a time:
//   scores  hd/8 lanes per key row (16-B pieces), U rows per lane in flight, G dot products per piece,
//           reduced across the row's lanes with xor shuffles -> LDS sc[g][key] (q pre-scaled)
//   softmax one wave per head: max, exp, sum over the keys in LDS
//   P V     the same row pieces of V, U rows in flight, fp32 accumulators per (head, 8 dims), then a
//           reduction over the 256/(hd/8) key groups through LDS.
// k_attn_decode walks each wave's 64 keys serially in P V (a shuffle and a
// 4-B load per key): 28 us per layer at a 300-key cache, llama-7B heads (profiles/r3_decode_splits_short_ctx.jsonl);
// this kernel 11.5 us, q4 decode 0.715 -> 0.577 ms/token (profiles/r3_decode_attn_small_ab.jsonl).  A 16-wave form
// (one load round per phase, shuffle + LDS reduction) measured slower: 14.1 us (r3_decode_attn_small_wide_ab.jsonl).
// Its split form runs the flash-decoding splits of longer caches: 3000-token prompt 0.840 -> 0.672 ms/token at 4 bits
// (profiles/r3_decode_attn_grouped_split_ab.jsonl).
// SPLIT: the same kernel as one split of the flash-decoding form -- workgroup (kvh, j) takes keys
// [j * chunk, (j + 1) * chunk) (chunk <= kSmallL, the k_attn_decode_split geometry) and writes each head's
// partial (max, sum, unnormalised P V) to ws for k_attn_combine.
  constexpr int hd = 64 * D, TPK = hd / 8, KP = 256 / TPK, U = 8;
  static_assert(64 % TPK == 0, "a key row's lanes must sit in one wave");
  int k0 = 0, k1 = L < kSmallL ? L : kSmallL;  // one workgroup: the host picks it only for capacities <= kSmallL
  if constexpr (SPLIT) {
    const int S = gridDim.y, chunk = ((L + S - 1) / S + 63) / 64 * 64;
    k0 = blockIdx.y * chunk;
    k1 = min(L, k0 + min(chunk, kSmallL));  // the host guarantees chunk <= kSmallL
  }
  const int n = k1 > k0 ? k1 - k0 : 0;
  const int kvh = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int sub = tid % TPK, kg = tid / TPK;
  __shared__ float sc[G][kSmallL];
  __shared__ float red[KP][G][hd];
  __shared__ float lsum[G], lmax[G];
  float qv[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float f[8];
    unpack8(*(const uint4*)(q + (long)(kvh * G + g) * hd + sub * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[g][e] = f[e] * scale;
  }
  const uint16_t* Kb = K + (long)kvh * hd + sub * 8 + (long)k0 * ldkv;
  const uint16_t* Vb = V + (long)kvh * hd + sub * 8 + (long)k0 * ldkv;
  // ---- scores
  for (int j0 = 0; j0 < n; j0 += KP * U) {
    uint4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KP + kg;
      r[u] = j < n ? *(const uint4*)(Kb + (long)j * ldkv) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KP + kg;
      float f[8], d[G];
      unpack8(r[u], f);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        d[g] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d[g] = fmaf(f[e], qv[g][e], d[g]);
#pragma unroll
        for (int o = TPK / 2; o >= 1; o >>= 1) d[g] += __shfl_xor(d[g], o, 64);
      }
      if (sub == 0 && j < n) {
#pragma unroll
        for (int g = 0; g < G; ++g) sc[g][j] = d[g];
      }
    }
  }
  __syncthreads();
  // ---- softmax, one wave per head
  for (int g = wave; g < G; g += 4) {
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) mx = fmaxf(mx, sc[g][j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int j = lane; j < n; j += 64) {
      const float p = __expf(sc[g][j] - mx);
      sc[g][j] = p;
      sum += p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) {
      lsum[g] = sum;
      lmax[g] = mx;
    }
  }
  __syncthreads();
  // ---- P V
  float acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  for (int j0 = 0; j0 < n; j0 += KP * U) {
    uint4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KP + kg;
      r[u] = j < n ? *(const uint4*)(Vb + (long)j * ldkv) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KP + kg;
      if (j < n) {
        float f[8];
        unpack8(r[u], f);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float p = sc[g][j];
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(p, f[e], acc[g][e]);
        }
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) red[kg][g][sub * 8 + e] = acc[g][e];
  __syncthreads();
  if constexpr (SPLIT) {
    // ws[head][split][hd + 2] = (max, sum, unnormalised P V): the k_attn_decode_split layout; an empty split
    // leaves max = -inf, sum 0 (k_attn_combine gives it weight 0)
    const int S = gridDim.y;
    for (int idx = tid; idx < G * (hd + 2); idx += 256) {
      const int g = idx / (hd + 2), c = idx - g * (hd + 2);
      float v;
      if (c == 0) v = n ? lmax[g] : -INFINITY;
      else if (c == 1) v = n ? lsum[g] : 0.f;
      else {
        v = 0.f;
#pragma unroll 8
        for (int k = 0; k < KP; ++k) v += red[k][g][c - 2];
      }
      ws[((long)(kvh * G + g) * S + blockIdx.y) * (hd + 2) + c] = v;
    }
  } else {
    for (int idx = tid; idx < G * hd; idx += 256) {
      const int g = idx / hd, d = idx - g * hd;
      float o = 0.f;
#pragma unroll 8
      for (int k = 0; k < KP; ++k) o += red[k][g][d];
      out[(long)(kvh * G + g) * hd + d] = __builtin_bit_cast(uint16_t, (__bf16)(o / lsum[g]));
    }
  }
