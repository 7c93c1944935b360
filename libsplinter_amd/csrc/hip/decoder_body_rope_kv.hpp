// No include guard: the body of k_rope_kv (decoder_kernels.hip) and k_rope_kv_b (decoder_batch.hip),
// included once by each after its own signature and prologue.  The prologue leaves qkv, kc, vc at this
// sequence's qkv row and layer cache and p, its position; H, KVH, hd, cs, sn, ldkv are kernel parameters.
//
// RoPE of the step's q (in place) and k at position p, and the k / v rows appended to the
// layer's KV cache (row p of [n_ctx, ldkv]).  One thread per rotation pair / per 8 v elements.
  const int half = hd >> 1;
  const int npairs = (H + KVH) * half;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npairs + KVH * hd; i += gridDim.x * blockDim.x) {
    if (i < npairs) {
      const int head = i / half, j = i - head * half;
      uint16_t* ptr = qkv + (long)head * hd + 2 * j;
      const float a = bf2f(ptr[0]), b = bf2f(ptr[1]);
      const float c = cs[p * half + j], s = sn[p * half + j];
      const uint16_t y0 = __builtin_bit_cast(uint16_t, (__bf16)(a * c - b * s));
      const uint16_t y1 = __builtin_bit_cast(uint16_t, (__bf16)(a * s + b * c));
      if (head < H) {
        ptr[0] = y0;
        ptr[1] = y1;
      } else {
        uint16_t* kr = kc + p * ldkv + (long)(head - H) * hd + 2 * j;
        kr[0] = y0;
        kr[1] = y1;
      }
    } else {
      const int e = i - npairs;
      vc[p * ldkv + e] = qkv[(long)(H + KVH) * hd + e];
    }
  }
