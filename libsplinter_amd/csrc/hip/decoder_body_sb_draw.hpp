// No include guard: the body of k_sb_draw (decoder_kernels.hip) and k_sb_draw_b (decoder_batch.hip),
// included once by each after its own signature and prologue.  The prologue leaves logits and ws at this
// sequence's row and workspace, seed, st (its state record) and host_tok; V, mask, temp, inc_pos are
// kernel parameters.
//
// G: the draw -- the block whose prefix range holds u, then inside its slice (thread t owns the
// contiguous elements [t c, t c + c)) the token; state update as k_sample_reg
  __shared__ float scan[kSbBins];
  __shared__ int pick;
  __shared__ float base_u;
  __shared__ int blk;
  const int tid = threadIdx.x;
  const float M = ws[SB_SCAL + 0], cut = ws[SB_SCAL + 5];
  const float it = 1.f / fmaxf(temp, 1e-6f);
  if (tid == 0) {
    double total = 0.0;
    for (int b = 0; b < kSbBlocks; ++b) total += ws[SB_BPART + b];
    const double u = uniform01(seed, (uint64_t)st[ST_STEP]) * total;
    double run = 0.0;
    int bb = -1;
    for (int b = 0; b < kSbBlocks; ++b) {
      const double p = ws[SB_BPART + b];
      if (p > 0.0) {
        if (u < run + p) { bb = b; break; }
        bb = b;  // rounding at the very end: the last block with mass
      }
      run += p;
    }
    if (bb >= 0 && u >= run + ws[SB_BPART + bb]) run -= ws[SB_BPART + bb];
    blk = bb;
    base_u = (float)(u - run);
    pick = 0x7fffffff;
  }
  __syncthreads();
  const int chunk = (V + kSbBlocks - 1) / kSbBlocks;
  if (blk >= 0) {
    const int b0 = blk * chunk, b1 = min(V, b0 + chunk);
    const int per = (b1 - b0 + kSbBins - 1) / kSbBins;
    const int t0 = b0 + tid * per, t1 = min(b1, t0 + per);
    float part = 0.f;
    for (int i = t0; i < t1; ++i) {
      const float l = sb_logit(logits, mask, i);
      if (l >= cut) part += __expf((l - M) * it);
    }
    scan[tid] = part;
    __syncthreads();
    for (int off = 1; off < kSbBins; off <<= 1) {
      const float x = tid >= off ? scan[tid - off] : 0.f;
      __syncthreads();
      scan[tid] += x;
      __syncthreads();
    }
    const float u = base_u, before = tid ? scan[tid - 1] : 0.f;
    if (part > 0.f && u >= before && (u < scan[tid] || tid == kSbBins - 1 || scan[tid] >= scan[kSbBins - 1])) {
      float run = before;
      int sel = -1;
      for (int i = t0; i < t1; ++i) {
        const float l = sb_logit(logits, mask, i);
        if (l < cut) continue;
        sel = i;
        run += __expf((l - M) * it);
        if (u < run) break;
      }
      if (sel >= 0) atomicMin(&pick, sel);
    }
    __syncthreads();
  }
  if (tid == 0) {
    int t = pick;
    if (t == 0x7fffffff) {  // rounding gap: the most probable token (first block holding the max)
      for (int b = 0; b < kSbBlocks; ++b)
        if (ws[SB_BMAX + b] == M) { t = __float_as_int(ws[SB_BIDX + b]); break; }
    }
    state_commit(st, t, inc_pos, host_tok);
  }
