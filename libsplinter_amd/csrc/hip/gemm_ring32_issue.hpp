// No include guard: the first half of the 32-wide ring K loop of k_gemm_rln (gemm_rln.hip) and of
// k_gemm384's BK = 32 arm (gemm384.hip): the LDS-DMA lambdas, the issue order and the fragment offsets.
// gemm_ring32_body.hpp, the second half, has the loop, the list of names the including kernel defines
// and the explanation of the pipeline.  Two files because k_gemm_rln declares its accumulators and its
// EPI 3 state between the two: declared anywhere else, hipcc allocates the kernel's registers differently.
  const int nk = K / kBK;
  // ring slot of stage t: t % kNW (W), t % kNA (A) -- stages enter each ring in order
  auto glds_w = [&](int t, int i) {
    __builtin_amdgcn_global_load_lds((gbl_void*)(W + (long)t * kBK + offW[i]),
                                     (lds_void*)(smem + (t % kNW) * kWBytes + (wave + kWaves * i) * 1024), 16, 0, 0);
  };
  auto glds_a = [&](int t, int i) {
    __builtin_amdgcn_global_load_lds((gbl_void*)(A + (long)t * kBK + offA[i]),
                                     (lds_void*)(smem + kABase + (t % kNA) * kABytes + (wave + kWaves * i) * 1024),
                                     16, 0, 0);
  };
  // op u (0 .. GA+GW-1) of the loads iteration s issues: stage A(s + LA), then W(s + LW) (the
  // counted wait at the top of an iteration relies on that order)
  static_assert(LW > LA, "an iteration issues its A stage before its W stage");
  constexpr int kOps = GA + GW;
  static_assert(kOps <= kNT, "two DMAs ahead of each of the kNT / 2 MFMA pairs cover a stage's loads");
  auto issue_op = [&](int s, int u) {
    const int tw = s + LW, ta = s + LA;
    if (u < GA) { if (ta >= 0 && ta < nk) glds_a(ta, u); }
    else if (tw >= 0 && tw < nk) glds_w(tw, u - GA);
  };
  auto issue = [&](int s) {
#pragma unroll
    for (int u = 0; u < kOps; ++u) issue_op(s, u);
  };
  // W(t + LW - 1) was issued after A(t): it may stay in flight at the top of iteration t
  auto younger = [&](int t) -> int { return t + LW - 1 < nk ? GW : 0; };

  // fragment read: row = base16 + (lane & 15), logical chunk lane >> 4
  const int fl = (lane & 15) * kRowBytes + (swz(lane & 15, lane >> 4) << 4);
  const int aoff = kABase + (wr * RW) * kRowBytes + fl;
  const int woff = (wn * kWN) * kRowBytes + fl;
