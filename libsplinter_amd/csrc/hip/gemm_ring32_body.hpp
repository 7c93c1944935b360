// No include guard: the 32-wide ring K loop of k_gemm_rln (gemm_rln.hip) and of k_gemm384's BK = 32 arm
// (gemm384.hip): the prologue issues and the loop over the K stages.  Each kernel includes
// gemm_ring32_issue.hpp (the DMA lambdas, the issue order, the fragment offsets) after its own prologue
// and this file after that.  As text and not as a function: the kernels sit at 254-255 registers with two
// waves per SIMD, and with the loop in a shared template hipcc spilled 35-40 registers in k_gemm_rln
// (profiles/gemm384/README.md).
//
// The including kernel has defined, before gemm_ring32_issue.hpp:
//   constants   kBK (32), kRowBytes (64), kWBytes / kABytes (bytes per W / A stage), kNW / kNA (ring
//               lengths, 3 / 2), LW = kNW - 1, LA = kNA - 1 (stages of lead), kABase (LDS: [W ring | A
//               ring]), kWaves (8), GA / GW (LDS-DMA wave-instructions per wave per A / W stage), kWN and
//               kNT (columns and 16-wide n-tiles per wave), RW and MT (rows and m-tiles per wave)
//   values      A, W (k_gemm384: advanced to the tile origin; k_gemm_rln: the matrices), K, smem, lane,
//               wave, wr / wn (the wave's row / column in the workgroup), offA[GA] / offW[GW] (per-lane
//               DMA source offsets in elements: row * ld + swz(row, lane & 3) * 8)
//   functions   wait_vm(n) with a case for GW; swz, raw_barrier (bf16_util.hpp)
// and before this file:
//   values      acc[MT][kNT], zeroed
//   hook        GEMM_RING32_STAGE_HOOK(t): statements of iteration t between its barrier and its MFMAs
//               (k_gemm_rln's EPI 3 residual pieces; empty in k_gemm384).  Vector loads it issues are
//               older than the iteration's DMAs, so the counted wait stays exact.
// It leaves acc holding the K sum; a kernel that reuses the LDS afterwards passes a barrier first.
//
// Pipeline: LDS rings of kNW W stages and kNA A stages, one barrier per stage.  Iteration t, after its
// barrier, issues the stages A(t + LA) and W(t + LW) into ring slots last read in iteration t - 1, then
// computes stage t.  W -- L2-resident, re-read by every workgroup -- runs two stages ahead; A -- streamed
// from HBM, read once -- one; a ring holds one slot more than its lead, and the longer rings that were
// measured are in the notes of the kernel they were measured on.  Ring discipline: a staged slot is read
// only after the issuing wave's counted wait and a barrier the reader has passed; a slot is restaged only
// after a barrier that follows its last read.
//
// The counted wait is exact because of the issue order.  Iteration s issues A(s + LA) first, then
// W(s + LW).  At the top of iteration t the loads a wave may still have in flight are, oldest first,
// W(t) [iteration t - 2], A(t) and W(t + 1) [iteration t - 1]: everything stage t needs is older than
// the GW pieces of W(t + LW - 1), so vmcnt(GW) waits for exactly stage t and leaves W(t + 1) flying
// (`younger`; 0 once no such stage exists).  Swapping issue_op's A and W arms breaks this silently.
//
// The stage's GA + GW DMAs go two ahead of each of the first MFMA pairs, in issue order: issued together
// after the barrier they held both waves of a SIMD off the matrix core for the ~100-cycle issue cost of
// each.
  for (int s = -LW; s < 0; ++s) issue(s);
  for (int t = 0; t < nk; ++t) {
    wait_vm(younger(t));
    raw_barrier();  // stage t visible to every wave; every wave is done with stage t-1's slots
    GEMM_RING32_STAGE_HOOK(t)
    const char* bw = smem + (t % kNW) * kWBytes;
    const char* ba = smem + (t % kNA) * kABytes;
    // A fragments for the whole stage, W fragments two n-tiles at a time with the next pair's reads
    // issued ahead of the current pair's MFMAs (sched_barrier pins the pairs: hoisting all 12 W
    // reads would need 48 more registers than the 256 two waves per SIMD allow)
    bf16x8 af[MT], w0, w1, x0, x1;
#pragma unroll
    for (int i = 0; i < MT; ++i) af[i] = *(const bf16x8*)(ba + aoff + i * 16 * kRowBytes);
    w0 = *(const bf16x8*)(bw + woff);
    w1 = *(const bf16x8*)(bw + woff + 16 * kRowBytes);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int jp = 0; jp < kNT / 2; ++jp) {
#pragma unroll
      for (int u = 2 * jp; u < 2 * jp + 2; ++u)
        if (u < kOps) issue_op(t, u);
      if (jp + 1 < kNT / 2) {
        x0 = *(const bf16x8*)(bw + woff + (2 * (jp + 1)) * 16 * kRowBytes);
        x1 = *(const bf16x8*)(bw + woff + (2 * (jp + 1) + 1) * 16 * kRowBytes);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        acc[i][2 * jp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, af[i], acc[i][2 * jp], 0, 0, 0);
        acc[i][2 * jp + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, af[i], acc[i][2 * jp + 1], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      w0 = x0;
      w1 = x1;
    }
    __builtin_amdgcn_s_setprio(0);
  }
