"""The encoder GEMM kernels on one shape, interleaved rounds in one process on random data.  Forms:

  256s0 / 256s1   256^2 kernel, tail split off / on (nomic_gemm_set_tail_split)
  128             128^2 kernel
  384             256x384 register-epilogue kernel (gemm384.hip), stage width as the process has it
  384k32 / 384k64 the same with 32- / 64-wide K stages (nomic_gemm384_set_bk)

Default shape: the encoder's qkv projection with the RoPE epilogue (32768 x 2304 x 768).  The n-band
of the tile order is a process-level knob: run once per NOMIC_GEMM_GN value for a band sweep.

One JSON line per form: median / min microseconds, TFLOP/s, and whether the form wrote the same bits
as the first one.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (NOMIC_GEMM, tail split, K per stage of the 256x384 kernel or 0 to leave it)
FORMS = {"256s0": (256, 0, 0), "256s1": (256, 1, 0), "128": (128, 1, 0), "384": (384, 1, 0), "384k32": (384, 1, 32),
         "384k64": (384, 1, 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--n", type=int, default=2304)
    ap.add_argument("--k", type=int, default=768)
    ap.add_argument("--mode", type=int, default=3, help="0 store, 2 SwiGLU, 3 RoPE (nomic_api.h NOMIC_EPI_*)")
    ap.add_argument("--forms", default="256s0,256s1,384", help="comma list of " + " ".join(FORMS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    from libsplinter_amd.models.nomic import _chk, _lib, _stream
    L = _lib()
    M, N, K = a.tokens, a.n, a.k
    forms = a.forms.split(",")
    torch.manual_seed(0)
    x = torch.randn(M, K, device="cuda").bfloat16()
    w = (torch.randn(N, K, device="cuda") * 0.03).bfloat16()
    ocols = N // 2 if a.mode == 2 else N
    outs = {f: torch.empty(M, ocols, device="cuda", dtype=torch.bfloat16) for f in forms}
    pos = (torch.arange(M, device="cuda", dtype=torch.int32) % 512).contiguous()
    ang = np.arange(8192)[:, None] * (1000.0 ** (-np.arange(0, 64, 2) / 64))[None, :]
    tab = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32).reshape(8192, -1)).cuda()

    def run(f):
        variant, split, bk = FORMS[f]
        L.nomic_gemm_set_variant(variant)
        L.nomic_gemm_set_tail_split(split)
        if bk:
            L.nomic_gemm384_set_bk(bk)
        _chk(L.nomic_gemm(a.mode, x.data_ptr(), K, w.data_ptr(), K, M, N, K, outs[f].data_ptr(), ocols, None, 0,
                          tab.data_ptr(), pos.data_ptr(), N * 2 // 3 if a.mode == 3 else 0, _stream()), "gemm")

    for f in forms:
        run(f)
    torch.cuda.synchronize()
    same = {f: bool(torch.equal(outs[f], outs[forms[0]])) for f in forms}
    maxdiff = {f: float((outs[f].float() - outs[forms[0]].float()).abs().max()) for f in forms}
    times = {f: [] for f in forms}
    for _ in range(a.rounds):
        for f in forms:
            run(f)
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            for _ in range(a.iters):
                run(f)
            e.record()
            torch.cuda.synchronize()
            times[f].append(b.elapsed_time(e) / a.iters * 1e3)
    for f in forms:
        t = np.array(times[f])
        L.nomic_gemm_set_tail_split(FORMS[f][1])
        print(json.dumps({"shape": [M, N, K], "mode": a.mode, "form": f, "gn": os.environ.get("NOMIC_GEMM_GN", "auto"),
                          "blocks256": L.nomic_gemm256_grid(M, N) if f.startswith("256") else None,
                          "us_median": round(float(np.median(t)), 2), "us_min": round(float(t.min()), 2),
                          "tflops": round(2.0 * M * N * K / np.median(t) / 1e6, 1), "same_bits": same[f],
                          "max_abs_diff": maxdiff[f]}), flush=True)


if __name__ == "__main__":
    main()
