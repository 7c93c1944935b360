"""256^2 GEMM with the tail split on and off (nomic_gemm_set_tail_split), interleaved rounds in one
process on random data.  Default shape: the encoder's qkv projection with the RoPE epilogue
(32768 x 2304 x 768: 1152 tiles, 4.5 rounds on 256 CUs).

One JSON line per arm: median / min microseconds, TFLOP/s, the launch's workgroup count, and whether
the two arms wrote the same bits.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--n", type=int, default=2304)
    ap.add_argument("--k", type=int, default=768)
    ap.add_argument("--mode", type=int, default=3, help="0 store, 2 SwiGLU, 3 RoPE (nomic_api.h NOMIC_EPI_*)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    from libsplinter_amd.models.nomic import _chk, _lib, _stream
    L = _lib()
    M, N, K = a.tokens, a.n, a.k
    torch.manual_seed(0)
    x = torch.randn(M, K, device="cuda").bfloat16()
    w = (torch.randn(N, K, device="cuda") * 0.03).bfloat16()
    ocols = N // 2 if a.mode == 2 else N
    outs = {s: torch.empty(M, ocols, device="cuda", dtype=torch.bfloat16) for s in (0, 1)}
    pos = (torch.arange(M, device="cuda", dtype=torch.int32) % 512).contiguous()
    ang = np.arange(8192)[:, None] * (1000.0 ** (-np.arange(0, 64, 2) / 64))[None, :]
    tab = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32).reshape(8192, -1)).cuda()
    L.nomic_gemm_set_variant(256)

    def run(split):
        L.nomic_gemm_set_tail_split(split)
        _chk(L.nomic_gemm(a.mode, x.data_ptr(), K, w.data_ptr(), K, M, N, K, outs[split].data_ptr(), ocols, None, 0,
                          tab.data_ptr(), pos.data_ptr(), N * 2 // 3 if a.mode == 3 else 0, _stream()), "gemm")

    grids = {}
    for s in (0, 1):
        run(s)
        grids[s] = L.nomic_gemm256_grid(M, N)
    torch.cuda.synchronize()
    same = bool(torch.equal(outs[0], outs[1]))
    times = {0: [], 1: []}
    for _ in range(a.rounds):
        for s in (0, 1):
            run(s)
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            for _ in range(a.iters):
                run(s)
            e.record()
            torch.cuda.synchronize()
            times[s].append(b.elapsed_time(e) / a.iters * 1e3)
    for s in (0, 1):
        t = np.array(times[s])
        print(json.dumps({"shape": [M, N, K], "mode": a.mode, "tail_split": s, "blocks": grids[s],
                          "us_median": round(float(np.median(t)), 2), "us_min": round(float(t.min()), 2),
                          "tflops": round(2.0 * M * N * K / np.median(t) / 1e6, 1), "same_bits": same}), flush=True)


if __name__ == "__main__":
    main()
