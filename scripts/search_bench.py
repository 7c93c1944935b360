"""Vector search benchmark (BASELINE config #5, one GPU's shard): QPS and recall of the
batched MFMA search against the exact fp32 kernel on an arena of N embedded slots.

python scripts/search_bench.py [--slots 25000000] [--nq 512] [--k 10] [--iters 3]
                               [--data clustered|iid] [--copy auto|bf16|int8|both]
Synthetic 768-d vectors (random, not a real corpus): clustered (4096 centres, sigma 0.5) or i.i.d.
normal.  Prints one JSON line per arm: `--copy both` on an arena created under SPLINTER_HBM_VEC8=1
times the bf16 and the int8 candidate copy on the same vectors in one process; per arm the QPS,
the time of one candidate pass alone, the candidates per query, the overflow count and recall@k /
identity of the top-k against the exact kernel.
200M x 768 across 8 GPUs = 25M slots per GPU (80 GB of 3200-B slots in HBM).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _pass_ms(vs, ar, q, copy, iters):
    """One candidate (emit) pass over the whole arena for the first 256 queries, alone: thresholds
    from the arm's own sample pass, best of `iters` by device events."""
    import torch
    from libsplinter_amd.ops.search import DELTA, MMA_GRID, MMA_Q, TILE
    qq = q[:MMA_Q].contiguous()
    n, slots = qq.shape[0], ar.slots
    sample = max(TILE, min(slots, max(TILE * 4096, slots // 16)) // TILE * TILE)
    bmax = torch.empty(sample // TILE, n, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(n, MMA_GRID, dtype=torch.int32, device="cuda")
    cand = torch.empty(n * MMA_GRID * 64, dtype=torch.int32, device="cuda")
    kind = "int8" if copy == "int8" else "bf16"
    qop = vs.qprep8(qq) if kind == "int8" else (vs.qprep16(qq),)
    vs.mma_pass(kind, qop, n, sample, 0, bmax=bmax)
    thr = (bmax.topk(10, dim=0).values[-1] - (0.0 if kind == "int8" else 2 * DELTA)).contiguous()
    best = 1e9
    for _ in range(iters + 1):
        cnt.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        vs.mma_pass(kind, qop, n, slots, 1, thr=thr, cnt=cnt, cand=cand, capb=64)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=25_000_000)
    ap.add_argument("--nq", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--recall-queries", type=int, default=32)
    ap.add_argument("--exact", action="store_true", help="also time the exact fp32 kernel on all queries")
    ap.add_argument("--data", default="clustered", choices=["clustered", "iid"])
    ap.add_argument("--copy", default="auto", choices=["auto", "bf16", "int8", "both"],
                    help="candidate copy per arm (int8 / both need an arena created under SPLINTER_HBM_VEC8=1)")
    ap.add_argument("--capb", type=int, default=64,
                    help="candidates kept per (block, query) segment; the product path (spl_search_batch) uses 64")
    a = ap.parse_args()
    import torch
    from libsplinter_amd.ops.arena import HbmArena, format_keys, format_values
    from libsplinter_amd.ops.search import VectorSearch
    name = f"sbench{os.getpid()}"
    ar = HbmArena.create(name, slots=a.slots, max_val=16, embeddings=True)
    try:
        n = int(a.slots * 0.9)
        t0 = time.time()
        g = torch.Generator(device="cuda").manual_seed(0)
        centers = torch.randn(4096, 768, device="cuda", generator=g)

        def draw(m):
            if a.data == "iid":
                return torch.randn(m, 768, device="cuda", generator=g)
            lab = torch.randint(0, 4096, (m,), device="cuda", generator=g)
            return centers[lab] + 0.5 * torch.randn(m, 768, device="cuda", generator=g)

        em = ar.embedding_matrix()
        step = 2_000_000
        for b in range(0, n, step):
            m = min(step, n - b)
            keys = format_keys(m, "s", 12, 16, first=b)
            vals, lens = format_values(m, 1, 8, 16, first=b)
            st = ar.set(keys, vals, lens)
            assert int((st == 0).sum()) == m
            del keys, vals, lens, st
        # vectors straight into the slot embedding fields (occupied or not: the kernels skip free slots)
        for b in range(0, a.slots, step):
            m = min(step, a.slots - b)
            em[b: b + m] = draw(m)
        ar.rebuild_vec16()  # raw writes through the view: the copies the search streams, recomputed
        torch.cuda.synchronize()
        fill_s = time.time() - t0
        vs = VectorSearch(ar, grid=1024)
        q = draw(a.nq)
        rq = min(a.recall_queries, a.nq)
        t = time.perf_counter()
        ei, es, _ = vs.search(q[:rq], k=a.k)
        torch.cuda.synchronize()
        exact_s = time.perf_counter() - t
        arms = ["bf16", "int8"] if a.copy == "both" else [a.copy]
        for copy in arms:
            st = {}
            vs.search_batch(q, k=a.k, stats=st, copy=copy, capb=a.capb)  # warmup
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.iters):
                t = time.perf_counter()
                idx, sim, _ = vs.search_batch(q, k=a.k, stats=st, copy=copy, capb=a.capb)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t)
            best = min(ts)
            hit = 0
            for j in range(rq):
                hit += len(set(idx[j].tolist()) & set(ei[j].tolist()))
            used = st["copy"]
            row_bytes = {"int8": 768, "bf16": 1536, "fp32": 3200}[used]
            out = {"bench": "vector_search", "arm": used, "slots": a.slots, "embedded": a.slots, "occupied": n,
                   "nq": a.nq, "k": a.k, "capb": a.capb, "qps": a.nq / best, "ms_per_batch": best * 1e3,
                   "ms_per_candidate_pass": _pass_ms(vs, ar, q, used, a.iters),
                   "recall_at_k": hit / (rq * a.k), "exact_match": bool(torch.equal(idx[:rq], ei)),
                   "sims_identical": bool(torch.equal(sim[:rq], es)),
                   "candidates_per_query": st["candidates"] / a.nq, "overflow_queries": st["overflow"],
                   "exact_kernel_qps": rq / exact_s,
                   "scan_GBps": a.slots * row_bytes / best / 1e9 * ((a.nq + 255) // 256),
                   "candidate_rows": {"int8": "int8 copy (side region)", "bf16": "bf16 copy (side region)",
                                      "fp32": "fp32 slot rows"}[used],
                   "fill_s": round(fill_s, 1),
                   "data": ("synthetic clustered (4096 centres, sigma 0.5)" if a.data == "clustered"
                            else "synthetic i.i.d. normal") + ", fp32 768-d in slots"}
            print(json.dumps(out), flush=True)
    finally:
        ar.close()


if __name__ == "__main__":
    main()
