"""Batched, chunked prompt prefill of BatchDecodeEngine (submit + prefill) against the eager admit, bf16 and
4-bit weights.

Llama-7B-shaped layers (d 4096, 32 heads, 8 kv heads, ffn 11008, vocab 32000) with --layers layers, random
init, one engine of 16 slots per weight format, everything in one process with the configurations alternated
over --rounds rounds after one discarded warm-up round (graph capture, first launches, workspaces).  Prints
one JSON line per measurement:

  admission  time to make 16 prompts of --admit-lens tokens live: 16 eager admits against 16 submits plus
             prefill(chunk = the prompt length) until nothing is pending
  stall      8 live streams step while one --long token prompt arrives: the longest gap between two
             consecutive steps of the live streams and the newcomer's time to its first token, eager admit
             against --chunks (one prefill pass between two steps)
  decode     ms per decode step of the 8 live streams with nothing pending, before and after the prefill
             passes of the round (the step's kernels are the same: it must not move)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from libsplinter_amd.models.decoder import BatchDecodeEngine, CausalLM, DecoderConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--quants", default="bf16,q4")
ap.add_argument("--admit-lens", default="64,512")
ap.add_argument("--long", type=int, default=3000)
ap.add_argument("--chunks", default="256,1024")
ap.add_argument("--live", type=int, default=8)
ap.add_argument("--live-prompt", type=int, default=128)
ap.add_argument("--steps", type=int, default=32)
a = ap.parse_args()
S = 16
lens = [int(x) for x in a.admit_lens.split(",")]
chunks = [int(x) for x in a.chunks.split(",")]
cfg = DecoderConfig(vocab=32000, d=4096, layers=a.layers, heads=32, kv_heads=8, ffn=11008, n_ctx=a.long + 200)
prompt = lambda n, k=0: [1] + [100 + (i * (k + 1)) % 200 for i in range(n - 1)]  # noqa: E731
sync = torch.cuda.synchronize


def clear(eng):
    for b in eng.active() + eng.pending():
        eng.release(b)


def timed_steps(eng, n):
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        eng.step()
    return (time.perf_counter() - t0) / n * 1e3


def admission(eng, n, batched):
    clear(eng)
    sync()
    t0 = time.perf_counter()
    if batched:
        for k in range(S):
            eng.submit(prompt(n, k), seed=k)
        while eng.pending():
            eng.prefill(n)
    else:
        for k in range(S):
            eng.admit(prompt(n, k), seed=k)
    sync()
    return (time.perf_counter() - t0) * 1e3


def stall(eng, chunk):
    """(longest gap between two steps of the live streams, newcomer's time to first token, steps it took), ms"""
    clear(eng)
    for k in range(a.live):
        eng.admit(prompt(a.live_prompt, k), seed=k)
    for _ in range(4):
        eng.step()
    sync()
    marks = [time.perf_counter()]
    for _ in range(4):
        eng.step()
        marks.append(time.perf_counter())
    t_arrive = time.perf_counter()
    long_ids = prompt(a.long, 99)
    ttft = None
    if chunk == 0:
        eng.admit(long_ids, seed=99)
        ttft = time.perf_counter() - t_arrive
    else:
        eng.submit(long_ids, seed=99)
    while ttft is None:
        if eng.prefill(chunk):
            ttft = time.perf_counter() - t_arrive
        eng.step()
        marks.append(time.perf_counter())
    for _ in range(4):
        eng.step()
        marks.append(time.perf_counter())
    gaps = [(y - x) * 1e3 for x, y in zip(marks, marks[1:])]
    return max(gaps), ttft * 1e3, len(marks) - 9


def decode_cost(eng):
    clear(eng)
    for k in range(a.live):
        eng.admit(prompt(a.live_prompt, k), seed=k)
    for _ in range(4):
        eng.step()
    return timed_steps(eng, a.steps)


for q in a.quants.split(","):
    t0 = time.time()
    m = CausalLM.random(cfg, seed=0, device="cuda", quant=q)
    eng = BatchDecodeEngine(m, max_seqs=S, seed=7, use_graph=True)
    print(f"[prefill_batch_bench] {q} model and engine built in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    res = {}
    for r in range(a.rounds + 1):
        rec = lambda k, v: res.setdefault(k, []).append(v) if r else None  # noqa: E731  (round 0 warms up)
        rec(("decode", "before"), decode_cost(eng))
        for n in lens:
            rec(("admission", n, "eager"), admission(eng, n, False))
            rec(("admission", n, "batched"), admission(eng, n, True))
        for c in [0] + chunks:
            rec(("stall", c), stall(eng, c))
        rec(("decode", "after"), decode_cost(eng))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    common = {"quant": q, "layers": a.layers, "d": cfg.d, "ffn": cfg.ffn, "vocab": cfg.vocab, "slots": S}
    for k, v in res.items():
        if k[0] == "decode":
            print(json.dumps({**common, "what": "decode", "when": k[1], "live": a.live, "ms_per_step_median": med(v),
                              "ms_per_step_all": v}), flush=True)
        elif k[0] == "admission":
            print(json.dumps({**common, "what": "admission", "prompts": S, "tokens_each": k[1], "path": k[2],
                              "ms_median": med(v), "ms_all": v}), flush=True)
        else:
            print(json.dumps({**common, "what": "stall", "live": a.live, "long_prompt": a.long,
                              "path": "eager admit" if k[1] == 0 else f"prefill chunk {k[1]}",
                              "max_gap_ms_median": med([x[0] for x in v]), "max_gap_ms_all": [x[0] for x in v],
                              "ttft_ms_median": med([x[1] for x in v]), "ttft_ms_all": [x[1] for x in v],
                              "steps_until_live": v[0][2]}), flush=True)
    del eng, m
    torch.cuda.empty_cache()
