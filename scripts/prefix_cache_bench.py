"""Shared prompt prefix reuse of BatchDecodeEngine (set_prefix) against the same engine with no prefix set, bf16
and 4-bit weights.

Llama-7B-shaped layers (d 4096, 32 heads, 8 kv heads, ffn 11008, vocab 32000) with --layers layers, random
init (one set of weights for both formats), one engine of 16 slots per weight format.  16 requests of one
shared --prefix token head plus --tail tokens of their own are submitted together and prefilled with --chunk
until nothing is pending; the time runs from the first submit to the last first token (every pass ends
synchronised).  The configurations alternate over --rounds rounds after one discarded warm-up round.  Prints
one JSON line per measurement:

  plain    no prefix set: every request prefills its whole prompt
  cold     set_prefix just before the wave: one request computes the head while the others wait, then all 16
           prefill their tails from copied rows
  warm     the same prefix already captured by an earlier wave: 16 hits in the first pass
  fanout   dec_kv_rows_fanout alone (events around the launch): the captured head restored to 15 slots"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from libsplinter_amd.models.decoder import (BatchDecodeEngine, CausalLM, DecoderConfig,  # noqa: E402
                                            random_decoder_weights)

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--quants", default="bf16,q4")
ap.add_argument("--prefix", type=int, default=1024)
ap.add_argument("--tail", type=int, default=64)
ap.add_argument("--chunk", type=int, default=256)
a = ap.parse_args()
S = 16
cfg = DecoderConfig(vocab=32000, d=4096, layers=a.layers, heads=32, kv_heads=8, ffn=11008, n_ctx=2048)
head = [1] + [100 + (7 * i) % 200 for i in range(a.prefix - 1)]
reqs = [head + [300 + (i * (k + 1)) % 200 for i in range(a.tail)] for k in range(S)]
sync = torch.cuda.synchronize


def wave(eng):
    """(ms from the first submit to the last first token, passes, packed rows, hits) of the 16 requests"""
    for b in eng.active() + eng.pending():
        eng.release(b)
    sync()
    p0, r0, h0 = eng.prefill_passes, eng.prefill_rows, eng.prefix_hits
    t0 = time.perf_counter()
    for k, ids in enumerate(reqs):
        eng.submit(ids, seed=k)
    while eng.pending():
        eng.prefill(a.chunk)
    sync()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, eng.prefill_passes - p0, eng.prefill_rows - r0, eng.prefix_hits - h0


def fanout_ms(eng, reps=20):
    """the restore launch alone: the captured head to slots 1..15 (slot 0's rows are the same bits)"""
    for b in eng.active() + eng.pending():
        eng.release(b)
    R = len(eng._pfx_ids)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        eng._fanout(eng._pfx_buf, R, eng.kv, cfg.n_ctx, eng.kv.stride(0), list(range(1, S)), S, R)
        e1.record()
    sync()
    return sorted(e0.elapsed_time(e1) for e0, e1 in ev)[reps // 2], R


t0 = time.time()
weights = {k: torch.from_numpy(v) for k, v in random_decoder_weights(cfg, 0).items()}
print(f"[prefix_cache_bench] weights drawn in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
for q in a.quants.split(","):
    t0 = time.time()
    m = CausalLM(cfg, weights, "cuda", quant=q)
    eng = BatchDecodeEngine(m, max_seqs=S, seed=7, use_graph=True)
    print(f"[prefix_cache_bench] {q} model and engine built in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    res = {}
    for r in range(a.rounds + 1):
        rec = lambda k, v: res.setdefault(k, []).append(v) if r else None  # noqa: E731  (round 0 warms up)
        eng.set_prefix(None, 0)
        rec("plain", wave(eng))
        eng.set_prefix(head, a.chunk)
        rec("cold", wave(eng))
        rec("warm", wave(eng))
    fan, R = fanout_ms(eng)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    common = {"quant": q, "layers": a.layers, "d": cfg.d, "ffn": cfg.ffn, "vocab": cfg.vocab, "slots": S,
              "prefix": a.prefix, "tail": a.tail, "chunk": a.chunk}
    for k, v in res.items():
        print(json.dumps({**common, "what": k, "ms_median": med([x[0] for x in v]), "ms_all": [x[0] for x in v],
                          "passes": v[0][1], "prefill_rows": v[0][2], "prefix_hits": v[0][3]}), flush=True)
    kvd = cfg.kv_heads * cfg.head_dim
    print(json.dumps({**common, "what": "fanout", "rows": R, "destinations": S - 1, "ms_median": fan,
                      "mib_read": cfg.layers * 2 * R * kvd * 2 / 2 ** 20,
                      "mib_written": (S - 1) * cfg.layers * 2 * R * kvd * 2 / 2 ** 20}), flush=True)
    del eng, m
    torch.cuda.empty_cache()
