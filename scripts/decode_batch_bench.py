"""Decode throughput of BatchDecodeEngine against the single-sequence DecodeEngine, bf16 and 4-bit weights.

Llama-7B-shaped layers (d 4096, 32 heads, 8 kv heads, ffn 11008, vocab 32000) with --layers layers, random
init, a --prompt token prompt in every slot.  For S in --seqs live sequences one step is one replay of the
batched HIP graph (S tokens); the comparison point is the single-sequence DecodeEngine of the same model,
timed in the same process with the configurations alternated over --rounds rounds.  Prints one JSON line
per configuration: ms per step (median and every round), aggregate tokens/s, the ratio to the
single-sequence rate, and the projection bytes streamed per step over the step time.  S = 1 runs an engine
of two slots with one live (the engine takes 2..16 slots)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from libsplinter_amd.models.decoder import (BatchDecodeEngine, CausalLM, DecodeEngine, DecoderConfig,  # noqa: E402
                                            Q4Weight)

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--prompt", type=int, default=128)
ap.add_argument("--tokens", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--seqs", default="1,2,4,8,16")
ap.add_argument("--quants", default="bf16,q4")
a = ap.parse_args()
seqs = [int(s) for s in a.seqs.split(",")]
cfg = DecoderConfig(vocab=32000, d=4096, layers=a.layers, heads=32, kv_heads=8, ffn=11008,
                    n_ctx=a.prompt + a.tokens + 24)


def weight_bytes(m):
    ws = [m.head] + [lw[k] for lw in m.layers for k in ("qkv", "o", "ug", "down")]
    return sum(w.nbytes() if isinstance(w, Q4Weight) else w.numel() * w.element_size() for w in ws)


prompt = [1] + [100 + i % 200 for i in range(a.prompt - 1)]
for q in a.quants.split(","):
    t0 = time.time()
    m = CausalLM.random(cfg, seed=0, device="cuda", quant=q)
    nb = weight_bytes(m)
    single = DecodeEngine(m, seed=7, use_graph=True)
    batched = {S: BatchDecodeEngine(m, max_seqs=max(S, 2), seed=7, use_graph=True) for S in seqs}
    print(f"[decode_batch_bench] {q} model and engines built in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    res = {k: [] for k in ["single"] + seqs}
    for r in range(a.rounds):
        single.first_token(prompt)
        for _ in range(4):
            single.next_token()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.tokens):
            single.next_token()
        res["single"].append((time.perf_counter() - t0) / a.tokens * 1e3)
        for S in seqs:
            eng = batched[S]
            for b in eng.active():
                eng.release(b)
            for b in range(S):
                eng.admit(prompt, seed=7 + b)
            for _ in range(4):
                eng.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.tokens):
                eng.step()
            res[S].append((time.perf_counter() - t0) / a.tokens * 1e3)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    ms1 = med(res["single"])
    common = {"quant": q, "layers": a.layers, "d": cfg.d, "ffn": cfg.ffn, "vocab": cfg.vocab, "ctx": a.prompt,
              "weight_GB": nb / 1e9}
    print(json.dumps({**common, "engine": "DecodeEngine", "seqs": 1, "ms_per_step_median": ms1,
                      "ms_per_step_all": res["single"], "tokens_per_s": 1e3 / ms1,
                      "weight_TB_per_s": nb / (ms1 * 1e-3) / 1e12}), flush=True)
    for S in seqs:
        ms = med(res[S])
        print(json.dumps({**common, "engine": "BatchDecodeEngine", "seqs": S, "max_seqs": max(S, 2),
                          "ms_per_step_median": ms, "ms_per_step_all": res[S], "tokens_per_s": S * 1e3 / ms,
                          "tokens_per_s_over_single": S * ms1 / ms, "step_over_single_token": ms / ms1,
                          "weight_TB_per_s": nb / (ms * 1e-3) / 1e12}), flush=True)
    del single, batched, m
    torch.cuda.empty_cache()
