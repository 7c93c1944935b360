"""Per-token decode latency of the splainference decoder.

Default: dec_attn_decode vs torch SDPA (A/B) on the eager forward.  Random-init 7B-shaped layers are too big
for a quick A/B, so this uses the default DecoderConfig with --layers layers, prefills --prefill tokens, then
times --steps single-token decode steps.

--engine: ms/token of DecodeEngine steps (the captured decode step; --no-graph: eager launches) for one
architecture, --arch llama | qwen2 | qwen3: qwen2 adds the q/k/v biases, qwen3 the per-head q/k norms, so the
step runs dec_qk_prep_kv where the llama step runs dec_rope_kv.  --d / --heads / --kv-heads / --head-dim /
--ffn set the layer shape, --quant the weights; --repeats timed blocks of --steps tokens give the spread.

--experts E --experts-used K --expert-ffn F make every layer a mixture of experts (--arch qwen3moe, or llama for
the mixtral form): the step then runs the router GEMV, dec_moe_route, dec_gemv_moe* and dec_gemv_moe_down*.  The
expert tensors are drawn on the device one at a time, so a Mixtral-sized layer needs no host copy.
--prefill-ms times the eager prompt prefill alone (CausalLM.forward on --prefill tokens, --repeats runs)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from libsplinter_amd.models.decoder import (CausalLM, DecodeEngine, DecoderConfig, LazyTensors,
                                            random_decoder_weights)

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--prefill", type=int, default=1024)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--kv-heads", type=int, default=8)
ap.add_argument("--arch", default="llama", choices=["llama", "qwen2", "qwen3", "qwen3moe"])
ap.add_argument("--experts", type=int, default=0)
ap.add_argument("--experts-used", type=int, default=0)
ap.add_argument("--expert-ffn", type=int, default=0)
ap.add_argument("--prefill-ms", action="store_true")
ap.add_argument("--engine", action="store_true")
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--quant", default="bf16", choices=["bf16", "q4"])
ap.add_argument("--d", type=int, default=512)
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--head-dim", type=int, default=0, help="0: d / heads")
ap.add_argument("--ffn", type=int, default=1536)
ap.add_argument("--repeats", type=int, default=1)
a = ap.parse_args()
cfg = DecoderConfig(layers=a.layers, kv_heads=a.kv_heads, d=a.d, heads=a.heads, ffn=a.ffn, arch=a.arch,
                    qkv_bias=a.arch == "qwen2", qk_norm=a.arch in ("qwen3", "qwen3moe"),
                    experts=a.experts, experts_used=a.experts_used, expert_ffn=a.expert_ffn,
                    key_length=a.head_dim if a.head_dim and a.head_dim * a.heads != a.d else None,
                    n_ctx=a.prefill + (a.steps * max(1, a.repeats) + 16 if a.engine else a.steps + 8))
if a.experts:
    # everything but the experts as CausalLM.random draws it; the experts on the device, at the same scale
    from dataclasses import replace
    host = {k: torch.from_numpy(v) for k, v in random_decoder_weights(replace(cfg, experts=0), 0).items()}
    E, F = cfg.experts, cfg.expert_ffn
    shapes = {"ffn_gate_inp": (E, cfg.d), "ffn_gate_exps": (E, F, cfg.d), "ffn_up_exps": (E, F, cfg.d),
              "ffn_down_exps": (E, cfg.d, F)}
    names = [n for n in host if ".ffn_gate." not in n and ".ffn_up." not in n and ".ffn_down." not in n]
    names += [f"blk.{i}.{n}.weight" for i in range(cfg.layers) for n in shapes]
    gen = torch.Generator(device="cuda").manual_seed(0)

    def load(n):
        if n in host:
            return host[n]
        return torch.randn(shapes[n.split(".")[2]], device="cuda", dtype=torch.bfloat16, generator=gen) * 0.02

    m = CausalLM(cfg, LazyTensors(names, load), "cuda", quant=a.quant)
else:
    m = CausalLM.random(cfg, seed=0, device="cuda", quant=a.quant)
shape = {"arch": a.arch, "quant": a.quant, "layers": a.layers, "ctx": a.prefill, "d": cfg.d, "heads": cfg.heads,
         "kv_heads": a.kv_heads, "head_dim": cfg.head_dim, "ffn": cfg.ffn}
if a.experts:
    shape.update(experts=a.experts, experts_used=a.experts_used, expert_ffn=a.expert_ffn)
    del shape["ffn"]
if a.prefill_ms:
    ms = []
    for _ in range(1 + max(1, a.repeats)):  # the first run loads code objects and sizes the scratch: not kept
        m.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.forward([1 + i % 200 for i in range(a.prefill)])
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    print(json.dumps({"prefill_ms": ms[1:], "tokens": a.prefill, **shape}))
    sys.exit(0)
if a.engine:
    eng = DecodeEngine(m, use_graph=not a.no_graph)
    eng.first_token([1] * a.prefill)
    for _ in range(8):
        eng.next_token()
    ms = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.next_token()
        ms.append(round((time.perf_counter() - t0) / a.steps * 1e3, 5))
    print(json.dumps({"engine_ms_per_token": ms, "graph": not a.no_graph, "steps": a.steps, **shape}))
    sys.exit(0)
res = {}
for mode in (False, True, False, True):
    m.attn_kernel = mode
    m.reset()
    m.forward([1] * a.prefill)
    for _ in range(4):
        m.forward([65])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        m.forward([65])
    torch.cuda.synchronize()
    res["kernel" if mode else "sdpa"] = (time.perf_counter() - t0) / a.steps * 1e3
print(json.dumps({"ms_per_token": res, "layers": a.layers, "ctx": a.prefill, "d": cfg.d, "heads": cfg.heads,
                  "kv_heads": a.kv_heads}))
