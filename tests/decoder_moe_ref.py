"""Shared by test_decoder_moe_cpu.py and test_decoder_moe_gpu.py: synthetic mixture-of-experts GGUFs (qwen3moe,
and mixtral-style: architecture "llama" with stacked *_exps tensors) and the fp64 torch reference of what such a
file computes, in the file's own conventions (decoder_arch_ref's: unpermuted rows, the file's rotation).  The
reference can be FORCED to a routing chosen elsewhere ([layers][n, k] expert ids): it then weights the forced
set with its own softmax probabilities, and still returns its own router logits, so a caller can count the
decisions where its free choice would have differed.  Routing: the k largest router logits, ties to the lower
index -- softmax is monotone, so that is the order of the probabilities -- weighted by softmax over the k
chosen logits, which is the full softmax renormalised over the chosen (the denominator cancels)."""
import numpy as np
import torch

import decoder_arch_ref as R


def spec(arch="qwen3moe", E=8, k=2, F=64, d=128, H=2, KVH=1, hd=64, layers=2, seed=0, **kw):
    """arch "qwen3moe": q/k norms, key_length; "llama": mixtral.  The dense width `ffn` written as
    feed_forward_length is F for mixtral (its files have only that key) and unused for qwen3moe."""
    norm = arch == "qwen3moe"
    sp = R.spec(arch, d=d, H=H, KVH=KVH, hd=hd if norm else None, ffn=F, layers=layers, norm=norm,
                rope_base=1e6 if norm else 10000.0, seed=seed, **kw)
    sp.update(E=E, k=k, F=F)
    return sp


def weights(sp):
    """decoder_arch_ref.weights with the dense feed-forward tensors replaced by router [E, d], gate / up
    [E, F, d] and down [E, d, F], drawn after everything else (the attention weights are the dense twin's)."""
    w = R.weights(sp)
    rng = np.random.default_rng(sp["seed"] + 1000)
    E, F, d = sp["E"], sp["F"], sp["d"]
    f = lambda *s: (rng.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)  # noqa: E731
    for i in range(sp["layers"]):
        p = f"blk.{i}."
        for n in ("ffn_gate.weight", "ffn_up.weight", "ffn_down.weight"):
            del w[p + n]
        # router rows of norm ~ 2: logits of order 2, so that the top-k gaps are well above bf16 noise mostly
        w[p + "ffn_gate_inp.weight"] = 2.0 * f(E, d)
        w[p + "ffn_gate_exps.weight"] = f(E, F, d)
        w[p + "ffn_up_exps.weight"] = f(E, F, d)
        w[p + "ffn_down_exps.weight"] = f(E, d, F)
    return w


def moe_keys(sp, used_key=True, expert_ffn_key=None):
    """The file's expert metadata; expert_ffn_key None: written for qwen3moe only (as the real files do)."""
    a = sp["arch"]
    kv = {f"{a}.expert_count": sp["E"]}
    if used_key:
        kv[f"{a}.expert_used_count"] = sp["k"]
    if expert_ffn_key if expert_ffn_key is not None else a == "qwen3moe":
        kv[f"{a}.expert_feed_forward_length"] = sp["F"]
    return kv


def write_gguf(path, sp, w, extra=None, **kw):
    return R.write_gguf(path, sp, w, extra={**moe_keys(sp), **(extra or {})}, **kw)


def route(logits, k):
    """[n, E] -> ids [n, k]: the k largest, best first, ties to the lower index."""
    return torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k]


def ref_logits(sp, w, ids, forced=None, tw=None):
    """fp64: (logits [n, vocab], per-layer router logits [n, E], per-layer ids used [n, k])."""
    t = tw or {n: torch.from_numpy(a).double() for n, a in w.items()}
    H, KVH, hd, eps, k = sp["H"], sp["KVH"], sp["hd"], sp["eps"], sp["k"]
    n = len(ids)
    pos = torch.arange(n)
    x = t["token_embd.weight"][torch.tensor(ids)]
    causal = torch.ones((n, n), dtype=torch.bool).tril()
    rl, used = [], []
    rsp = dict(sp, arch="qwen3") if sp["arch"] == "qwen3moe" else sp  # qwen3moe rotates as qwen3 does (NeoX)
    for i in range(sp["layers"]):
        p = f"blk.{i}."
        h = R._rms(x, t[p + "attn_norm.weight"], eps)
        q, kk, v = (h @ t[p + f"attn_{c}.weight"].T for c in "qkv")
        q, kk, v = q.view(n, H, hd), kk.view(n, KVH, hd), v.view(n, KVH, hd)
        if sp["norm"]:
            q, kk = R._rms(q, t[p + "attn_q_norm.weight"], eps), R._rms(kk, t[p + "attn_k_norm.weight"], eps)
        q, kk = R.rotate(q, pos, rsp, w), R.rotate(kk, pos, rsp, w)
        kk, v = kk.repeat_interleave(H // KVH, 1), v.repeat_interleave(H // KVH, 1)
        sc = torch.einsum("qhd,khd->hqk", q, kk) * hd ** -0.5
        pr = torch.softmax(sc.masked_fill(~causal, -float("inf")), -1)
        x = x + torch.einsum("hqk,khd->qhd", pr, v).reshape(n, H * hd) @ t[p + "attn_output.weight"].T
        h = R._rms(x, t[p + "ffn_norm.weight"], eps)
        logits = h @ t[p + "ffn_gate_inp.weight"].T
        sel = route(logits, k) if forced is None else torch.as_tensor(forced[i]).long().reshape(n, k)
        wt = torch.softmax(logits.gather(1, sel), -1)
        rl.append(logits)
        used.append(sel)
        G, U, D = (t[p + f"ffn_{c}_exps.weight"] for c in ("gate", "up", "down"))
        y = torch.zeros_like(x)
        for j in range(k):
            e = sel[:, j]
            g = torch.einsum("nd,nfd->nf", h, G[e])
            u = torch.einsum("nd,nfd->nf", h, U[e])
            y = y + wt[:, j, None] * torch.einsum("nf,ndf->nd", torch.nn.functional.silu(g) * u, D[e])
        x = x + y
    head = t.get("output.weight", t["token_embd.weight"])
    return R._rms(x, t["output_norm.weight"], eps) @ head.T, rl, used


def dense_twin(sp):
    """The dense llama twin of an expert spec: same d, heads and seed (so the same attention weights),
    ffn = k * F."""
    return R.spec("llama", d=sp["d"], H=sp["H"], KVH=sp["KVH"], hd=sp["hd"] if sp["key_length"] else None,
                  ffn=sp["k"] * sp["F"], layers=sp["layers"], vocab=sp["vocab"], n_ctx=sp["n_ctx"], seed=sp["seed"])
