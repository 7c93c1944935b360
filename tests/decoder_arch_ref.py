"""Shared by test_decoder_arch_cpu.py and test_decoder_arch_gpu.py: synthetic GGUFs of the decoder
architectures (llama, qwen2, qwen3) built with GGUFWriter from seeded numpy weights, and the fp64 torch
reference of what such a file computes.  The reference works in the file's own convention -- unpermuted
rows, the NeoX half rotation for qwen2 / qwen3, adjacent pairs for llama -- so it shares nothing with the
loader's row permutation."""
import numpy as np
import torch

NEOX = ("qwen2", "qwen3")


def spec(arch="llama", d=128, H=2, KVH=1, hd=None, ffn=256, layers=2, vocab=384, n_ctx=64, bias=False, norm=False,
         tied=False, rope_base=10000.0, rope_freqs=False, scaling=None, eps=1e-6, seed=0):
    """hd None: d // H and no key_length in the file; scaling: None or (type, factor[, original context])."""
    return dict(arch=arch, d=d, H=H, KVH=KVH, hd=hd or d // H, key_length=hd is not None, ffn=ffn, layers=layers,
                vocab=vocab, n_ctx=n_ctx, bias=bias, norm=norm, tied=tied, rope_base=rope_base,
                rope_freqs=rope_freqs, scaling=scaling, eps=eps, seed=seed)


def weights(sp):
    """name -> float32 array, GGUF names and layouts.  Projections ~ N(0, 1/K) so that logits and attention
    scores are of order one; norm weights 1 + noise; biases ~ 0.5."""
    rng = np.random.default_rng(sp["seed"])
    d, H, KVH, hd, ffn = sp["d"], sp["H"], sp["KVH"], sp["hd"], sp["ffn"]
    f = lambda n, k: (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)  # noqa: E731
    nw = lambda n: (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)  # noqa: E731
    w = {"token_embd.weight": rng.standard_normal((sp["vocab"], d)).astype(np.float32),
         "output_norm.weight": nw(d)}
    if not sp["tied"]:
        w["output.weight"] = f(sp["vocab"], d)
    if sp["rope_freqs"]:
        w["rope_freqs.weight"] = np.linspace(1.0, 8.0, hd // 2).astype(np.float32)
    for i in range(sp["layers"]):
        p = f"blk.{i}."
        w[p + "attn_norm.weight"] = nw(d)
        w[p + "attn_q.weight"] = f(H * hd, d)
        w[p + "attn_k.weight"] = f(KVH * hd, d)
        w[p + "attn_v.weight"] = f(KVH * hd, d)
        w[p + "attn_output.weight"] = f(d, H * hd)
        w[p + "ffn_norm.weight"] = nw(d)
        w[p + "ffn_gate.weight"] = f(ffn, d)
        w[p + "ffn_up.weight"] = f(ffn, d)
        w[p + "ffn_down.weight"] = f(d, ffn)
    # drawn after the matrices: a llama twin of the same seed has the same projections
    for i in range(sp["layers"]):
        p = f"blk.{i}."
        if sp["bias"]:
            for n, rows in (("q", H * hd), ("k", KVH * hd), ("v", KVH * hd)):
                w[p + f"attn_{n}.bias"] = (0.5 * rng.standard_normal(rows)).astype(np.float32)
        if sp["norm"]:
            w[p + "attn_q_norm.weight"] = nw(hd)
            w[p + "attn_k_norm.weight"] = nw(hd)
    return w


def chatml_vocab(vocab):
    """A byte-level BPE vocabulary of `vocab` entries with the chatml control tokens, no merges."""
    from libsplinter_amd.models.llm_tokenizer import gpt2_byte_map
    m = gpt2_byte_map()
    toks = [m[b] for b in range(256)] + ["<|im_start|>", "<|im_end|>", "<|endoftext|>"]
    types = [1] * 256 + [3, 3, 3]
    while len(toks) < vocab:
        toks.append(f"<|pad{len(toks)}|>")
        types.append(3)
    return toks, types


def write_gguf(path, sp, w, arch_key=True, tokenizer=False, extra=None):
    """The file of spec `sp`.  arch_key False: no general.architecture (the keys stay under "llama.");
    extra: further {key: value} metadata, written as given."""
    from libsplinter_amd.models.gguf import GGUFWriter
    a = sp["arch"]
    gw = GGUFWriter(str(path), a)
    if not arch_key:
        gw.kv = [e for e in gw.kv if e[0] != "general.architecture"]
    for k, v in (("embedding_length", sp["d"]), ("block_count", sp["layers"]), ("attention.head_count", sp["H"]),
                 ("attention.head_count_kv", sp["KVH"]), ("feed_forward_length", sp["ffn"]),
                 ("context_length", sp["n_ctx"])):
        gw.add(f"{a}.{k}", v)
    gw.add(f"{a}.rope.freq_base", float(sp["rope_base"]))
    gw.add(f"{a}.attention.layer_norm_rms_epsilon", float(sp["eps"]))
    if sp["key_length"]:
        gw.add(f"{a}.attention.key_length", sp["hd"])
        gw.add(f"{a}.attention.value_length", sp["hd"])
    if sp["scaling"]:
        gw.add(f"{a}.rope.scaling.type", sp["scaling"][0])
        gw.add(f"{a}.rope.scaling.factor", float(sp["scaling"][1]))
        if len(sp["scaling"]) > 2:
            gw.add(f"{a}.rope.scaling.original_context_length", int(sp["scaling"][2]))
    for k, v in (extra or {}).items():
        gw.add(k, v)
    if tokenizer:
        toks, types = chatml_vocab(sp["vocab"])
        gw.add("tokenizer.ggml.model", "gpt2")
        gw.add("tokenizer.ggml.pre", "qwen2")
        gw.add("tokenizer.ggml.tokens", toks)
        gw.add("tokenizer.ggml.token_type", types)
        gw.add("tokenizer.ggml.merges", ["a b"])
        gw.add("tokenizer.ggml.eos_token_id", 258)
        gw.add("tokenizer.chat_template", "{% for m in messages %}<|im_start|>{{ m.role }}\n{{ m.content }}"
                                          "<|im_end|>\n{% endfor %}<|im_start|>assistant\n")
    for n, arr in w.items():
        gw.add_tensor(n, arr, "F32")
    gw.write()
    return str(path)


def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def rotate(x, pos, sp, w):
    """x [n, heads, hd] fp64 at positions pos [n]: the file's rotation (NeoX halves or adjacent pairs)."""
    hd = sp["hd"]
    inv = 1.0 / (sp["rope_base"] ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    if "rope_freqs.weight" in w:
        inv = inv / torch.from_numpy(w["rope_freqs.weight"]).double()
    p = pos.double()
    if sp["scaling"] and sp["scaling"][0] == "linear":
        p = p / sp["scaling"][1]
    ang = p[:, None] * inv[None, :]
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
    if sp["arch"] in NEOX:
        a, b = x[..., : hd // 2], x[..., hd // 2:]
        return torch.cat([a * c - b * s, a * s + b * c], -1)
    a, b = x[..., 0::2], x[..., 1::2]
    return torch.stack([a * c - b * s, a * s + b * c], -1).flatten(-2)


def ref_logits(sp, w, ids, tw=None):
    """fp64 logits [len(ids), vocab] of every position.  tw: the weights as fp64 tensors (built once)."""
    t = tw or {n: torch.from_numpy(a).double() for n, a in w.items()}
    H, KVH, hd, eps = sp["H"], sp["KVH"], sp["hd"], sp["eps"]
    n = len(ids)
    pos = torch.arange(n)
    x = t["token_embd.weight"][torch.tensor(ids)]
    causal = torch.ones((n, n), dtype=torch.bool).tril()
    for i in range(sp["layers"]):
        p = f"blk.{i}."
        h = _rms(x, t[p + "attn_norm.weight"], eps)
        q, k, v = (h @ t[p + f"attn_{c}.weight"].T for c in "qkv")
        if sp["bias"]:
            q, k, v = q + t[p + "attn_q.bias"], k + t[p + "attn_k.bias"], v + t[p + "attn_v.bias"]
        q, k, v = q.view(n, H, hd), k.view(n, KVH, hd), v.view(n, KVH, hd)
        if sp["norm"]:
            q, k = _rms(q, t[p + "attn_q_norm.weight"], eps), _rms(k, t[p + "attn_k_norm.weight"], eps)
        q, k = rotate(q, pos, sp, w), rotate(k, pos, sp, w)
        k, v = k.repeat_interleave(H // KVH, 1), v.repeat_interleave(H // KVH, 1)
        sc = torch.einsum("qhd,khd->hqk", q, k) * hd ** -0.5
        pr = torch.softmax(sc.masked_fill(~causal, -float("inf")), -1)
        a = torch.einsum("hqk,khd->qhd", pr, v).reshape(n, H * hd)
        x = x + a @ t[p + "attn_output.weight"].T
        h = _rms(x, t[p + "ffn_norm.weight"], eps)
        x = x + (torch.nn.functional.silu(h @ t[p + "ffn_gate.weight"].T) * (h @ t[p + "ffn_up.weight"].T)) \
            @ t[p + "ffn_down.weight"].T
    head = t.get("output.weight", t["token_embd.weight"])
    return _rms(x, t["output_norm.weight"], eps) @ head.T


def prompt(n, k=0):
    return [(7 + 13 * i + 5 * k + i * i // 3) % 256 for i in range(n)]
