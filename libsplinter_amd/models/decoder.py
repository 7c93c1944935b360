"""Causal decoder (llama architecture) for the splainference completion daemon.

The reference completion daemon drives llama.cpp (/root/reference/
splainference.cpp:181-400: prefill, then one llama_decode per sampled token,
top-p 0.9 / temperature 0.7 / seeded dist sampler chain, :272-279).  This is
the MI355X replacement, demo-grade as SURVEY §2.1 N8 scopes it:

* weights: GGUF arch "llama" (token_embd, blk.N.{attn_norm, attn_q, attn_k,
  attn_v, attn_output, ffn_norm, ffn_gate, ffn_up, ffn_down}, output_norm,
  output) dequantised on the device, or random init (``DecoderConfig``); arch "qwen2" adds
  blk.N.attn_{q,k,v}.bias, arch "qwen3" blk.N.attn_{q,k}_norm.weight and a head dim of its own
  (attention.key_length); their NeoX rotation becomes the adjacent-pair one by a row permutation at load,
  and bias + q/k norm + RoPE (+ cache append) are one fused launch (``csrc/hip/decoder_arch.hip``); arch
  "qwen3moe", and "llama" with expert_count > 0 (mixtral), replace every layer's feed-forward by a mixture of
  experts (blk.N.ffn_gate_inp, ffn_{gate,up,down}_exps stacked over the experts): the k largest router logits
  pick each token's experts, on the device (``csrc/hip/decoder_moe.hip``); any other architecture or expert
  layout is refused (``config_from_gguf``);
* every projection (q|k|v fused, o + residual, gate|up + SwiGLU, down +
  residual, LM head) runs on the gfx950 MFMA GEMM (``nomic_gemm``) with its
  fused epilogues; RMSNorm and RoPE (llama "normal" adjacent-pair rotation, as
  llama.cpp applies for arch llama, in place on the q|k GEMM output) are the
  HIP kernels of ``csrc/hip/decoder_kernels.hip``, and so is the per-token
  decode attention over the KV cache (``dec_attn_decode``), the causal prefill
  attention of a fresh or continued prompt over the cache (``dec_attn_prefill_kv``,
  head dim 64 / 128) and the nucleus sampler (``dec_sample_ws``);
* tokenizer: the GGUF's own -- SentencePiece score merging (model "llama") or
  byte-level BPE over the merges (model "gpt2"), models/llm_tokenizer.py -- or,
  for random init, bytes 0..255 + BOS/EOS.

On a host without a GPU the same module runs entirely in torch on the CPU
(``device="cpu"``) so the daemon's label state machine is testable anywhere;
on a GPU box the projections MUST go through the HIP GEMM (no silent fallback).
"""
from __future__ import annotations

import ctypes
import math
import re
from collections.abc import Mapping
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

BYTE_BOS, BYTE_EOS = 256, 257


@dataclass
class DecoderConfig:
    vocab: int = 384          # 256 bytes + BOS/EOS, padded to a multiple of 128
    d: int = 512
    layers: int = 4
    heads: int = 8
    kv_heads: int = 8
    ffn: int = 1536
    eps: float = 1e-5
    rope_base: float = 10000.0
    n_ctx: int = 2048
    arch: str = "llama"       # general.architecture: one of SUPPORTED_ARCHS
    qkv_bias: bool = False    # blk.N.attn_{q,k,v}.bias (qwen2)
    qk_norm: bool = False     # blk.N.attn_{q,k}_norm.weight, a per-head RMSNorm ahead of the rotation (qwen3)
    key_length: Optional[int] = None  # {arch}.attention.key_length: the head dim where heads * head_dim != d
    rope_scale: float = 1.0   # rope.scaling.factor of type "linear": positions are divided by it
    experts: int = 0          # {arch}.expert_count: 0 is a dense feed-forward, else every layer is mixture-of-experts
    experts_used: int = 0     # {arch}.expert_used_count: experts per token (k)
    expert_ffn: int = 0       # {arch}.expert_feed_forward_length: an expert's hidden width (F)

    @property
    def head_dim(self) -> int:
        return self.key_length or self.d // self.heads

    @property
    def q_dim(self) -> int:
        """Width of the q columns, of the attention output and of the o-projection's K (d unless key_length)."""
        return self.heads * self.head_dim


# general.architecture values CausalLM computes (mistral files say "llama"); qwen2 / qwen3 rotate the halves
# of a head against each other (NeoX), which the loader turns into adjacent pairs by permuting rows
SUPPORTED_ARCHS = ("llama", "qwen2", "qwen3", "qwen3moe")
NEOX_ARCHS = ("qwen2", "qwen3", "qwen3moe")
# mixture-of-experts limits of the router kernel (csrc/hip/decoder_moe.hip) and the one-token GEMV's K
MOE_MAX_EXPERTS, MOE_MAX_USED, GEMV_MAX_K = 256, 8, 16384


def neox_rows_to_pairs(t: torch.Tensor, hd: int) -> torch.Tensor:
    """Rows of t grouped in heads of hd: new row 2j of a head is old row j, new row 2j + 1 old row j + hd/2.
    Applied to attn_q / attn_k weights, their biases and the per-head norm weights, it makes the adjacent-pair
    rotation of the permuted head the NeoX rotation of the original one; q . k and the RMS over a head do not
    change under a permutation applied to both."""
    r = t.reshape(-1, 2, hd // 2, *t.shape[1:])
    return r.transpose(1, 2).reshape(t.shape).contiguous()


class ByteTokenizer:
    """bytes 0..255, BOS 256, EOS 257 (random-init demo vocabulary)."""
    bos_id, eos_id = BYTE_BOS, BYTE_EOS

    def encode(self, text: str, add_bos: bool = True) -> List[int]:
        return ([self.bos_id] if add_bos else []) + list(text.encode("utf-8"))

    def piece(self, tok: int) -> bytes:
        return bytes([tok]) if tok < 256 else b""

    def is_eog(self, tok: int) -> bool:
        return tok == self.eos_id

    def printable_mask(self, vocab: int) -> torch.Tensor:
        m = torch.zeros(vocab, dtype=torch.bool)
        m[32:127] = True
        m[10] = True
        m[self.eos_id] = True
        return m


def random_decoder_weights(cfg: DecoderConfig, seed: int = 0, std: float = 0.02) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    f = lambda *s: (rng.standard_normal(s) * std).astype(np.float32)  # noqa: E731
    kvd = cfg.kv_heads * cfg.head_dim
    w = {"token_embd.weight": f(cfg.vocab, cfg.d), "output_norm.weight": np.ones(cfg.d, np.float32),
         "output.weight": f(cfg.vocab, cfg.d)}
    for i in range(cfg.layers):
        p = f"blk.{i}."
        w[p + "attn_norm.weight"] = np.ones(cfg.d, np.float32)
        w[p + "attn_q.weight"] = f(cfg.q_dim, cfg.d)
        w[p + "attn_k.weight"] = f(kvd, cfg.d)
        w[p + "attn_v.weight"] = f(kvd, cfg.d)
        w[p + "attn_output.weight"] = f(cfg.d, cfg.q_dim)
        w[p + "ffn_norm.weight"] = np.ones(cfg.d, np.float32)
        if cfg.experts:
            continue
        w[p + "ffn_gate.weight"] = f(cfg.ffn, cfg.d)
        w[p + "ffn_up.weight"] = f(cfg.ffn, cfg.d)
        w[p + "ffn_down.weight"] = f(cfg.d, cfg.ffn)
    # the extras are drawn after every matrix, so a config without them keeps its weights
    for i in range(cfg.layers):
        p = f"blk.{i}."
        if cfg.qkv_bias:
            for n, rows in (("q", cfg.q_dim), ("k", kvd), ("v", kvd)):
                w[p + f"attn_{n}.bias"] = (rng.standard_normal(rows) * 0.5).astype(np.float32)
        if cfg.qk_norm:
            for n in ("q", "k"):
                w[p + f"attn_{n}_norm.weight"] = (1.0 + 0.1 * rng.standard_normal(cfg.head_dim)).astype(np.float32)
    # the experts come last of all: router [E, d], gate / up [E, F, d], down [E, d, F]
    for i in range(cfg.layers if cfg.experts else 0):
        p = f"blk.{i}."
        w[p + "ffn_gate_inp.weight"] = f(cfg.experts, cfg.d)
        w[p + "ffn_gate_exps.weight"] = f(cfg.experts, cfg.expert_ffn, cfg.d)
        w[p + "ffn_up_exps.weight"] = f(cfg.experts, cfg.expert_ffn, cfg.d)
        w[p + "ffn_down_exps.weight"] = f(cfg.experts, cfg.d, cfg.expert_ffn)
    return w


def gguf_quant_kind(g) -> str:
    """"q4" when most projection weights (2-D blk.* tensors, and the stacked 3-D *_exps tensors that hold nearly
    all of a mixture-of-experts file) of a GGUF are 4-bit types (Q4_0, Q4_1, Q4_K), else "bf16"."""
    proj = [t for n, t in g.tensors.items() if n.startswith("blk.") and
            (len(t.shape) == 2 or (len(t.shape) == 3 and n.endswith("_exps.weight")))]
    q4 = sum(t.nelems for t in proj if t.ggml_type in (2, 3, 12))
    return "q4" if proj and q4 * 2 > sum(t.nelems for t in proj) else "bf16"


def _moe_config(g, a: str, cfg: DecoderConfig) -> None:
    """The mixture-of-experts keys of the file into cfg, and the refusal, by name, of what CausalLM does not
    compute: shared experts, the old one-tensor-per-expert layout, dense and expert layers in one file, and a
    router wider than the kernel's."""
    sup = f"(supported: {', '.join(SUPPORTED_ARCHS)}; experts: stacked *_exps tensors in every layer, no shared expert)"
    names = list(g.tensors)
    E = int(g.get(f"{a}.expert_count", 0) or 0)
    shared = [n for n in names if "_shexp" in n]
    if shared or int(g.get(f"{a}.expert_shared_count", 0) or 0) > 0:
        what = f"tensor {shared[0]}" if shared else f"{a}.expert_shared_count {int(g.get(f'{a}.expert_shared_count'))}"
        raise ValueError(f"architecture {a!r} with shared experts ({what}) is not supported {sup}")
    split = [n for n in names if re.fullmatch(r"blk\.\d+\.ffn_(gate|up|down)\.\d+\.weight", n)]
    if split:
        raise ValueError(f"architecture {a!r} with one tensor per expert ({split[0]}) is not supported {sup}")
    moe = {int(n.split(".")[1]) for n in names if re.fullmatch(r"blk\.\d+\.ffn_gate_inp\.weight", n)}
    dense = {int(n.split(".")[1]) for n in names if re.fullmatch(r"blk\.\d+\.ffn_gate\.weight", n)}
    if moe and dense:
        raise ValueError(f"architecture {a!r} with dense layers ({len(dense)}, first blk.{min(dense)}) beside expert "
                         f"layers ({len(moe)}, first blk.{min(moe)}) is not supported {sup}")
    if (E > 0) != bool(moe):
        raise ValueError(f"architecture {a!r} with {a}.expert_count {E} and {len(moe)} router tensors "
                         f"(blk.N.ffn_gate_inp.weight) is not supported {sup}")
    if not E:
        return
    k = int(g.get(f"{a}.expert_used_count", 0) or 0)
    if E > MOE_MAX_EXPERTS or not 1 <= k <= min(MOE_MAX_USED, E):
        raise ValueError(f"architecture {a!r} with {E} experts, {k} used per token is not supported "
                         f"(up to {MOE_MAX_EXPERTS} experts, 1 to {MOE_MAX_USED} used and no more than there are) {sup}")
    cfg.experts, cfg.experts_used = E, k
    cfg.expert_ffn = int(g.get(f"{a}.expert_feed_forward_length", None) or cfg.ffn)


def config_from_gguf(g) -> DecoderConfig:
    """ValueError for an architecture CausalLM does not compute, for partial rotary and for a rope scaling type
    other than none / linear / yarn: such a file would load and write wrong text."""
    a = g.arch() or "llama"
    if a not in SUPPORTED_ARCHS:
        raise ValueError(f"architecture {a!r} is not supported (supported: {', '.join(SUPPORTED_ARCHS)})")
    get = lambda k, d: g.get(f"{a}.{k}", d)  # noqa: E731
    tok = g.tensors["token_embd.weight"]
    d = int(get("embedding_length", 4096))
    heads = int(get("attention.head_count", 32))
    kl = get("attention.key_length", None)
    cfg = DecoderConfig(vocab=int(tok.shape[0]), d=d, layers=int(get("block_count", 32)), heads=heads,
                        kv_heads=int(get("attention.head_count_kv", heads)), ffn=int(get("feed_forward_length", 11008)),
                        eps=float(get("attention.layer_norm_rms_epsilon", 1e-5)),
                        rope_base=float(get("rope.freq_base", 10000.0)), n_ctx=int(get("context_length", 2048)),
                        arch=a, qkv_bias="blk.0.attn_q.bias" in g.tensors,
                        qk_norm="blk.0.attn_q_norm.weight" in g.tensors,
                        key_length=int(kl) if kl is not None and int(kl) * heads != d else None)
    _moe_config(g, a, cfg)
    rot = get("rope.dimension_count", None)
    if rot is not None and int(rot) != cfg.head_dim:
        raise ValueError(f"architecture {a!r} with partial rotary (rope.dimension_count {int(rot)} of head dim "
                         f"{cfg.head_dim}) is not supported (supported: {', '.join(SUPPORTED_ARCHS)}, full rotary)")
    kind = get("rope.scaling.type", None) or "none"
    if kind == "linear":
        cfg.rope_scale = float(get("rope.scaling.factor", 1.0))
    elif kind == "yarn":
        orig = int(get("rope.scaling.original_context_length", cfg.n_ctx))
        cfg.n_ctx = min(cfg.n_ctx, orig)
        print(f"[Startup]: rope scaling yarn is not applied: context window clamped to the original {cfg.n_ctx} "
              "tokens.", flush=True)
    elif kind != "none":
        raise ValueError(f"architecture {a!r} with rope.scaling.type {kind!r} is not supported (none, linear, yarn)")
    return cfg


class LazyTensors(Mapping):
    """name -> tensor, made by ``load(name)`` at every access and not kept: what CausalLM is handed where the
    whole set of fp32 tensors would not fit in host memory (CausalLM.from_gguf)."""

    def __init__(self, names, load):
        self._names, self._load = tuple(names), load
        self._set = frozenset(self._names)

    def __getitem__(self, n):
        if n not in self._set:
            raise KeyError(n)
        return self._load(n)

    def __contains__(self, n):
        return n in self._set

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)


class Q4Weight:
    """A projection W [N, K] resident as Q4G32 (csrc/hip/decoder_kernels.hip): 4-bit nibbles
    ``q`` uint8 [N, K/2] plus one bf16 (d, m) pair per 32-k group ``sm`` int32 [N, K/32], w = d q + m;
    0.625 B per weight instead of 2.  Decode reads it with dec_gemv_q4; prefill dequantises one matrix
    at a time into a bf16 scratch for the MFMA GEMM.  The role of llama.cpp's Q4 weights in the
    reference's llama_decode (splainference.cpp:272-330)."""

    bits = 4  # Q8Weight: 8; picks the dec_q<bits>_* symbols and the bytes per row, K * bits / 8

    def __init__(self, q: torch.Tensor, sm: torch.Tensor):
        self.q, self.sm = q, sm
        self.shape = (q.shape[0], q.shape[1] * 8 // self.bits)

    @classmethod
    def quantize(cls, L, w: torch.Tensor):
        from .nomic import _chk, _stream
        w = w.to(torch.bfloat16).contiguous()
        N, K = w.shape
        q = torch.empty((N, K * cls.bits // 8), dtype=torch.uint8, device=w.device)
        sm = torch.empty((N, K // 32), dtype=torch.int32, device=w.device)
        name = f"dec_q{cls.bits}_quantize"
        _chk(getattr(L, name)(w.data_ptr(), N, K, q.data_ptr(), sm.data_ptr(), _stream()), name[4:])
        return cls(q, sm)

    def dequant(self, L, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        from .nomic import _chk, _stream
        N, K = self.shape
        if out is None:
            out = torch.empty((N, K), dtype=torch.bfloat16, device=self.q.device)
        name = f"dec_q{self.bits}_dequant"
        _chk(getattr(L, name)(self.q.data_ptr(), self.sm.data_ptr(), N, K, out.data_ptr(), _stream()), name[4:])
        return out

    def nbytes(self) -> int:
        return self.q.numel() + self.sm.numel() * 4

    def rows(self, a: int, b: int):
        """Rows a .. b-1 as a weight of their own, over the same memory (one expert of a stacked matrix)."""
        return type(self)(self.q[a:b], self.sm[a:b])


class Q8Weight(Q4Weight):
    """Q8G32: one byte per weight (u in 0..255) and the same bf16 (d, m) pair per 32-k group,
    w = d u + m; 1.125 B per weight.  Holds the tensors a mostly-4-bit GGUF keeps at more than 4
    bits (a Q4_K_M file's Q6_K attn_v / ffn_down / output), so they are not re-gridded below the
    file's precision.  Decode reads it with dec_gemv_q8, prefill dequantises with dec_q8_dequant."""
    bits = 8


# GGUF tensor types stored at <= 4 bits per weight (Q4_0, Q4_1, Q2_K, Q3_K, Q4_K, IQ2/IQ3/IQ4, IQ1):
# Q4G32 keeps them at no loss of grid resolution; every other type (Q5_x, Q6_K, Q8_0, F16, BF16,
# F32) goes to Q8G32
GGML_LE4 = {2, 3, 10, 11, 12, 16, 17, 18, 19, 20, 21, 22, 23, 29}


class CausalLM:
    def __init__(self, cfg: DecoderConfig, tensors: Dict[str, torch.Tensor], device: str = "cuda",
                 quant: str = "bf16", ggml_types: Optional[Dict[str, int]] = None):
        """quant "q4": every projection (qkv, o, up|gate, down, LM head) is kept as a Q4Weight
        (GPU only) -- except those whose source GGUF tensors (``ggml_types``, name -> GGML type)
        hold more than 4 bits per weight, which are kept as Q8Weight; "bf16": bf16 weights."""
        if quant not in ("bf16", "q4"):
            raise ValueError(f"quant must be bf16 or q4, not {quant!r}")
        self.cfg = cfg
        self.device = device
        self.hip = device != "cpu"
        self.quant = quant if self.hip else "bf16"
        dt = torch.bfloat16 if self.hip else torch.float32
        hd = cfg.head_dim
        # NeoX rotation as adjacent pairs: permute the q / k rows of every head (and what goes with them) on
        # the fp32 tensors, ahead of any 4- / 8-bit re-gridding (groups run along K, so rows move whole).
        # The cache holds permuted k rows; nothing outside attention reads them.  ``tensors`` may dequantise
        # on access (LazyTensors), so every tensor is taken once, where it is used.
        neox = ("attn_q.weight", "attn_k.weight", "attn_q.bias", "attn_k.bias", "attn_q_norm.weight",
                "attn_k_norm.weight") if cfg.arch in NEOX_ARCHS else ()

        def src(n):
            t = tensors[n]
            return neox_rows_to_pairs(t.float(), hd) if n.startswith("blk.") and n.split(".", 2)[2] in neox else t

        T = lambda n: src(n).to(device=device, dtype=dt).contiguous()  # noqa: E731
        self.emb = T("token_embd.weight")
        self.norm_out = T("output_norm.weight").float()
        head = tensors["output.weight" if "output.weight" in tensors else "token_embd.weight"]
        vpad = (cfg.vocab + 127) // 128 * 128
        hw = torch.zeros((vpad, cfg.d), dtype=dt, device=device)
        hw[: cfg.vocab] = head.to(device=device, dtype=dt)
        self.head = hw
        self.layers = []
        if self.hip:
            self._declare()
        gt = ggml_types or {}

        def Q(t, *names):
            if self.quant != "q4":
                return t
            wide = any(n in gt and gt[n] not in GGML_LE4 for n in names)
            return (Q8Weight if wide else Q4Weight).quantize(self.L, t)

        self.head = Q(self.head, "output.weight" if "output.weight" in tensors else "token_embd.weight")
        self.extras = cfg.qkv_bias or cfg.qk_norm  # the fused q/k preparation stands where RoPE stood
        E, EF = cfg.experts, cfg.expert_ffn
        if E and (E > MOE_MAX_EXPERTS or not 1 <= cfg.experts_used <= min(MOE_MAX_USED, E) or EF < 16 or EF % 16):
            raise ValueError(f"{E} experts, {cfg.experts_used} used, expert width {EF}: up to {MOE_MAX_EXPERTS} "
                             f"experts, 1 to {MOE_MAX_USED} used, a width that is a multiple of 16")
        if E and self.hip and (EF % 64 or EF > GEMV_MAX_K):
            raise ValueError(f"expert_feed_forward_length {EF} is not supported on the GPU: the expert kernels take "
                             f"a multiple of 64 up to {GEMV_MAX_K}")
        # debug hooks of the eager mixture-of-experts layer, both off: a list that collects every layer call's
        # chosen ids [n, k]; per-layer ids [n, k] used in place of the layer's own choice
        self.route_log: Optional[list] = None
        self.route_force: Optional[list] = None
        F32 = lambda n: src(n).to(device=device, dtype=torch.float32).contiguous()  # noqa: E731
        from .nomic import pack_upgate
        for i in range(cfg.layers):
            p = f"blk.{i}."
            qkv = torch.cat([T(p + "attn_q.weight"), T(p + "attn_k.weight"), T(p + "attn_v.weight")], 0)
            lw = {"n1": T(p + "attn_norm.weight").float(),
                  "qkv": Q(qkv.contiguous(), p + "attn_q.weight", p + "attn_k.weight", p + "attn_v.weight"),
                  "o": Q(T(p + "attn_output.weight"), p + "attn_output.weight"),
                  "n2": T(p + "ffn_norm.weight").float()}
            if E:
                # experts stacked along rows: up|gate [E * 2F, d], each expert's 2F rows packed on their own, and
                # down [E * d, F]; the router stays bf16, with a copy zero-padded to the GEMM's 128-row multiple
                up, gate = T(p + "ffn_up_exps.weight"), T(p + "ffn_gate_exps.weight")
                ug = torch.cat([pack_upgate(up[e], gate[e]) for e in range(E)], 0)
                del up, gate
                lw["ug"] = Q(ug.contiguous(), p + "ffn_gate_exps.weight", p + "ffn_up_exps.weight")
                lw["down"] = Q(T(p + "ffn_down_exps.weight").reshape(E * cfg.d, EF), p + "ffn_down_exps.weight")
                rp = torch.zeros(((E + 127) // 128 * 128, cfg.d), dtype=dt, device=device)
                rp[:E] = T(p + "ffn_gate_inp.weight")
                lw["router_pad"], lw["router"] = rp, rp[:E]
            else:
                gate, up = T(p + "ffn_gate.weight"), T(p + "ffn_up.weight")
                # SwiGLU epilogue layout: rows interleaved [up16 | gate16] (nomic_api.h NOMIC_EPI_SWIGLU)
                ug = pack_upgate(up, gate)
                lw["ug"] = Q(ug.contiguous(), p + "ffn_gate.weight", p + "ffn_up.weight")
                lw["down"] = Q(T(p + "ffn_down.weight"), p + "ffn_down.weight")
                del gate, up
            self.layers.append(lw)
            # the architecture's extras, fp32: the fused bias [(H + 2 KVH) hd] and the per-head norm weights [hd]
            lw["qkv_b"] = torch.cat([F32(p + f"attn_{c}.bias") for c in "qkv"]) if cfg.qkv_bias else None
            lw["qn"] = F32(p + "attn_q_norm.weight") if cfg.qk_norm else None
            lw["kn"] = F32(p + "attn_k_norm.weight") if cfg.qk_norm else None
            del qkv, ug
        self._q4_scratch: Optional[torch.Tensor] = None
        # RoPE tables (host only; the kernels read cos / sin): inv_freq[j] over rope_freqs.weight[j] where the
        # file has that tensor (llama 3.1+), positions over the linear scaling factor
        inv = 1.0 / (cfg.rope_base ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
        if "rope_freqs.weight" in tensors:
            inv = inv / tensors["rope_freqs.weight"].to(torch.float64).reshape(-1)[: hd // 2]
        rpos = torch.arange(cfg.n_ctx, dtype=torch.float64)
        if cfg.rope_scale != 1.0:
            rpos = rpos / cfg.rope_scale
        ang = rpos[:, None] * inv[None, :]
        self.cos = ang.cos().float().to(device)
        self.sin = ang.sin().float().to(device)
        # KV cache: one [layers, 2, n_ctx, kv_heads, head_dim] buffer allocated on first use and
        # written in place (no per-token torch.cat regrowth: decode stays O(1) copies per token)
        self.kv: Optional[torch.Tensor] = None
        self.pos = 0
        self.attn_kernel = True  # HIP prefill / decode attention (False: torch SDPA, for A/B only)
        if self.hip:
            ffn = EF if E else cfg.ffn
            ok = all(n % 128 == 0 for n in (cfg.q_dim + 2 * cfg.kv_heads * hd, cfg.d, 2 * ffn, vpad)) \
                and cfg.d % 64 == 0 and ffn % 64 == 0 and cfg.q_dim % 64 == 0
            if not ok:
                raise ValueError("decoder dims must be multiples of 128 (N) / 64 (K) for the MFMA GEMM")
            if self.extras and hd not in (64, 128):
                raise ValueError(f"head dim {hd} with a qkv bias or q/k norms: the fused q/k preparation "
                                 "(dec_qk_prep) takes 64 or 128")
        # HIP attention where the kernels take the head dim (prefill: 64 / 128, decode: any multiple of
        # 64 up to 256); other head dims (e.g. 80, 96) run those layers' attention on torch SDPA
        self.prefill_kernel = hd in (64, 128)
        self.decode_kernel = hd % 64 == 0 and hd <= 256

    def _declare(self):
        """ctypes signatures of the decoder kernels (csrc/hip/decoder_kernels.hip)."""
        from .nomic import _lib
        self.L = _lib()
        if not getattr(self.L, "_dec_declared", False):
            P, c_long, c_int, c_float = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
            self.L.dec_rmsnorm.argtypes = [P, c_long, P, c_long, c_int, c_float, P, c_long, P]
            self.L.dec_rmsnorm.restype = c_int
            self.L.dec_rope.argtypes = [P, c_long, c_long, c_int, c_int, c_int, P, P, P]
            self.L.dec_rope.restype = c_int
            self.L.dec_attn_decode.argtypes = [P, P, P, c_long, c_int, c_int, c_int, c_int, c_float, P, P]
            self.L.dec_attn_decode.restype = c_int
            self.L.dec_attn_decode_st.argtypes = [P, P, P, c_long, c_int, c_int, c_int, c_int, c_float, P, P, P]
            self.L.dec_attn_decode_st.restype = c_int
            self.L.dec_attn_decode_ws.argtypes = [P, P, P, c_long, c_int, c_int, c_int, c_int, c_float, P, P, P, P]
            self.L.dec_attn_decode_ws.restype = c_int
            self.L.dec_attn_prefill_kv.argtypes = [P, c_long, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_float,
                                                   P, c_long, P]
            self.L.dec_attn_prefill_kv.restype = c_int
            self.L.dec_gemv.argtypes = [c_int, P, P, c_float, P, c_int, c_int, P, P, P]
            self.L.dec_gemv.restype = c_int
            self.L.dec_embed_tok.argtypes = [P, c_int, P, P, P]
            self.L.dec_embed_tok.restype = c_int
            self.L.dec_rope_kv.argtypes = [P, c_int, c_int, c_int, P, P, P, P, P, c_long, P]
            self.L.dec_rope_kv.restype = c_int
            self.L.dec_sample_ws.argtypes = [P, c_int, P, c_float, c_float, ctypes.c_uint64, P, c_int, P, P, P]
            self.L.dec_sample_ws.restype = c_int
            self.L.dec_sample_ws_floats.argtypes = []
            self.L.dec_sample_ws_floats.restype = c_long
            self.L.dec_gemv_q4.argtypes = [c_int, P, P, c_float, P, P, c_int, c_int, P, P, P]
            self.L.dec_gemv_q4.restype = c_int
            self.L.dec_q4_quantize.argtypes = [P, c_long, c_int, P, P, P]
            self.L.dec_q4_quantize.restype = c_int
            self.L.dec_q4_dequant.argtypes = [P, P, c_long, c_int, P, P]
            self.L.dec_q4_dequant.restype = c_int
            self.L.dec_gemv_q8.argtypes = [c_int, P, P, c_float, P, P, c_int, c_int, P, P, P]
            self.L.dec_gemv_q8.restype = c_int
            self.L.dec_q8_quantize.argtypes = [P, c_long, c_int, P, P, P]
            self.L.dec_q8_quantize.restype = c_int
            self.L.dec_q8_dequant.argtypes = [P, P, c_long, c_int, P, P]
            self.L.dec_q8_dequant.restype = c_int
            # the batched step (csrc/hip/decoder_batch.hip)
            for name in ("dec_gemm_small", "dec_gemm_small_q4", "dec_gemm_small_q8"):
                planes = [P] if name == "dec_gemm_small" else [P, P]
                getattr(self.L, name).argtypes = [c_int, P, c_long, c_int] + planes + [c_int, c_int, P, c_long, P,
                                                                                      c_long, P]
                getattr(self.L, name).restype = c_int
            self.L.dec_embed_tok_b.argtypes = [P, c_int, P, c_int, P, c_long, P]
            self.L.dec_embed_tok_b.restype = c_int
            self.L.dec_rope_kv_b.argtypes = [P, c_long, c_int, c_int, c_int, c_int, P, P, P, P, P, c_long, c_long, P]
            self.L.dec_rope_kv_b.restype = c_int
            self.L.dec_attn_b_ws_floats.argtypes = [c_int, c_int, c_int]
            self.L.dec_attn_b_ws_floats.restype = c_long
            self.L.dec_attn_decode_b.argtypes = [P, c_long, P, P, c_long, c_long, c_int, c_int, c_int, c_int, c_int,
                                                 c_float, P, c_long, P, P, P]
            self.L.dec_attn_decode_b.restype = c_int
            self.L.dec_sample_b_ws_floats.argtypes = [c_int]
            self.L.dec_sample_b_ws_floats.restype = c_long
            self.L.dec_sample_b.argtypes = [P, c_long, c_int, c_int, P, c_float, c_float, P, c_int, P, P, P]
            self.L.dec_sample_b.restype = c_int
            # the batched prompt prefill: the segment table is a host int32 [nseg][4] array
            self.L.dec_rope_kv_seg.argtypes = [P, c_long, c_long, P, c_int, c_int, c_int, c_int, P, P, P, P, c_long,
                                               c_long, c_int, c_int, P]
            self.L.dec_rope_kv_seg.restype = c_int
            self.L.dec_attn_prefill_kv_seg.argtypes = [P, c_long, c_long, P, c_int, P, P, c_long, c_long, c_int, c_int,
                                                       c_int, c_int, c_int, c_float, P, c_long, P]
            self.L.dec_attn_prefill_kv_seg.restype = c_int
            # the shared prompt prefix: the destination slots are a host int32 [ndst] array
            self.L.dec_kv_rows_fanout.argtypes = [P, c_long, c_int, P, c_long, c_long, P, c_int, c_int, c_int, c_int,
                                                  c_int, c_int, P]
            self.L.dec_kv_rows_fanout.restype = c_int
            # the fused q/k preparation (csrc/hip/decoder_arch.hip): each twin's arguments, then the fp32 bias,
            # the q and k norm weights, the norm's eps
            ex = [P, P, P, c_float, P]
            self.L.dec_qk_prep.argtypes = [P, c_long, c_long, c_int, c_int, c_int, c_int, P, P] + ex
            self.L.dec_qk_prep_kv.argtypes = self.L.dec_rope_kv.argtypes[:-1] + ex
            self.L.dec_qk_prep_kv_b.argtypes = self.L.dec_rope_kv_b.argtypes[:-1] + ex
            self.L.dec_qk_prep_kv_seg.argtypes = self.L.dec_rope_kv_seg.argtypes[:-1] + ex
            for name in ("dec_qk_prep", "dec_qk_prep_kv", "dec_qk_prep_kv_b", "dec_qk_prep_kv_seg"):
                getattr(self.L, name).restype = c_int
            # mixture of experts (csrc/hip/decoder_moe.hip): ids / k / E follow the weight planes
            moe = {"dec_moe_route": [P, c_long, c_int, c_int, c_int, P, P, P],
                   "dec_gemv_moe": [P, P, c_float, P, c_int, c_int, P, c_int, c_int, P, P],
                   "dec_gemv_moe_q4": [P, P, c_float, P, P, c_int, c_int, P, c_int, c_int, P, P],
                   "dec_gemv_moe_down": [P, P, c_int, c_int, P, P, c_int, c_int, P, P, P],
                   "dec_gemv_moe_down_q4": [P, P, P, c_int, c_int, P, P, c_int, c_int, P, P, P],
                   "dec_moe_plan": [P, c_int, c_int, c_int, c_int, P, P, P, P],
                   "dec_moe_gather": [P, c_long, c_int, c_int, c_int, P, c_int, P, P],
                   "dec_moe_combine": [P, c_int, c_int, c_int, c_int, P, P, P, c_long, P, c_long, P]}
            moe["dec_gemv_moe_q8"], moe["dec_gemv_moe_down_q8"] = moe["dec_gemv_moe_q4"], moe["dec_gemv_moe_down_q4"]
            for name, args in moe.items():
                getattr(self.L, name).argtypes = args
                getattr(self.L, name).restype = c_int
            self.L._dec_declared = True

    def _prep_args(self, lw) -> tuple:
        """The trailing arguments of a dec_qk_prep* call for one layer: bias, q norm, k norm (null where the
        architecture has none), eps."""
        P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return P(lw["qkv_b"]), P(lw["qn"]), P(lw["kn"]), self.cfg.eps

    @classmethod
    def random(cls, cfg: DecoderConfig, seed: int = 0, device: str = "cuda", quant: str = "bf16") -> "CausalLM":
        return cls(cfg, {k: torch.from_numpy(v) for k, v in random_decoder_weights(cfg, seed).items()}, device,
                   quant=quant)

    @classmethod
    def from_gguf(cls, path: str, device: str = "cuda", quant: str = "auto"):
        """quant "auto": Q4G32 when most projection weights of the file are 4-bit GGUF types
        (Q4_0 / Q4_1 / Q4_K), with the file's wider tensors (a Q4_K_M file's Q6_K) on Q8G32; else bf16."""
        from .gguf import GGUFFile
        g = GGUFFile(path)
        cfg = config_from_gguf(g)
        if quant == "auto":
            quant = gguf_quant_kind(g)
        # fp32 on access, one tensor at a time: a mixture-of-experts file's stacked experts never stand in host
        # memory as fp32 all at once (CausalLM takes a layer's, converts them and lets go)
        tensors = LazyTensors(g.tensors, lambda n: torch.from_numpy(np.ascontiguousarray(g.to_numpy_f32(n))))
        from .llm_tokenizer import tokenizer_from_gguf
        tok = tokenizer_from_gguf(g) or ByteTokenizer()  # SPM / BPE by tokenizer.ggml.model
        if not hasattr(tok, "chat_template"):
            tok.chat_template = None  # rendered by splainference.build_prompt
        types = {n: t.ggml_type for n, t in g.tensors.items()}
        return cls(cfg, tensors, device, quant=quant if device != "cpu" else "bf16", ggml_types=types), tok

    # ------------------------------------------------------------- pieces --
    def _dense(self, w):
        """The bf16 matrix the MFMA GEMM reads: a 4- / 8-bit one is dequantised into the shared scratch."""
        if not isinstance(w, Q4Weight):
            return w
        n_el = w.shape[0] * w.shape[1]
        if self._q4_scratch is None or self._q4_scratch.numel() < n_el:
            self._q4_scratch = torch.empty(n_el, dtype=torch.bfloat16, device=self.device)
        return w.dequant(self.L, self._q4_scratch[:n_el].view(w.shape))

    def _mm(self, mode: int, x: torch.Tensor, w, out_cols: int, res: Optional[torch.Tensor] = None):
        """x [M, K] @ w[N, K]^T with a fused epilogue; HIP MFMA on the GPU, torch on the CPU."""
        M, K = x.shape
        w = self._dense(w)  # prefill runs on bf16 weights
        if not self.hip:
            if mode == 2:
                up, gate = self._split_ug(x @ w.T)
                return up * torch.nn.functional.silu(gate)
            y = x @ w.T
            return y + res if res is not None else y
        from .nomic import _chk, _stream
        Mp = (M + 127) // 128 * 128
        if Mp != M:
            xp = torch.zeros((Mp, K), dtype=x.dtype, device=x.device)
            xp[:M] = x
            x = xp
        x = x.contiguous()
        f32 = mode == 4
        out = torch.empty((Mp, out_cols), dtype=torch.float32 if f32 else torch.bfloat16, device=x.device)
        rp = None
        if res is not None:
            rp = torch.zeros((Mp, out_cols), dtype=torch.bfloat16, device=x.device)
            rp[:M] = res
        _chk(self.L.nomic_gemm(mode, x.data_ptr(), K, w.data_ptr(), K, M, w.shape[0], K, out.data_ptr(), out_cols,
                               None if rp is None else rp.data_ptr(), out_cols, None, None, 0, _stream()), "gemm")
        return out[:M]

    @staticmethod
    def _split_ug(y: torch.Tensor):
        g = y.reshape(y.shape[0], -1, 2, 16)  # pack_upgate: [up16 | gate16] per 16 outputs
        return g[:, :, 0].reshape(y.shape[0], -1), g[:, :, 1].reshape(y.shape[0], -1)

    def _rms(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        if self.hip:  # dec_rmsnorm (csrc/hip/decoder_kernels.hip): one wave per row
            from .nomic import _chk, _stream
            x = x.contiguous()
            out = torch.empty_like(x)
            _chk(self.L.dec_rmsnorm(x.data_ptr(), x.shape[1], w.data_ptr(), x.shape[0], x.shape[1], self.cfg.eps,
                                    out.data_ptr(), x.shape[1], _stream()), "rmsnorm")
            return out
        xf = x.float()
        y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.cfg.eps) * w
        return y.to(x.dtype)

    def _rope(self, t: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
        # llama "normal" rotation: adjacent pairs (x[2i], x[2i+1])
        c, s = self.cos[pos][:, None, :], self.sin[pos][:, None, :]
        tf = t.float()
        x1, x2 = tf[..., 0::2], tf[..., 1::2]
        out = torch.stack([x1 * c - x2 * s, x1 * s + x2 * c], -1).flatten(-2)
        return out.to(t.dtype)

    def reset(self):
        self.pos = 0

    # ------------------------------------------------------ mixture of experts --
    def _moe(self, li: int, lw, h: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """x + sum over each token's k experts of weight * down_e(SwiGLU(up|gate_e(h))) for the n >= 1 rows of
        h (the normalised x).  Routing: the k largest router logits (ties to the lower index), weighted by
        their softmax probabilities renormalised over the k.  On the GPU the rows are grouped by expert into
        128-row aligned segments (dec_moe_plan / dec_moe_gather), each non-empty expert runs the two MFMA
        GEMMs on its segment, and dec_moe_combine sums back; one host read (the counts) per layer."""
        cfg = self.cfg
        E, k, F, d = cfg.experts, cfg.experts_used, cfg.expert_ffn, cfg.d
        n = h.shape[0]
        forced = None
        if self.route_force is not None:
            forced = torch.as_tensor(self.route_force[li], device=self.device).reshape(n, k)
            if int(forced.min()) < 0 or int(forced.max()) >= E:
                raise ValueError(f"route_force names an expert outside 0..{E - 1}")
        if not self.hip:
            logits = (h @ lw["router"].T).float()
            ids = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :k] if forced is None \
                else forced.long()
            w = torch.softmax(logits.gather(1, ids), -1)
            if self.route_log is not None:
                self.route_log.append(ids.to(torch.int32).clone())
            acc = torch.zeros_like(x)
            for e in ids.unique().tolist():
                t, j = (ids == e).nonzero(as_tuple=True)
                up, gate = self._split_ug(h[t] @ lw["ug"][e * 2 * F: (e + 1) * 2 * F].T)
                y = (up * torch.nn.functional.silu(gate)) @ lw["down"][e * d: (e + 1) * d].T
                acc.index_add_(0, t, w[t, j, None].to(y.dtype) * y)
            return x + acc
        from .nomic import _chk, _stream
        L, s = self.L, _stream()
        i32 = dict(dtype=torch.int32, device=self.device)
        logits = self._mm(4, h, lw["router_pad"], lw["router_pad"].shape[0])
        ids = torch.empty((n, k), **i32)
        w = torch.empty((n, k), dtype=torch.float32, device=self.device)
        _chk(L.dec_moe_route(logits.data_ptr(), logits.stride(0), n, E, k, ids.data_ptr(), w.data_ptr(), s), "moe_route")
        if forced is not None:  # the forced set, weighted by this layer's own probabilities over it
            ids = forced.to(torch.int32).contiguous()
            w = torch.softmax(logits[:, :E].gather(1, ids.long()), -1).contiguous()
        if self.route_log is not None:
            self.route_log.append(ids.clone())
        counts, base = torch.empty(E, **i32), torch.empty(E, **i32)
        slot = torch.full((n, k), -1, **i32)
        _chk(L.dec_moe_plan(ids.data_ptr(), n, k, E, 128, counts.data_ptr(), base.data_ptr(), slot.data_ptr(), s),
             "moe_plan")
        cnt = counts.tolist()  # the layer's one host read; the starts follow from the counts
        rows, start = 0, []
        for c in cnt:
            start.append(rows)
            rows += (c + 127) // 128 * 128
        # the GEMM reads whole 128-row tiles: rows no token fills are zero, so that every product is finite
        xg = torch.zeros((rows, d), dtype=torch.bfloat16, device=self.device)
        h = h.contiguous()
        _chk(L.dec_moe_gather(h.data_ptr(), h.stride(0), n, k, d, slot.data_ptr(), rows, xg.data_ptr(), s), "moe_gather")
        f = torch.empty((rows, F), dtype=torch.bfloat16, device=self.device)
        y = torch.empty((rows, d), dtype=torch.float32, device=self.device)
        part = lambda m, a, b: m.rows(a, b) if isinstance(m, Q4Weight) else m[a:b]  # noqa: E731
        for e, c in enumerate(cnt):
            if not c:
                continue
            r0 = start[e]
            ug = self._dense(part(lw["ug"], e * 2 * F, (e + 1) * 2 * F))  # a 4- / 8-bit slice: into the scratch
            _chk(L.nomic_gemm(2, xg[r0:].data_ptr(), d, ug.data_ptr(), d, c, 2 * F, d, f[r0:].data_ptr(), F, None, F,
                              None, None, 0, s), "gemm up|gate (expert)")
            dn = self._dense(part(lw["down"], e * d, (e + 1) * d))
            _chk(L.nomic_gemm(4, f[r0:].data_ptr(), F, dn.data_ptr(), F, c, d, F, y[r0:].data_ptr(), d, None, d,
                              None, None, 0, s), "gemm down (expert)")
        x = x.contiguous()
        out = torch.empty_like(x)
        _chk(L.dec_moe_combine(y.data_ptr(), rows, n, k, d, slot.data_ptr(), w.data_ptr(), x.data_ptr(), d,
                               out.data_ptr(), d, s), "moe_combine")
        return out

    @torch.no_grad()
    def forward(self, ids: List[int]) -> torch.Tensor:
        """Append tokens to the KV cache; returns fp32 logits of the last position."""
        cfg = self.cfg
        hd, H, KVH, qd = cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.q_dim
        n = len(ids)
        if self.pos + n > cfg.n_ctx:
            raise ValueError("context window exceeded")
        pos = torch.arange(self.pos, self.pos + n, device=self.device)
        x = self.emb[torch.tensor(ids, device=self.device)]
        for li, lw in enumerate(self.layers):
            h = self._rms(x, lw["n1"])
            qkv = self._mm(0, h, lw["qkv"], qd + 2 * KVH * hd)
            if self.hip and self.extras:
                # bias, per-head RMSNorm and RoPE in place, one launch where dec_rope stands (dec_qk_prep)
                from .nomic import _chk, _stream
                _chk(self.L.dec_qk_prep(qkv.data_ptr(), qkv.stride(0), n, H, KVH, hd, self.pos, self.cos.data_ptr(),
                                        self.sin.data_ptr(), *self._prep_args(lw), _stream()), "qk_prep")
            elif self.hip:  # RoPE in place over the q|k columns (dec_rope)
                from .nomic import _chk, _stream
                _chk(self.L.dec_rope(qkv.data_ptr(), qkv.stride(0), n, qd + KVH * hd, hd, self.pos,
                                     self.cos.data_ptr(), self.sin.data_ptr(), _stream()), "rope")
            elif lw["qkv_b"] is not None:
                qkv = qkv + lw["qkv_b"]
            q = qkv[:, :qd].reshape(n, H, hd)
            k = qkv[:, qd: qd + KVH * hd].reshape(n, KVH, hd)
            v = qkv[:, qd + KVH * hd:].reshape(n, KVH, hd)
            if not self.hip:
                if lw["qn"] is not None:  # per-head RMSNorm of q and k, ahead of the rotation
                    nrm = lambda t, w: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + cfg.eps) * w  # noqa: E731
                    q, k = nrm(q, lw["qn"]), nrm(k, lw["kn"])
                q, k = self._rope(q, pos), self._rope(k, pos)
            if self.kv is None:
                self.kv = torch.empty((cfg.layers, 2, cfg.n_ctx, KVH, hd), dtype=qkv.dtype, device=self.device)
            self.kv[li, 0, self.pos: self.pos + n] = k
            self.kv[li, 1, self.pos: self.pos + n] = v
            L_ = self.pos + n
            if self.hip and self.attn_kernel and self.prefill_kernel and n > 1:
                # prompt prefill, fresh or continuing a live cache: causal MFMA attention of the n new
                # queries over cache rows 0 .. pos+n-1 (dec_attn_prefill_kv, hd 64 / 128)
                from .nomic import _chk, _stream
                a = torch.empty((n, qd), dtype=qkv.dtype, device=self.device)
                _chk(self.L.dec_attn_prefill_kv(qkv.data_ptr(), qkv.stride(0), self.kv[li, 0].data_ptr(),
                                                self.kv[li, 1].data_ptr(), KVH * hd, n, self.pos, H, KVH, hd,
                                                hd ** -0.5, a.data_ptr(), qd, _stream()), "attn_prefill")
            elif self.hip and self.attn_kernel and self.decode_kernel and n == 1:
                # per-token decode: dec_attn_decode (one workgroup per q head, split-L online softmax)
                from .nomic import _chk, _stream
                a = torch.empty((1, qd), dtype=qkv.dtype, device=self.device)
                qrow = qkv[0, :qd].contiguous()
                _chk(self.L.dec_attn_decode(qrow.data_ptr(), self.kv[li, 0].data_ptr(), self.kv[li, 1].data_ptr(),
                                            KVH * hd, L_, H, KVH, hd, hd ** -0.5, a.data_ptr(), _stream()),
                     "attn_decode")
            else:
                K_, V_ = self.kv[li, 0, :L_], self.kv[li, 1, :L_]
                qh, kh, vh = q.transpose(0, 1), K_.transpose(0, 1), V_.transpose(0, 1)
                # causal over the cache: query i (absolute position pos + i) sees keys 0..pos+i; a single
                # decode token sees the whole cache, so no mask is needed
                # a fresh prompt (pos 0) is plain causal: is_causal lets torch pick its fused kernel instead
                # of the materialised-mask path
                fresh = n > 1 and L_ == n
                mask = None if n == 1 or fresh else \
                    torch.ones((n, L_), dtype=torch.bool, device=self.device).tril(L_ - n)
                a = torch.nn.functional.scaled_dot_product_attention(qh.unsqueeze(0), kh.unsqueeze(0),
                                                                     vh.unsqueeze(0), attn_mask=mask,
                                                                     is_causal=fresh, enable_gqa=KVH != H)[0]
                a = a.transpose(0, 1).reshape(n, qd).contiguous()
            x = self._mm(1, a, lw["o"], cfg.d, res=x)
            h = self._rms(x, lw["n2"])
            if cfg.experts:
                x = self._moe(li, lw, h, x)
                continue
            f = self._mm(2, h, lw["ug"], cfg.ffn)
            x = self._mm(1, f.contiguous(), lw["down"], cfg.d, res=x)
        self.pos += n
        h = self._rms(x[-1:], self.norm_out)
        logits = self._mm(4, h, self.head, self.head.shape[0])
        return logits[0, : cfg.vocab].float()


def _run_step(eng, span: int):
    """One decode step of a DecodeEngine or a BatchDecodeEngine for the attention span ``span``: eager
    launches, or the replay of the step captured for that span (captured on its first use)."""
    if not eng.use_graph:
        eng._enqueue_step(span)
        return
    g = eng.graphs.get(span)
    if g is None:
        # warm up once outside capture (first-launch code-object loading), then capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        saved = eng.st.clone()
        with torch.cuda.stream(side):
            eng._enqueue_step(span)
        torch.cuda.current_stream().wait_stream(side)
        eng.st.copy_(saved)  # the warm-up step is undone: same state, cache rows rewritten next
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng._enqueue_step(span)
        eng.graphs[span] = g
    g.replay()


class DecodeEngine:
    """Token generation with no host compute in the loop (K18): prompt prefill on the MFMA GEMMs
    and the causal MFMA attention, then per token ONE replay of a HIP graph holding the whole
    decode step -- embedding row, per layer (RMSNorm+QKV GEMV, RoPE + KV-cache append, decode
    attention, o GEMV + residual, RMSNorm+up|gate GEMV + SwiGLU, down GEMV + residual), final
    RMSNorm + LM-head GEMV and the top-p / temperature sampler (dec_sample_ws).  Every kernel reads
    the position and the input token from a device state {pos, token, step}, so the captured
    arguments never change; the host reads back only the sampled token id (pinned memory).
    Reference: splainference.cpp:272-365 (sampler chain, llama_decode per token)."""

    def __init__(self, model: "CausalLM", top_p: float = 0.9, temp: float = 0.7, seed: int = 0xFFFFFFFF,
                 mask: Optional[torch.Tensor] = None, use_graph: bool = True):
        assert model.hip, "DecodeEngine runs on the GPU"
        if not model.decode_kernel:
            raise ValueError(f"head dim {model.cfg.head_dim}: the graph decode engine needs a multiple of 64 "
                             "up to 256 (use CausalLM.forward)")
        m, cfg = model, model.cfg
        self.m, self.top_p, self.temp, self.seed = m, float(top_p), float(temp), int(seed) & 0xFFFFFFFFFFFFFFFF
        dev = m.device
        e = dict(device=dev, dtype=torch.bfloat16)
        kvd = cfg.kv_heads * cfg.head_dim
        self.st = torch.zeros(4, dtype=torch.int32, device=dev)      # pos, token, step
        self.xa = torch.empty(cfg.d, **e)
        self.xb = torch.empty(cfg.d, **e)
        self.qkv = torch.empty(cfg.q_dim + 2 * kvd, **e)
        self.attn = torch.empty(cfg.q_dim, **e)
        self.ffn = torch.empty(cfg.experts_used * cfg.expert_ffn if cfg.experts else cfg.ffn, **e)
        # mixture of experts: the router's logits, and per layer the step's chosen experts and their weights
        # (kept per layer so that a step's choices can be read afterwards)
        k = cfg.experts_used
        self.router_logits = torch.zeros(max(cfg.experts, 1), dtype=torch.float32, device=dev)
        self.moe_ids = [torch.zeros(k, dtype=torch.int32, device=dev) for _ in range(cfg.layers if k else 0)]
        self.moe_w = [torch.zeros(k, dtype=torch.float32, device=dev) for _ in range(cfg.layers if k else 0)]
        self.logits = torch.empty(m.head.shape[0], dtype=torch.float32, device=dev)
        self.attn_ws = torch.empty(cfg.heads * 32 * (cfg.head_dim + 2), dtype=torch.float32, device=dev)  # split-L
        self.samp_ws = torch.empty(m.L.dec_sample_ws_floats(), dtype=torch.float32, device=dev)  # multi-block sampler
        self.host_tok = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self.mask = mask[: cfg.vocab].to(device=dev, dtype=torch.uint8).contiguous() if mask is not None else None
        if m.kv is None:
            m.kv = torch.empty((cfg.layers, 2, cfg.n_ctx, cfg.kv_heads, cfg.head_dim), dtype=torch.bfloat16, device=dev)
        self.use_graph = use_graph
        self.graphs = {}  # attention span (512 or the capacity) -> captured decode step
        self.steps = 0

    def _enqueue_step(self, span: int = 0):
        from .nomic import _chk, _stream
        m, cfg, L = self.m, self.m.cfg, self.m.L
        s = _stream()
        H, KVH, hd = cfg.heads, cfg.kv_heads, cfg.head_dim
        P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _chk(L.dec_embed_tok(m.emb.data_ptr(), cfg.d, self.st.data_ptr(), self.xa.data_ptr(), s), "embed_tok")

        def gemv(mode, x, rms, w, N, K, res, out, what):
            rp = rms.data_ptr() if rms is not None else None
            if isinstance(w, Q4Weight):  # 4-bit: 0.625 B per weight streamed (dec_gemv_q4); 8-bit: 1.125 B
                _chk((L.dec_gemv_q8 if w.bits == 8 else L.dec_gemv_q4)(mode, x.data_ptr(), rp, cfg.eps, w.q.data_ptr(), w.sm.data_ptr(), N, K,
                                   P(res), out.data_ptr(), s), what)
            else:
                _chk(L.dec_gemv(mode, x.data_ptr(), rp, cfg.eps, w.data_ptr(), N, K, P(res), out.data_ptr(), s), what)

        for li, lw in enumerate(m.layers):
            gemv(0, self.xa, lw["n1"], lw["qkv"], lw["qkv"].shape[0], cfg.d, None, self.qkv, "gemv qkv")
            kc, vc = m.kv[li, 0], m.kv[li, 1]
            if m.extras:  # bias, per-head RMSNorm, RoPE and the cache append in the one launch (dec_qk_prep_kv)
                _chk(L.dec_qk_prep_kv(self.qkv.data_ptr(), H, KVH, hd, m.cos.data_ptr(), m.sin.data_ptr(),
                                      self.st.data_ptr(), kc.data_ptr(), vc.data_ptr(), KVH * hd, *m._prep_args(lw), s),
                     "qk_prep_kv")
            else:
                _chk(L.dec_rope_kv(self.qkv.data_ptr(), H, KVH, hd, m.cos.data_ptr(), m.sin.data_ptr(),
                                   self.st.data_ptr(), kc.data_ptr(), vc.data_ptr(), KVH * hd, s), "rope_kv")
            # L = the span the step is captured for (<= 512: one workgroup per head group; else the
            # capacity, sizing the split-L grid); the length itself is read on the device
            _chk(L.dec_attn_decode_ws(self.qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), KVH * hd, span or cfg.n_ctx, H, KVH,
                                      hd, hd ** -0.5, self.attn.data_ptr(), self.st.data_ptr(),
                                      self.attn_ws.data_ptr(), s), "attn_decode")
            gemv(1, self.attn, None, lw["o"], cfg.d, cfg.q_dim, self.xa, self.xb, "gemv o")
            if cfg.experts:
                # four launches where the dense layer has two: router logits (RMSNorm fused), the choice, then
                # the k experts' up|gate and down, each reading the ids the choice left on the device
                E, k, F = cfg.experts, cfg.experts_used, cfg.expert_ffn
                ids, wts, ug, dn = self.moe_ids[li], self.moe_w[li], lw["ug"], lw["down"]
                x, n2, f = self.xb.data_ptr(), lw["n2"].data_ptr(), self.ffn.data_ptr()
                gemv(4, self.xb, lw["n2"], lw["router"], E, cfg.d, None, self.router_logits, "gemv router")
                _chk(L.dec_moe_route(self.router_logits.data_ptr(), E, 1, E, k, ids.data_ptr(), wts.data_ptr(), s),
                     "moe_route")
                if isinstance(ug, Q4Weight):
                    _chk(getattr(L, f"dec_gemv_moe_q{ug.bits}")(x, n2, cfg.eps, ug.q.data_ptr(), ug.sm.data_ptr(), 2 * F,
                                                                cfg.d, ids.data_ptr(), k, E, f, s), "gemv_moe up|gate")
                else:
                    _chk(L.dec_gemv_moe(x, n2, cfg.eps, ug.data_ptr(), 2 * F, cfg.d, ids.data_ptr(), k, E, f, s),
                         "gemv_moe up|gate")
                if isinstance(dn, Q4Weight):
                    _chk(getattr(L, f"dec_gemv_moe_down_q{dn.bits}")(f, dn.q.data_ptr(), dn.sm.data_ptr(), cfg.d, F,
                                                                     ids.data_ptr(), wts.data_ptr(), k, E, x,
                                                                     self.xa.data_ptr(), s), "gemv_moe down")
                else:
                    _chk(L.dec_gemv_moe_down(f, dn.data_ptr(), cfg.d, F, ids.data_ptr(), wts.data_ptr(), k, E, x,
                                             self.xa.data_ptr(), s), "gemv_moe down")
                continue
            gemv(2, self.xb, lw["n2"], lw["ug"], lw["ug"].shape[0], cfg.d, None, self.ffn, "gemv up|gate")
            gemv(1, self.ffn, None, lw["down"], cfg.d, cfg.ffn, self.xb, self.xa, "gemv down")
        gemv(4, self.xa, m.norm_out, m.head, m.head.shape[0], cfg.d, None, self.logits, "gemv head")
        self._sample(self.logits, inc_pos=1)

    def _sample(self, logits: torch.Tensor, inc_pos: int):
        from .nomic import _chk, _stream
        m = self.m
        _chk(m.L.dec_sample_ws(logits.data_ptr(), m.cfg.vocab, self.mask.data_ptr() if self.mask is not None else None,
                               self.top_p, self.temp, self.seed, self.st.data_ptr(), inc_pos, self.host_tok.data_ptr(),
                               self.samp_ws.data_ptr(), _stream()), "sample")

    def _step(self):
        # two captured steps: up to 512 cached keys the single-workgroup attention kernel, past that
        # the split-L one sized for the cache capacity (a split grid costs ~9 us more per layer on
        # short caches: profiles/r2_decode_splits_gqa.jsonl); the host knows the position
        span = self.m.cfg.n_ctx if self.m.pos + 1 > 512 else min(512, self.m.cfg.n_ctx)
        _run_step(self, span)

    def first_token(self, ids: List[int]) -> int:
        """Prefill the prompt (KV cache rows 0..n-1) and sample the first token on the device."""
        m = self.m
        m.reset()
        logits = m.forward(ids)
        self.st[0] = len(ids)
        self.st[1] = 0
        self._sample(logits.contiguous(), inc_pos=0)
        torch.cuda.current_stream().synchronize()
        return int(self.host_tok[0])

    def next_token(self) -> int:
        """One decode step on the device: consume the last sampled token, return the next one."""
        self._step()
        torch.cuda.current_stream().synchronize()
        self.m.pos += 1
        self.steps += 1
        return int(self.host_tok[0])


class BatchDecodeEngine:
    """Up to ``max_seqs`` generations decoded together (csrc/hip/decoder_batch.hip): a decode step
    streams every projection weight once whatever the number of sequences, so one step serves every
    live sequence -- per layer dec_rmsnorm, the qkv small GEMM, dec_rope_kv_b, dec_attn_decode_b, the
    o small GEMM + residual, dec_rmsnorm, the up|gate small GEMM + SwiGLU, the down small GEMM +
    residual; then the final dec_rmsnorm, the head small GEMM and dec_sample_b -- captured once as a
    HIP graph on one stream (two graphs, as DecodeEngine: span <= 512 and span = capacity, picked by
    the longest live sequence).  The launches are always sized for ``max_seqs``; which slots are live
    is device state ({pos, token, step, active, seed} per slot), so ``admit`` and ``release`` never
    recapture.  Each slot draws from its own seed and draw index: a sequence's tokens do not depend on
    what shares its steps.

    ``admit`` prefills the prompt with the eager ``CausalLM.forward`` into the slot's cache between
    two steps; the other sequences wait for its duration.

    ``submit`` + ``prefill(chunk)`` is the batched, chunked admission: ``submit`` only reserves a slot
    on the host (its device record stays inactive, so ``step`` skips it), and one ``prefill`` pass takes
    the next ``min(chunk, remaining)`` prompt tokens of EVERY pending slot through the layers as one
    packed token matrix -- per layer dec_rmsnorm, the qkv GEMM, dec_rope_kv_seg, dec_attn_prefill_kv_seg,
    the o GEMM + residual, dec_rmsnorm, the up|gate GEMM and the down GEMM + residual -- so a weight is
    streamed (and a 4- / 8-bit one dequantised) once per pass, not once per prompt, and a long prompt
    holds the live streams for one chunk at a time.  A prompt that ends in the pass gets the final norm
    and the LM head on its last row, its record, and its first token from dec_sample_b, as ``admit``
    does.  With a fixed ``chunk`` a request's chunk boundaries sit at multiples of ``chunk`` from its own
    start, the two segment kernels never look past a segment, and every GEMM of a pass runs on the
    128 x 128 kernel, whose row results do not depend on the row count or on where a row sits: a
    request's first token, cache rows and later tokens do not depend on what shares its passes.
    Prefill overlapped with the decode step on a second stream is out of scope.

    ``set_prefix(ids, chunk)`` names a prompt prefix many requests share (a system prompt): its first
    R = floor(len / chunk) * chunk tokens' K / V rows are computed once, by the first request that carries
    them (the donor), copied into a compact [layers, 2, R, kvd] buffer, and copied from there into the
    cache of every later carrying request (dec_kv_rows_fanout, one launch per pass for all of them), which
    then starts its prefill at position R.  R is a multiple of the chunk, so such a request runs exactly
    the passes it would have run past R anyway, over cache rows that hold the bits it would have computed:
    no completion changes by a byte.  Only ``submit`` + ``prefill`` use the prefix; the eager ``admit`` path
    and the single-sequence ``DecodeEngine`` always prefill the whole prompt."""

    ST_WORDS = 8

    def __init__(self, model: "CausalLM", max_seqs: int = 8, top_p: float = 0.9, temp: float = 0.7,
                 seed: int = 0xFFFFFFFF, mask: Optional[torch.Tensor] = None, use_graph: bool = True):
        assert model.hip, "BatchDecodeEngine runs on the GPU"
        if not 2 <= max_seqs <= 16:
            raise ValueError(f"max_seqs must be 2..16, not {max_seqs}")
        if model.cfg.experts:
            raise ValueError("the batched decode engine has no mixture-of-experts step (use DecodeEngine)")
        if not model.decode_kernel:
            raise ValueError(f"head dim {model.cfg.head_dim}: the batched decode engine needs a multiple of 64 "
                             "up to 256 (use CausalLM.forward)")
        m, cfg = model, model.cfg
        self.m, self.S = m, int(max_seqs)
        self.top_p, self.temp, self.seed = float(top_p), float(temp), int(seed) & 0xFFFFFFFFFFFFFFFF
        dev, S = m.device, self.S
        kvd = cfg.kv_heads * cfg.head_dim
        need = S * cfg.layers * 2 * cfg.n_ctx * kvd * 2
        free = torch.cuda.mem_get_info(torch.device(dev))[0]
        if need > free:
            raise RuntimeError(f"KV cache for {S} sequences x {cfg.n_ctx} tokens needs {need >> 20} MiB, "
                               f"{free >> 20} MiB of device memory are free: lower max_seqs or the context")
        self.kv = torch.zeros((S, cfg.layers, 2, cfg.n_ctx, cfg.kv_heads, cfg.head_dim), dtype=torch.bfloat16,
                              device=dev)
        z = lambda n, dt=torch.bfloat16: torch.zeros((S, n), dtype=dt, device=dev)  # noqa: E731
        self.xa, self.xb, self.h = z(cfg.d), z(cfg.d), z(cfg.d)
        self.qkv, self.attn, self.ffn = z(cfg.q_dim + 2 * kvd), z(cfg.q_dim), z(cfg.ffn)
        self.logits = z(m.head.shape[0], torch.float32)
        self.st = torch.zeros((S, self.ST_WORDS), dtype=torch.int32, device=dev)
        self.attn_ws = torch.empty(m.L.dec_attn_b_ws_floats(S, cfg.heads, cfg.head_dim), dtype=torch.float32,
                                   device=dev)
        self.samp_ws = torch.empty(m.L.dec_sample_b_ws_floats(S), dtype=torch.float32, device=dev)
        self.host_tok = torch.full((S,), -1, dtype=torch.int32).pin_memory()
        self._rec = torch.zeros(self.ST_WORDS, dtype=torch.int32).pin_memory()
        self.mask = mask[: cfg.vocab].to(device=dev, dtype=torch.uint8).contiguous() if mask is not None else None
        self.use_graph = use_graph
        self.graphs = {}                      # attention span (512 or the capacity) -> captured step
        self.pos: List[Optional[int]] = [None] * S   # host mirror of each live slot's position
        self.steps = 0
        self.pend: Dict[int, list] = {}       # pending slot -> [prompt ids, tokens prefilled, seed, carries prefix]
        self._pf: Optional[dict] = None       # prefill workspaces, sized for S * chunk rows
        self.prefill_passes = 0
        self.prefill_rows = 0                 # packed rows T summed over the passes
        self.prefix_hits = 0                  # requests that started from the captured prefix rows
        self.prefix_rows_reused = 0           # R per hit
        self._pfx_ids: Optional[List[int]] = None     # the kept ids[:R]; None: no prefix set
        self._pfx_chunk = 0
        self._pfx_buf: Optional[torch.Tensor] = None  # [layers, 2, R, kvd]
        self._pfx_ready = False               # the buffer holds the rows (a donor reached R)
        self._pfx_donor: Optional[int] = None

    # ---------------------------------------------------------------- slots --
    def active(self) -> List[int]:
        return [b for b, p in enumerate(self.pos) if p is not None]

    def _write_state(self, slot: int, words: List[int]):
        for i, w in enumerate(words):
            w &= 0xFFFFFFFF
            self._rec[i] = w - (1 << 32) if w >= 1 << 31 else w
        self.st[slot].copy_(self._rec, non_blocking=True)
        torch.cuda.current_stream().synchronize()  # _rec is reused by the next write

    def _free_slot(self, ids: List[int]) -> int:
        """The lowest slot that is neither live nor pending, for a prompt that fits the context."""
        free = [b for b, p in enumerate(self.pos) if p is None and b not in self.pend]
        if not free:
            raise RuntimeError(f"all {self.S} sequence slots are in use")
        if not ids or len(ids) >= self.m.cfg.n_ctx:
            raise ValueError(f"a prompt of {len(ids)} tokens leaves no room in a context of {self.m.cfg.n_ctx}")
        return free[0]

    def _seed(self, seed: Optional[int]) -> int:
        return self.seed if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF

    def _first_token(self, slot: int, n: int, sd: int, logits: torch.Tensor):
        """A prefilled prompt of n tokens goes live: its record, its logits row, its first draw (enqueued)."""
        self._write_state(slot, [n, 0, 0, 1, sd & 0xFFFFFFFF, sd >> 32, 0, 0])
        self.logits[slot, : self.m.cfg.vocab].copy_(logits)
        self._sample(slot, 1, inc_pos=0)

    def admit(self, ids: List[int], seed: Optional[int] = None):
        """Prefill ``ids`` into a free slot and sample its first token: (slot, first_token)."""
        m = self.m
        slot = self._free_slot(ids)
        saved = (m.kv, m.pos)
        m.kv, m.pos = self.kv[slot], 0  # the eager forward appends to whatever cache the model points at
        try:
            logits = m.forward(ids)
        finally:
            m.kv, m.pos = saved
        self._first_token(slot, len(ids), self._seed(seed), logits)
        torch.cuda.current_stream().synchronize()
        self.pos[slot] = len(ids)
        return slot, int(self.host_tok[slot])

    def release(self, slot: int):
        """Retire a sequence: the slot is skipped by every later step until it is admitted again."""
        if slot in self.pend:  # a pending prompt is cancelled: its record was never active
            del self.pend[slot]
            if slot == self._pfx_donor:  # the next pass picks the lowest carrying slot, from its offset 0
                self._pfx_donor = None
            return
        if self.pos[slot] is None:
            raise ValueError(f"slot {slot} is not in use")
        self._write_state(slot, [0] * self.ST_WORDS)
        self.pos[slot] = None

    def set_token(self, slot: int, tok: int):
        """Replace the token the slot's next step consumes (teacher forcing)."""
        self.st[slot, 1] = int(tok)

    # -------------------------------------------------------------- prefill --
    PF_ROWS = 128  # row multiple of the MFMA GEMM's A operand (nomic_api.h)

    def pending(self) -> List[int]:
        """Slots reserved by ``submit`` whose prompt is not fully prefilled yet."""
        return sorted(self.pend)

    def submit(self, ids: List[int], seed: Optional[int] = None) -> int:
        """Reserve a free slot for ``ids`` (host only: the slot's device record stays inactive until its
        prompt is prefilled, so ``step`` skips it) and return it; ``prefill`` does the work."""
        m = self.m
        if not m.prefill_kernel:
            raise ValueError(f"head dim {m.cfg.head_dim}: the batched prefill needs 64 or 128 (use admit)")
        slot = self._free_slot(ids)
        ids = list(ids)
        R = len(self._pfx_ids or ())
        # carrying is all or nothing: the whole kept prefix, and at least one token of the request's own
        self.pend[slot] = [ids, 0, self._seed(seed), R > 0 and len(ids) > R and ids[:R] == self._pfx_ids]
        return slot

    def set_prefix(self, ids: Optional[List[int]], chunk: int) -> int:
        """Name the prompt prefix that requests share and return R = (len(ids) // chunk) * chunk, the tokens
        whose cache rows are reused (0: nothing is).  A new prefix drops the captured rows; the next request
        that carries it computes them again.  ``set_prefix(None, 0)`` turns the reuse off and frees the buffer.
        RuntimeError while a request is pending: change the prefix between two admission waves."""
        if self.pend:
            raise RuntimeError(f"set_prefix with {len(self.pend)} pending request(s): wait until pending() is empty")
        self._pfx_ids, self._pfx_chunk, self._pfx_buf = None, 0, None
        self._pfx_ready, self._pfx_donor = False, None
        if ids is None:
            return 0
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, not {chunk}")
        cfg = self.m.cfg
        R = len(ids) // chunk * chunk
        if R >= cfg.n_ctx:
            raise ValueError(f"a prefix of {R} tokens leaves no room in a context of {cfg.n_ctx}")
        if R > 0:
            kvd = cfg.kv_heads * cfg.head_dim
            need = cfg.layers * 2 * R * kvd * 2
            free = torch.cuda.mem_get_info(torch.device(self.m.device))[0]
            if need > free:
                raise RuntimeError(f"prefix rows for {R} tokens need {need >> 20} MiB, {free >> 20} MiB of device "
                                   "memory are free: shorten the prefix")
            self._pfx_buf = torch.zeros((cfg.layers, 2, R, kvd), dtype=torch.bfloat16, device=self.m.device)
        self._pfx_ids, self._pfx_chunk = [int(t) for t in ids[:R]], chunk
        return R

    def _fanout(self, src: torch.Tensor, src_rows: int, dst: torch.Tensor, dst_rows: int, seq_stride: int,
                slots: List[int], nslots: int, rows: int):
        """rows [0, rows) of every (layer, k | v) plane: src [layers, 2, src_rows, ..] -> dst [.., layers, 2,
        dst_rows, ..] of each listed slot, one launch on the current stream."""
        from .nomic import _chk, _stream
        cfg = self.m.cfg
        kvd = cfg.kv_heads * cfg.head_dim
        tb = np.ascontiguousarray(np.array(slots, dtype=np.int32))  # host array, read at launch
        _chk(self.m.L.dec_kv_rows_fanout(src.data_ptr(), src_rows * kvd, src_rows, dst.data_ptr(), dst_rows * kvd,
                                         seq_stride, tb.ctypes.data, len(slots), nslots, dst_rows, 2 * cfg.layers,
                                         rows, kvd, _stream()), "kv_rows_fanout")

    def _prefill_ws(self, chunk: int) -> dict:
        """The pass's workspaces for S * chunk packed rows, allocated once (again only for a larger chunk)."""
        rows = (self.S * chunk + self.PF_ROWS - 1) // self.PF_ROWS * self.PF_ROWS
        w = self._pf
        if w is not None and w["rows"] >= rows:
            return w
        cfg, dev = self.m.cfg, self.m.device
        kvd = cfg.kv_heads * cfg.head_dim
        z = lambda r, n, dt=torch.bfloat16: torch.zeros((r, n), dtype=dt, device=dev)  # noqa: E731
        w = {"rows": rows, "x": z(rows, cfg.d), "xb": z(rows, cfg.d), "h": z(rows, cfg.d),
             "qkv": z(rows, cfg.q_dim + 2 * kvd), "attn": z(rows, cfg.q_dim), "ffn": z(rows, cfg.ffn),
             "last": z(self.PF_ROWS, cfg.d), "hl": z(self.PF_ROWS, cfg.d),
             "lg": z(self.PF_ROWS, self.m.head.shape[0], torch.float32),
             "ids": torch.zeros(rows, dtype=torch.int64, device=dev),
             "ids_host": torch.zeros(rows, dtype=torch.int64).pin_memory(),
             "sel": torch.zeros(self.S, dtype=torch.int64, device=dev),
             "sel_host": torch.zeros(self.S, dtype=torch.int64).pin_memory()}
        self._pf = w
        return w

    def _pf_mm(self, mode, x, M, w, res, out, what):
        """out[:M] = epilogue(x[:M] @ w^T) on nomic_gemm; x / res / out are workspace row blocks."""
        from .nomic import _chk, _stream
        wd = self.m._dense(w)
        N, K = wd.shape
        rp, ldr = (res.data_ptr(), res.stride(0)) if res is not None else (None, 0)
        _chk(self.m.L.nomic_gemm(mode, x.data_ptr(), x.stride(0), wd.data_ptr(), K, M, N, K, out.data_ptr(),
                                 out.stride(0), rp, ldr, None, None, 0, _stream()), what)

    def _prefix_plan(self):
        """What the shared prefix asks of the next pass, from host state alone: (hits, donor, held).  Once the
        rows are captured, a carrying request still at offset 0 starts from copied rows (a hit).  Until then one
        carrying request (the donor) computes them and the others wait at offset 0 (held).  The donor stays the
        donor while it is pending (a request submitted into a lower slot meanwhile is held like the rest); after
        its release the lowest carrying slot takes over, from its own offset 0."""
        carrying = [b for b in sorted(self.pend) if self.pend[b][3]] if self._pfx_ids else []
        if self._pfx_ready:
            return [b for b in carrying if self.pend[b][1] == 0], None, []
        if not carrying:
            return [], None, []
        if self._pfx_donor not in carrying:
            self._pfx_donor = carrying[0]
        return [], self._pfx_donor, [b for b in carrying if b != self._pfx_donor]

    @torch.no_grad()
    def prefill(self, chunk: int) -> Dict[int, int]:
        """ONE pass over the next ``min(chunk, remaining)`` prompt tokens of every pending slot (at most
        S * chunk packed rows): {slot: first token} for the prompts that end in this pass, which are live
        from here on.  Call it until ``pending()`` is empty; between two passes the live slots may ``step``."""
        from .nomic import _chk, _stream
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, not {chunk}")
        R = len(self._pfx_ids or ())
        if R and chunk != self._pfx_chunk:
            raise ValueError(f"chunk {chunk} under a prefix set for chunk {self._pfx_chunk}: reuse stops at a "
                             "multiple of the chunk so that a request's passes do not move")
        if not self.pend:
            return {}
        m, cfg, L, S = self.m, self.m.cfg, self.m.L, self.S
        H, KVH, hd = cfg.heads, cfg.kv_heads, cfg.head_dim
        w = self._prefill_ws(chunk)
        hits, donor, held = self._prefix_plan()
        if hits:  # one launch for every such slot of the pass, ahead of its first kernel
            self._fanout(self._pfx_buf, R, self.kv, cfg.n_ctx, self.kv.stride(0), hits, S, R)
            for b in hits:
                self.pend[b][1] = R
            self.prefix_hits += len(hits)
            self.prefix_rows_reused += R * len(hits)
        # pack: the next chunk of every pending slot that is not held, as one token matrix
        segs, toks, ends = [], [], []
        for slot in sorted(self.pend):
            if slot in held:
                continue
            ids, off = self.pend[slot][:2]
            n = min(chunk, len(ids) - off)
            if off + n == len(ids):
                ends.append((slot, len(toks) + n - 1))
            segs.append((len(toks), n, off, slot))
            toks += ids[off: off + n]
        T = len(toks)
        Tp = (T + self.PF_ROWS - 1) // self.PF_ROWS * self.PF_ROWS
        table = np.ascontiguousarray(np.array(segs, dtype=np.int32))  # host {row0, n, pos0, slot}, read at launch
        tp, ns = table.ctypes.data, len(segs)
        s = _stream()
        x, xb, h, qkv, attn, ffn = w["x"], w["xb"], w["h"], w["qkv"], w["attn"], w["ffn"]
        w["ids_host"][:T] = torch.tensor(toks, dtype=torch.int64)
        w["ids"][:T].copy_(w["ids_host"][:T], non_blocking=True)
        torch.index_select(m.emb, 0, w["ids"][:T], out=x[:T])  # packed once ...
        x[T:Tp].zero_()                                         # ... and padded once, to the GEMM's row multiple

        def rms(src, wt, dst, rows):
            _chk(L.dec_rmsnorm(src.data_ptr(), src.stride(0), wt.data_ptr(), rows, cfg.d, cfg.eps, dst.data_ptr(),
                               dst.stride(0), s), "rmsnorm")

        # one GEMM kernel for every pass: the automatic choice moves with the rows of a pass, and a request's
        # bits must not (the 128 x 128 kernel's row results depend on neither M nor the row's place)
        prev = L.nomic_gemm_set_variant(128)
        try:
            for li, lw in enumerate(m.layers):
                rms(x, lw["n1"], h, T)
                self._pf_mm(0, h, T, lw["qkv"], None, qkv, "gemm qkv")
                kc, vc = self.kv[0, li, 0], self.kv[0, li, 1]
                if m.extras:
                    _chk(L.dec_qk_prep_kv_seg(qkv.data_ptr(), qkv.stride(0), T, tp, ns, H, KVH, hd, m.cos.data_ptr(),
                                              m.sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), KVH * hd,
                                              self.kv.stride(0), S, cfg.n_ctx, *m._prep_args(lw), s), "qk_prep_kv_seg")
                else:
                    _chk(L.dec_rope_kv_seg(qkv.data_ptr(), qkv.stride(0), T, tp, ns, H, KVH, hd, m.cos.data_ptr(),
                                           m.sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), KVH * hd,
                                           self.kv.stride(0), S, cfg.n_ctx, s), "rope_kv_seg")
                _chk(L.dec_attn_prefill_kv_seg(qkv.data_ptr(), qkv.stride(0), T, tp, ns, kc.data_ptr(), vc.data_ptr(),
                                               KVH * hd, self.kv.stride(0), S, cfg.n_ctx, H, KVH, hd, hd ** -0.5,
                                               attn.data_ptr(), attn.stride(0), s), "attn_prefill_kv_seg")
                self._pf_mm(1, attn, T, lw["o"], x, xb, "gemm o")
                rms(xb, lw["n2"], h, T)
                self._pf_mm(2, h, T, lw["ug"], None, ffn, "gemm up|gate")
                self._pf_mm(1, ffn, T, lw["down"], xb, x, "gemm down")
            if ends:  # only the last rows of the prompts that end here see the final norm and the LM head
                k = len(ends)
                w["sel_host"][:k] = torch.tensor([r for _, r in ends], dtype=torch.int64)
                w["sel"][:k].copy_(w["sel_host"][:k], non_blocking=True)
                torch.index_select(x, 0, w["sel"][:k], out=w["last"][:k])
                rms(w["last"], m.norm_out, w["hl"], k)
                self._pf_mm(4, w["hl"], k, m.head, None, w["lg"], "gemm head")
        finally:
            L.nomic_gemm_set_variant(prev)
        # finish: offsets, the donor's rows, and the prompts that ended go live
        for _, n, _, slot in segs:
            self.pend[slot][1] += n
        if donor is not None and self.pend[donor][1] >= R:
            # the donor's rows [0, R) are final: keep them (its cache -> the buffer, behind the pass on the same
            # stream); the prefix counts as captured from the next pass on
            self._fanout(self.kv[donor], cfg.n_ctx, self._pfx_buf, R, 0, [0], 1, R)
            self._pfx_ready, self._pfx_donor = True, None
        out = {}
        for i, (slot, _) in enumerate(ends):
            ids, _, sd = self.pend[slot][:3]
            self._first_token(slot, len(ids), sd, w["lg"][i, : cfg.vocab])
        torch.cuda.current_stream().synchronize()
        for slot, _ in ends:
            self.pos[slot] = len(self.pend.pop(slot)[0])
            out[slot] = int(self.host_tok[slot])
        self.prefill_passes += 1
        self.prefill_rows += T
        return out

    # ----------------------------------------------------------------- step --
    def _sample(self, slot0: int, n: int, inc_pos: int):
        from .nomic import _chk, _stream
        m, lg = self.m, self.logits
        _chk(m.L.dec_sample_b(lg[slot0].data_ptr(), lg.stride(0), n, m.cfg.vocab,
                              self.mask.data_ptr() if self.mask is not None else None, self.top_p, self.temp,
                              self.st[slot0].data_ptr(), inc_pos, self.host_tok[slot0:].data_ptr(),
                              self.samp_ws[slot0 * (self.samp_ws.numel() // self.S):].data_ptr(), _stream()), "sample_b")

    def _mm(self, mode, x, w, N, K, res, out, what):
        from .nomic import _chk, _stream
        L, S = self.m.L, self.S
        rp, ldr = (res.data_ptr(), res.stride(0)) if res is not None else (None, 0)
        if isinstance(w, Q4Weight):
            fn = L.dec_gemm_small_q8 if w.bits == 8 else L.dec_gemm_small_q4
            rc = fn(mode, x.data_ptr(), x.stride(0), S, w.q.data_ptr(), w.sm.data_ptr(), N, K, rp, ldr,
                    out.data_ptr(), out.stride(0), _stream())
        else:
            rc = L.dec_gemm_small(mode, x.data_ptr(), x.stride(0), S, w.data_ptr(), N, K, rp, ldr, out.data_ptr(),
                                  out.stride(0), _stream())
        _chk(rc, what)

    def _enqueue_step(self, span: int):
        from .nomic import _chk, _stream
        m, cfg, L, S = self.m, self.m.cfg, self.m.L, self.S
        s = _stream()
        H, KVH, hd = cfg.heads, cfg.kv_heads, cfg.head_dim
        st = self.st.data_ptr()

        def rms(x, w, out):
            _chk(L.dec_rmsnorm(x.data_ptr(), x.stride(0), w.data_ptr(), S, cfg.d, cfg.eps, out.data_ptr(),
                               out.stride(0), s), "rmsnorm")

        _chk(L.dec_embed_tok_b(m.emb.data_ptr(), cfg.d, st, S, self.xa.data_ptr(), self.xa.stride(0), s), "embed_tok_b")
        for li, lw in enumerate(m.layers):
            rms(self.xa, lw["n1"], self.h)
            self._mm(0, self.h, lw["qkv"], lw["qkv"].shape[0], cfg.d, None, self.qkv, "gemm qkv")
            kc, vc = self.kv[0, li, 0], self.kv[0, li, 1]
            if m.extras:
                _chk(L.dec_qk_prep_kv_b(self.qkv.data_ptr(), self.qkv.stride(0), S, H, KVH, hd, m.cos.data_ptr(),
                                        m.sin.data_ptr(), st, kc.data_ptr(), vc.data_ptr(), KVH * hd,
                                        self.kv.stride(0), *m._prep_args(lw), s), "qk_prep_kv_b")
            else:
                _chk(L.dec_rope_kv_b(self.qkv.data_ptr(), self.qkv.stride(0), S, H, KVH, hd, m.cos.data_ptr(),
                                     m.sin.data_ptr(), st, kc.data_ptr(), vc.data_ptr(), KVH * hd, self.kv.stride(0),
                                     s), "rope_kv_b")
            _chk(L.dec_attn_decode_b(self.qkv.data_ptr(), self.qkv.stride(0), kc.data_ptr(), vc.data_ptr(), KVH * hd,
                                     self.kv.stride(0), span, S, H, KVH, hd, hd ** -0.5, self.attn.data_ptr(),
                                     self.attn.stride(0), st, self.attn_ws.data_ptr(), s), "attn_decode_b")
            self._mm(1, self.attn, lw["o"], cfg.d, cfg.q_dim, self.xa, self.xb, "gemm o")
            rms(self.xb, lw["n2"], self.h)
            self._mm(2, self.h, lw["ug"], lw["ug"].shape[0], cfg.d, None, self.ffn, "gemm up|gate")
            self._mm(1, self.ffn, lw["down"], cfg.d, cfg.ffn, self.xb, self.xa, "gemm down")
        rms(self.xa, m.norm_out, self.h)
        self._mm(4, self.h, m.head, m.head.shape[0], cfg.d, None, self.logits, "gemm head")
        self._sample(0, S, inc_pos=1)

    def step(self) -> Dict[int, int]:
        """One decode step for every live slot: {slot: sampled token}."""
        live = self.active()
        if not live:
            return {}
        n_ctx = self.m.cfg.n_ctx
        for b in live:
            if self.pos[b] >= n_ctx:
                raise ValueError(f"slot {b}: context window of {n_ctx} tokens exceeded")
        span = n_ctx if max(self.pos[b] for b in live) + 1 > 512 else min(512, n_ctx)
        _run_step(self, span)
        torch.cuda.current_stream().synchronize()
        self.steps += 1
        out = {}
        for b in live:
            self.pos[b] += 1
            out[b] = int(self.host_tok[b])
        return out


class Sampler:
    """top-p 0.9 -> temperature 0.7 -> seeded categorical (reference :272-279)."""

    def __init__(self, top_p: float = 0.9, temp: float = 0.7, seed: int = 0xFFFFFFFF, mask=None):
        self.top_p, self.temp, self.seed = top_p, temp, seed
        self.g = torch.Generator().manual_seed(seed)
        self.mask = mask

    def __call__(self, logits: torch.Tensor) -> int:
        lg = logits.detach().float().cpu()
        if self.mask is not None:
            lg = lg.masked_fill(~self.mask[: lg.shape[0]], -math.inf)
        p = torch.softmax(lg, -1)
        sp, si = torch.sort(p, descending=True)
        keep = torch.cumsum(sp, 0) - sp < self.top_p
        keep[0] = True
        lg2 = torch.full_like(lg, -math.inf)
        lg2[si[keep]] = lg[si[keep]]
        probs = torch.softmax(lg2 / self.temp, -1)
        return int(torch.multinomial(probs, 1, generator=self.g).item())
