"""The fused q/k preparation step (csrc/hip/decoder_arch.hip: dec_qk_prep, dec_qk_prep_kv, dec_qk_prep_kv_b,
dec_qk_prep_kv_seg) and the qwen2 / qwen3 models that run on it: kernel numerics against fp64, the bit
identity of the four forms, what they must not write, their refusals, and the models end to end -- eager
forward against the fp64 reference of tests/decoder_arch_ref.py, DecodeEngine and BatchDecodeEngine against
the eager forward, batch independence and the prefix cache on the new path."""
import functools

import pytest

import decoder_arch_ref as R

pytestmark = pytest.mark.gpu

N_CTX, BASE, EPS = 256, 1e6, 1e-6
INVALID = 1  # hipErrorInvalidValue
SENT = 7.0


@functools.lru_cache(maxsize=None)
def _lib():
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig
    return CausalLM.random(DecoderConfig(layers=1), seed=1, device="cuda").L


@functools.lru_cache(maxsize=None)
def _tables(hd):
    import torch
    inv = 1.0 / (BASE ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    ang = torch.arange(N_CTX, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float().cuda(), ang.sin().float().cuda()


def _extras(H, KVH, hd, bias, norm, seed=5):
    """(bias, qn, kn) fp32 device tensors or None: biases ~ 0.5, norm weights 1 + noise."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    b = 0.5 * torch.randn((H + 2 * KVH) * hd, device="cuda", generator=g) if bias else None
    qn = 1.0 + 0.1 * torch.randn(hd, device="cuda", generator=g) if norm else None
    kn = 1.0 + 0.1 * torch.randn(hd, device="cuda", generator=g) if norm else None
    return b, qn, kn


def _p(t):
    return t.data_ptr() if t is not None else None


def _ref_rows(x, pos, H, KVH, hd, ex):
    """fp64 reference of rows x [T, (H + 2 KVH) hd] (bf16 values) at positions pos [T]."""
    import torch
    b, qn, kn = ex
    cs, sn = _tables(hd)
    T = x.shape[0]
    y = x.double() + (b.double() if b is not None else 0.0)
    qk = y[:, : (H + KVH) * hd].reshape(T, H + KVH, hd)
    if qn is not None:
        w = torch.cat([qn.double().expand(H, hd), kn.double().expand(KVH, hd)])
        qk = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + EPS) * w
    c, s = cs[pos].double()[:, None, :], sn[pos].double()[:, None, :]
    a0, a1 = qk[..., 0::2], qk[..., 1::2]
    rot = torch.stack([a0 * c - a1 * s, a0 * s + a1 * c], -1).flatten(-2).reshape(T, -1)
    return torch.cat([rot, y[:, (H + KVH) * hd:]], 1)


def _prep(L, qkv, T, H, KVH, hd, pos0, ex, eps=EPS):
    cs, sn = _tables(hd if hd in (64, 128) else 64)
    return L.dec_qk_prep(qkv.data_ptr(), qkv.stride(0), T, H, KVH, hd, pos0, cs.data_ptr(), sn.data_ptr(), _p(ex[0]),
                         _p(ex[1]), _p(ex[2]), eps, None)


@pytest.mark.parametrize("H,KVH", [(14, 2), (4, 4)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("bias,norm", [(True, False), (False, True), (True, True)])
def test_qk_prep_against_fp64(bias, norm, hd, H, KVH):
    """dec_qk_prep on 1 and 131 rows at positions 0, 1 and n_ctx - 1: every element within
    2^-8 |ref| + 1e-5 max|ref| of the fp64 result on the bf16 inputs.  The relative term is what ONE
    round-to-nearest to bf16 (8 significant bits) can cost, so a second rounding anywhere would miss it; the
    absolute term covers the fp32 arithmetic ahead of it, the sum over hd squares and results near zero
    crossings.  Measured: the worst element sits at 0.99 of its bound.  The pad columns keep their sentinel."""
    import torch
    L = _lib()
    W = (H + 2 * KVH) * hd
    ex = _extras(H, KVH, hd, bias, norm)
    g = torch.Generator(device="cuda").manual_seed(hd + H)
    for T, pos0 in ((1, 0), (1, 1), (1, N_CTX - 1), (131, 0), (131, 1), (131, N_CTX - 131)):
        qkv = torch.full((T, W + 8), SENT, device="cuda", dtype=torch.bfloat16)
        qkv[:, :W] = torch.randn((T, W), device="cuda", generator=g).to(torch.bfloat16)
        x0 = qkv[:, :W].clone()
        assert _prep(L, qkv, T, H, KVH, hd, pos0, ex) == 0
        torch.cuda.synchronize()
        ref = _ref_rows(x0, torch.arange(pos0, pos0 + T, device="cuda"), H, KVH, hd, ex)
        err = (qkv[:, :W].double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max()
        worst = (err / bound).max().item()
        print(f"qk_prep bias={bias} norm={norm} hd={hd} H={H} KVH={KVH} T={T} pos0={pos0}: max err/bound {worst:.3f}")
        assert bool((err <= bound).all()), (T, pos0, worst)
        assert bool((qkv[:, W:] == SENT).all())
        if not bias:  # v has nothing to add: not a bit of it moves
            assert torch.equal(qkv[:, (H + KVH) * hd: W], x0[:, (H + KVH) * hd:])


def _state(rows):
    """int32 [n, 8] slot records from (pos, token, step, active)."""
    import torch
    return torch.tensor([[p, t, s, a, 0, 0, 0, 0] for p, t, s, a in rows], dtype=torch.int32, device="cuda")


SEGS = [(0, 1, 7, 2), (1, 3, 50, 0), (4, 130, 100, 4)]  # {row0, n, pos0, slot}
ROWS, NSLOT = 140, 5  # rows 134 .. 139 belong to no segment; slots 1 and 3 get nothing


def _seg_call(L, qkv, segs, H, KVH, hd, kv, ex, T=None):
    import numpy as np
    cs, sn = _tables(hd)
    tb = np.ascontiguousarray(np.array(segs, dtype=np.int32))
    return L.dec_qk_prep_kv_seg(qkv.data_ptr(), qkv.stride(0), qkv.shape[0] if T is None else T, tb.ctypes.data,
                                len(segs), H, KVH, hd, cs.data_ptr(), sn.data_ptr(), kv[0, 0].data_ptr(),
                                kv[0, 1].data_ptr(), KVH * hd, kv.stride(0), kv.shape[0], N_CTX, _p(ex[0]), _p(ex[1]),
                                _p(ex[2]), EPS, None)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("bias,norm", [(True, False), (False, True), (True, True)])
def test_four_forms_leave_the_same_bits_and_write_nothing_else(bias, norm, hd):
    """One random qkv matrix through dec_qk_prep + slice copies, dec_qk_prep_kv row by row, dec_qk_prep_kv_seg
    (segments of 1, 3 and 130 rows at non-zero positions) and dec_qk_prep_kv_b (5 slots, 1 and 3 inactive):
    equal bits in the q rows and the cache rows; rows outside the segments, the pad columns, inactive slots,
    every other cache row and -- for the _kv forms -- the k / v columns of qkv keep what they held."""
    import torch
    L = _lib()
    H, KVH = 14, 2
    qd, kvd = H * hd, KVH * hd
    W = qd + 2 * kvd
    ex = _extras(H, KVH, hd, bias, norm)
    cs, sn = _tables(hd)
    g = torch.Generator(device="cuda").manual_seed(99 + hd)
    qkv0 = torch.full((ROWS, W + 8), SENT, device="cuda", dtype=torch.bfloat16)
    qkv0[:, :W] = torch.randn((ROWS, W), device="cuda", generator=g).to(torch.bfloat16)
    fresh_kv = lambda: torch.full((NSLOT, 2, N_CTX, kvd), SENT, device="cuda", dtype=torch.bfloat16)  # noqa: E731

    # form 1: in place per segment, then the slice copies of CausalLM.forward
    q1, kv1 = qkv0.clone(), fresh_kv()
    for row0, n, pos0, slot in SEGS:
        assert _prep(L, q1[row0:], n, H, KVH, hd, pos0, ex) == 0
        kv1[slot, 0, pos0: pos0 + n] = q1[row0: row0 + n, qd: qd + kvd]
        kv1[slot, 1, pos0: pos0 + n] = q1[row0: row0 + n, qd + kvd: W]
    torch.cuda.synchronize()
    assert torch.equal(q1[134:], qkv0[134:]) and bool((q1[:, W:] == SENT).all())
    assert not torch.equal(q1[:134, :W], qkv0[:134, :W])

    # form 2: one row at a time at the position of a device state word
    q2, kv2 = qkv0.clone(), fresh_kv()
    where = [(row0 + r, pos0 + r, slot) for row0, n, pos0, slot in SEGS for r in range(n)]
    st = _state([(p, 0, 0, 1) for _, p, _ in where])
    for i, (row, _, slot) in enumerate(where):
        assert L.dec_qk_prep_kv(q2[row].data_ptr(), H, KVH, hd, cs.data_ptr(), sn.data_ptr(), st[i].data_ptr(),
                                kv2[slot, 0].data_ptr(), kv2[slot, 1].data_ptr(), kvd, _p(ex[0]), _p(ex[1]), _p(ex[2]),
                                EPS, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(q2[:, :qd], q1[:, :qd]) and torch.equal(kv2, kv1)
    assert torch.equal(q2[:, qd:], qkv0[:, qd:])  # k / v columns, pad columns, rows past the segments

    # form 4: the by-value segment table, one launch
    q4, kv4 = qkv0.clone(), fresh_kv()
    assert _seg_call(L, q4, SEGS, H, KVH, hd, kv4, ex) == 0
    torch.cuda.synchronize()
    assert torch.equal(q4[:, :qd], q1[:, :qd]) and torch.equal(kv4, kv1)
    assert torch.equal(q4[:, qd:], qkv0[:, qd:])

    # form 3: one row per slot, slots 1 and 3 inactive, each active slot at its own position
    pick = {0: (2, 51), 2: (0, 7), 4: (81, 177)}  # slot -> (row of the matrix, its position)
    qb = torch.full((NSLOT, W + 8), SENT, device="cuda", dtype=torch.bfloat16)
    for slot, (row, _) in pick.items():
        qb[slot] = qkv0[row]
    qb0, kvb = qb.clone(), fresh_kv()
    stb = _state([(pick[b][1], 0, 0, 1) if b in pick else (9, 0, 0, 0) for b in range(NSLOT)])
    stb0 = stb.clone()
    assert L.dec_qk_prep_kv_b(qb.data_ptr(), qb.stride(0), NSLOT, H, KVH, hd, cs.data_ptr(), sn.data_ptr(),
                              stb.data_ptr(), kvb[0, 0].data_ptr(), kvb[0, 1].data_ptr(), kvd, kvb.stride(0), _p(ex[0]),
                              _p(ex[1]), _p(ex[2]), EPS, None) == 0
    torch.cuda.synchronize()
    want = fresh_kv()
    for slot, (row, pos) in pick.items():
        want[slot, :, pos] = kv1[slot, :, pos]
        assert torch.equal(qb[slot, :qd], q1[row, :qd])
    assert torch.equal(kvb, want) and torch.equal(qb[:, qd:], qb0[:, qd:]) and torch.equal(stb, stb0)
    assert torch.equal(qb[1], qb0[1]) and torch.equal(qb[3], qb0[3])


def test_bad_arguments_are_refused_before_any_launch():
    """Neither flag, head dim 96, a misaligned pointer, an overlapping segment table (and a few more): every
    call returns hipErrorInvalidValue and the sentinel-filled outputs keep every bit."""
    import torch
    L = _lib()
    H, KVH, hd = 4, 2, 64
    qd, kvd = H * hd, KVH * hd
    W = qd + 2 * kvd
    cs, sn = _tables(hd)
    ex = _extras(H, KVH, hd, True, True)
    none = (None, None, None)
    qkv = torch.full((8, W + 8), SENT, device="cuda", dtype=torch.bfloat16)
    kv = torch.full((NSLOT, 2, N_CTX, kvd), SENT, device="cuda", dtype=torch.bfloat16)
    st = _state([(3, 0, 0, 1)] * NSLOT)
    P = lambda e: (_p(e[0]), _p(e[1]), _p(e[2]), EPS, None)  # noqa: E731

    def kv1(q=None, hd_=hd, e=ex, kc=None):
        return L.dec_qk_prep_kv(q or qkv.data_ptr(), H, KVH, hd_, cs.data_ptr(), sn.data_ptr(), st.data_ptr(),
                                kc or kv[0, 0].data_ptr(), kv[0, 1].data_ptr(), kvd, *P(e))

    def kvb(q=None, hd_=hd, e=ex, n=NSLOT):
        return L.dec_qk_prep_kv_b(q or qkv.data_ptr(), qkv.stride(0), n, H, KVH, hd_, cs.data_ptr(), sn.data_ptr(),
                                  st.data_ptr(), kv[0, 0].data_ptr(), kv[0, 1].data_ptr(), kvd, kv.stride(0), *P(e))

    bad = {
        "prep: neither flag": _prep(L, qkv, 8, H, KVH, hd, 0, none),
        "prep: hd 96": _prep(L, qkv, 8, H, KVH, 96, 0, ex),
        "prep: misaligned qkv": L.dec_qk_prep(qkv.data_ptr() + 2, qkv.stride(0), 4, H, KVH, hd, 0, cs.data_ptr(),
                                              sn.data_ptr(), *P(ex)),
        "prep: one norm weight": _prep(L, qkv, 8, H, KVH, hd, 0, (None, ex[1], None)),
        "prep: misaligned bias": L.dec_qk_prep(qkv.data_ptr(), qkv.stride(0), 4, H, KVH, hd, 0, cs.data_ptr(),
                                               sn.data_ptr(), ex[0].data_ptr() + 4, None, None, EPS, None),
        "prep: negative position": _prep(L, qkv, 8, H, KVH, hd, -1, ex),
        "kv: neither flag": kv1(e=none),
        "kv: hd 96": kv1(hd_=96),
        "kv: misaligned qkv": kv1(q=qkv.data_ptr() + 2),
        "kv: misaligned cache": kv1(kc=kv[0, 0].data_ptr() + 2),
        "kv_b: neither flag": kvb(e=none),
        "kv_b: hd 96": kvb(hd_=96),
        "kv_b: misaligned qkv": kvb(q=qkv.data_ptr() + 2),
        "kv_b: 17 slots": kvb(n=17),
        "seg: neither flag": _seg_call(L, qkv, [(0, 2, 0, 0)], H, KVH, hd, kv, none),
        "seg: hd 96": _seg_call(L, qkv, [(0, 2, 0, 0)], H, KVH, 96, kv, ex),
        "seg: overlapping rows": _seg_call(L, qkv, [(0, 3, 0, 0), (2, 2, 0, 1)], H, KVH, hd, kv, ex),
        "seg: one slot twice": _seg_call(L, qkv, [(0, 2, 0, 1), (2, 2, 9, 1)], H, KVH, hd, kv, ex),
        "seg: rows past T": _seg_call(L, qkv, [(6, 3, 0, 0)], H, KVH, hd, kv, ex),
        "seg: past n_ctx": _seg_call(L, qkv, [(0, 2, N_CTX - 1, 0)], H, KVH, hd, kv, ex),
        "seg: slot 5 of 5": _seg_call(L, qkv, [(0, 2, 0, NSLOT)], H, KVH, hd, kv, ex),
        "seg: empty table": _seg_call(L, qkv, [], H, KVH, hd, kv, ex),
    }
    torch.cuda.synchronize()
    for what, rc in bad.items():
        assert rc == INVALID, (what, rc)
    assert bool((qkv == SENT).all()) and bool((kv == SENT).all())


# ------------------------------------------------------------------------------------------ the models --
MODELS = {
    "qwen2": R.spec("qwen2", d=896, H=14, KVH=2, hd=64, ffn=512, n_ctx=128, bias=True, rope_base=1e6, seed=21),
    "qwen3": R.spec("qwen3", d=256, H=4, KVH=2, hd=128, ffn=512, n_ctx=128, norm=True, rope_base=1e6, seed=22),
}
MODELS["qwen2"]["key_length"] = False  # 14 x 64 = 896: no key_length in the file


@functools.lru_cache(maxsize=None)
def _file(name, twin=False):
    """(spec, weights, path) of a model's GGUF; twin: its llama-architecture twin -- the same shapes and seed
    (so the same projections), no bias, no norm."""
    import os
    import tempfile
    sp = MODELS[name]
    if twin:
        sp = dict(sp, arch="llama", bias=False, norm=False)
    w = R.weights(sp)
    path = os.path.join(tempfile.mkdtemp(prefix="decoder_arch_"), f"{name}{'_twin' if twin else ''}.gguf")
    return sp, w, R.write_gguf(path, sp, w)


def _build(name, quant="bf16", twin=False):
    """A CausalLM on the GPU from the file's tensors (no GGML types: quant "q4" puts every projection on Q4G32)."""
    import numpy as np
    import torch
    from libsplinter_amd.models.decoder import CausalLM, config_from_gguf
    from libsplinter_amd.models.gguf import GGUFFile
    g = GGUFFile(_file(name, twin)[2])
    tensors = {n: torch.from_numpy(np.ascontiguousarray(g.to_numpy_f32(n))) for n in g.tensors}
    return CausalLM(config_from_gguf(g), tensors, "cuda", quant=quant)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("name", list(MODELS))
def test_gpu_forward_against_fp64_and_the_llama_twin(name):
    """40-token prompt, eager GPU forward (MFMA GEMMs, dec_qk_prep, HIP attention) against the fp64 reference.
    The fused step adds no rounding -- everything up to its single bf16 store is fp32 -- so the relative error
    may be at most twice that of the llama twin of the same shapes against the twin's own reference, measured
    here.  Measured on an MI355X: see profiles/decoder_arch/README.md."""
    ids = R.prompt(40)
    rel = {}
    for twin in (False, True):
        sp, w, _ = _file(name, twin)
        m = _build(name, twin=twin)
        assert m.extras != twin and m.cfg.q_dim == sp["H"] * sp["hd"]
        got = m.forward(ids).cpu()
        rel[twin] = _rel(got, R.ref_logits(sp, w, ids)[-1])
    print(f"{name}: rel {rel[False]:.4e}, llama twin rel {rel[True]:.4e}, ratio {rel[False] / rel[True]:.3f}")
    assert rel[False] <= 2.0 * rel[True]


def test_llama_paths_keep_the_bits_of_the_commit_before():
    """A file without general.architecture (served as llama), the random-init model's eager forward and its
    DecodeEngine after 8 steps: the logits the commit before qwen2 / qwen3 support computed on an MI355X, stored
    under tests/golden/decoder_arch, bit for bit -- the llama path calls the same kernels with the same
    arguments as before."""
    import os
    import tempfile
    import numpy as np
    from libsplinter_amd.models.decoder import CausalLM, DecodeEngine, DecoderConfig
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_arch")
    sp = R.spec("llama", seed=11)
    path = R.write_gguf(os.path.join(tempfile.mkdtemp(prefix="decoder_arch_"), "noarch.gguf"), sp, R.weights(sp),
                        arch_key=False)
    m, _ = CausalLM.from_gguf(path, device="cuda", quant="bf16")
    assert not m.extras and m.cfg.arch == "llama"
    got = m.forward(R.prompt(24)).cpu().numpy()
    assert np.array_equal(got, np.load(os.path.join(gold, "noarch_llama_logits_gpu.npy")))
    rid = [256] + list(b"hello there, decoder")
    got = CausalLM.random(DecoderConfig(), device="cuda").forward(rid).cpu().numpy()
    assert np.array_equal(got, np.load(os.path.join(gold, "random_init_logits_gpu.npy")))
    eng = DecodeEngine(CausalLM.random(DecoderConfig(), device="cuda"), use_graph=False)
    eng.first_token(rid)
    for _ in range(8):
        eng.next_token()
    assert np.array_equal(eng.logits.cpu().numpy(), np.load(os.path.join(gold, "random_init_engine_logits_gpu.npy")))


PROMPTS = [[256] + [97 + (i * (k + 3)) % 26 for i in range(n - 1)] for k, n in enumerate((5, 27, 90))]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("quant", ["bf16", "q4"])
@pytest.mark.parametrize("name", list(MODELS))
def test_decode_engine_steps_match_eager_forward(name, quant, graph):
    """DecodeEngine (GEMVs, dec_qk_prep_kv inside the step, device-state attention) against the eager forward,
    token by token, teacher forced."""
    import torch
    eager, mdl = _build(name, quant), _build(name, quant)
    from libsplinter_amd.models.decoder import DecodeEngine
    eng = DecodeEngine(mdl, use_graph=graph)
    ids = PROMPTS[1]
    eng.first_token(ids)
    eager.forward(ids)
    for t in (72, 101, 108, 108, 111):
        eng.st[1] = t
        eng._step()
        torch.cuda.synchronize()
        mdl.pos += 1
        ref = eager.forward([t])
        got = eng.logits[: mdl.cfg.vocab]
        assert (got - ref).norm() / ref.norm() < 3e-2
    if graph:
        assert len(eng.graphs) == 1


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("quant", ["bf16", "q4"])
@pytest.mark.parametrize("name", list(MODELS))
def test_batch_engine_steps_match_eager_forward(name, quant, graph):
    """Three sequences (prompts of 5, 27 and 90 tokens) stepped together, teacher forced: each slot's logits
    against its own eager CausalLM.forward."""
    from libsplinter_amd.models.decoder import BatchDecodeEngine
    mdl = _build(name, quant)
    cfg = mdl.cfg
    eng = BatchDecodeEngine(mdl, max_seqs=4, use_graph=graph)
    eagers, slots = [], []
    for ids in PROMPTS:
        e = _build(name, quant)
        e.forward(ids)
        eagers.append(e)
        slots.append(eng.admit(ids)[0])
    assert slots == [0, 1, 2] and mdl.kv is None and mdl.pos == 0
    for i in range(5):
        toks = [72 + i + 3 * k for k in range(3)]
        for s, t in zip(slots, toks):
            eng.set_token(s, t)
        out = eng.step()
        assert sorted(out) == slots
        for k, s in enumerate(slots):
            ref = eagers[k].forward([toks[k]])
            got = eng.logits[s, : cfg.vocab]
            rel = ((got - ref).norm() / ref.norm()).item()
            assert rel < 3e-2, (i, k, rel)
    assert int(eng.host_tok[3]) == -1
    if graph:
        assert len(eng.graphs) == 1


def test_qwen2_sequence_in_a_batch_of_three_equals_the_sequence_alone():
    """Tokens and per-step logits of one sequence, bit for bit, alone and with two others sharing its steps."""
    import torch
    from libsplinter_amd.models.decoder import BatchDecodeEngine
    mdl = _build("qwen2")
    runs = []
    for others in (False, True):
        eng = BatchDecodeEngine(mdl, max_seqs=4, seed=99)
        if others:
            eng.admit(PROMPTS[2], seed=3)
        slot, first = eng.admit(PROMPTS[1], seed=7)
        if others:
            eng.admit(PROMPTS[0], seed=5)
        toks, lgs = [first], []
        for _ in range(12):
            toks.append(eng.step()[slot])
            lgs.append(eng.logits[slot].clone())
        runs.append((toks, lgs, eng.kv[slot, :, :, : len(PROMPTS[1]) + 12].clone()))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert torch.equal(runs[0][2], runs[1][2])


def test_qwen2_chunked_prefill_with_and_without_the_prefix_cache():
    """prefill(C = 16) of three requests, two of which carry a 40-token shared head (32 rows reused): first
    tokens, cache rows and the logits of teacher-forced steps are bit-identical with and without set_prefix."""
    import torch
    from libsplinter_amd.models.decoder import BatchDecodeEngine
    C = 16
    mdl = _build("qwen2")
    head = [256] + [97 + (7 * i + i // 5) % 26 for i in range(39)]
    wave = [head + [65 + (3 * i) % 26 for i in range(7)], [256] + [70 + i % 20 for i in range(30)],
            head + [66 + (5 * i) % 26 for i in range(21)]]
    engs, firsts = [], []
    for prefix in (True, False):
        eng = BatchDecodeEngine(mdl, max_seqs=4, use_graph=False)
        if prefix:
            assert eng.set_prefix(head, C) == 32
        slots = [eng.submit(ids, seed=11 + k) for k, ids in enumerate(wave)]
        assert slots == [0, 1, 2]
        first = {}
        while eng.pending():
            first.update(eng.prefill(C))
            assert eng.prefill_passes < 20
        engs.append(eng)
        firsts.append(first)
    a, b = engs
    assert a.prefix_hits == 1 and a.prefix_rows_reused == 32 and b.prefix_hits == 0
    assert firsts[0] == firsts[1]
    for s, ids in enumerate(wave):
        assert torch.equal(a.kv[s, :, :, : len(ids)], b.kv[s, :, :, : len(ids)]), s
    for i in range(3):
        for s in range(3):
            a.set_token(s, 70 + i + 3 * s)
            b.set_token(s, 70 + i + 3 * s)
        a.step()
        b.step()
        for s in range(3):
            assert torch.equal(a.logits[s], b.logits[s]), (i, s)
