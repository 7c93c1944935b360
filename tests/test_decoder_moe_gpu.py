"""Mixture-of-experts decoders on the GPU (csrc/hip/decoder_moe.hip and its users in models/decoder.py): the
router against fp64, the per-expert GEMV bit for bit against dec_gemv* on the expert's slice, the weighted
down GEMV and the prefill grouping kernels against fp64 / numpy, and the models end to end -- eager forward
against the forced fp64 reference of tests/decoder_moe_ref.py, DecodeEngine against the forced eager forward,
run-to-run bits, and the --batch fallback.  Every test prints the figure it bounds; those measured on an MI355X
are in profiles/decoder_moe/README.md."""
import functools

import pytest

import decoder_arch_ref as R
import decoder_moe_ref as M

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue
EPS = 1e-6


@functools.lru_cache(maxsize=None)
def _lib():
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig
    return CausalLM.random(DecoderConfig(layers=1), seed=1, device="cuda").L


def _gen(seed):
    import torch
    return torch.Generator(device="cuda").manual_seed(seed)


# ------------------------------------------------------------------ router --
def _distinct_logits(T, E, ld, spread, seed):
    """[T, ld] fp32: columns < E hold a per-row permutation of E evenly spaced values over +-spread (pairwise
    distinct in fp32 and in fp64), columns >= E a sentinel that would win every round if it were read."""
    import torch
    g = _gen(seed)
    grid = torch.linspace(-spread, spread, E, device="cuda", dtype=torch.float64).float()
    out = torch.full((T, ld), 3e38, device="cuda")
    for t in range(T):
        out[t, :E] = grid[torch.randperm(E, device="cuda", generator=g)]
    return out


def _route(L, logits, T, E, k, ids=None, w=None):
    import torch
    ids = torch.full((T, k), -7, dtype=torch.int32, device="cuda") if ids is None else ids
    w = torch.full((T, k), -7.0, device="cuda") if w is None else w
    rc = L.dec_moe_route(logits.data_ptr(), logits.stride(0), T, E, k, ids.data_ptr(), w.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, ids, w


@pytest.mark.parametrize("spread", [30.0, 1e4])
@pytest.mark.parametrize("T", [1, 131])
@pytest.mark.parametrize("E", [8, 60, 128, 256])
def test_route_against_fp64(E, T, spread):
    """Chosen ids and their order equal the fp64 choice on pairwise-distinct logits; weights within 2^-16
    relative of fp64 (fp32 exp and one division sit near 2^-22; a bf16 rounding, 2^-9, does not fit) plus 2^-126,
    the smallest normal fp32, below which a weight of the +-1e4 rows flushes; the weights of a row sum to 1 within
    2^-16; columns >= E (a sentinel larger than every logit) are never read."""
    import torch
    L = _lib()
    for k in (1, 2, 8):
        lg = _distinct_logits(T, E, E + 5, spread, seed=E * 31 + T + k)
        rc, ids, w = _route(L, lg, T, E, k)
        assert rc == 0
        ref = lg[:, :E].double()
        rid = M.route(ref, k)
        assert torch.equal(ids.long(), rid), (E, T, k)
        assert all(len(set(r)) == k for r in ids.tolist())
        rw = torch.softmax(ref.gather(1, rid), -1)
        err = (w.double() - rw).abs()
        bound = 2.0 ** -16 * rw + 2.0 ** -126
        print(f"route E={E} T={T} k={k} spread={spread}: max err/bound {(err / bound).max().item():.4f}")
        assert bool((err <= bound).all())
        assert bool(((w.double().sum(-1) - 1.0).abs() <= 2.0 ** -16).all())


def test_route_ties_go_to_the_lowest_index():
    import torch
    L = _lib()
    lg = torch.zeros((3, 70), device="cuda")
    lg[1, [5, 64, 65, 69]] = 2.0           # four equal maxima across two lanes' columns, then equal zeros
    lg[2] = torch.arange(70, device="cuda") // 4 * -1.0   # runs of four equal values
    rc, ids, w = _route(L, lg, 3, 70, 8)
    assert rc == 0
    assert ids.tolist() == [list(range(8)), [5, 64, 65, 69, 0, 1, 2, 3], list(range(8))]
    assert torch.allclose(w[0], torch.full((8,), 0.125, device="cuda"), rtol=0, atol=2 ** -20)


def test_route_refuses_bad_arguments_before_any_launch():
    import torch
    L = _lib()
    lg = torch.randn((4, 300), device="cuda")
    for T, E, k, ld in ((4, 257, 2, 300), (4, 8, 9, 300), (4, 4, 5, 300), (4, 8, 0, 300), (0, 8, 2, 300),
                        (4, 0, 1, 300), (4, 8, 2, 7)):
        ids = torch.full((4, 9), -7, dtype=torch.int32, device="cuda")
        w = torch.full((4, 9), -7.0, device="cuda")
        assert L.dec_moe_route(lg.data_ptr(), ld, T, E, k, ids.data_ptr(), w.data_ptr(), None) == INVALID
        torch.cuda.synchronize()
        assert bool((ids == -7).all()) and bool((w == -7.0).all())
    ids = torch.full((4, 2), -7, dtype=torch.int32, device="cuda")
    assert L.dec_moe_route(None, 300, 4, 8, 2, ids.data_ptr(), ids.data_ptr(), None) == INVALID
    assert L.dec_moe_route(lg.data_ptr(), 300, 4, 8, 2, None, ids.data_ptr(), None) == INVALID


# ------------------------------------------------------------------ expert GEMVs --
IDS = {1: [3], 2: [3, 1], 4: [2, 0, 3, 1]}  # out of order; E = 4
E4 = 4


def _planes(L, W, kind):
    """(weight object, ctypes plane pointers) of a bf16 matrix as bf16 / Q4G32 / Q8G32."""
    from libsplinter_amd.models.decoder import Q4Weight, Q8Weight
    if kind == "bf16":
        return W, (W.data_ptr(),)
    q = (Q4Weight if kind == "q4" else Q8Weight).quantize(L, W)
    return q, (q.q.data_ptr(), q.sm.data_ptr())


def _rows(w, a, b):
    return w[a:b] if not hasattr(w, "rows") else w.rows(a, b)


def _ptrs(w):
    return (w.data_ptr(),) if not hasattr(w, "q") else (w.q.data_ptr(), w.sm.data_ptr())


def _exact(w):
    """fp64 values of a weight as the GEMV kernels read it: bf16, or d * q + m from the planes."""
    import torch
    if not hasattr(w, "q"):
        return w.double()
    sm = w.sm.view(torch.int32)
    d = (sm << 16).view(torch.float32).double()
    m = (sm & -65536).view(torch.float32).double()
    if w.bits == 4:
        q = torch.stack([w.q & 15, w.q >> 4], -1).reshape(w.q.shape[0], -1).double()
    else:
        q = w.q.double()
    N, K = q.shape
    return (q.reshape(N, K // 32, 32) * d[:, :, None] + m[:, :, None]).reshape(N, K)


@pytest.mark.parametrize("kind", ["bf16", "q4", "q8"])
@pytest.mark.parametrize("K", [64, 576, 2048])
def test_expert_upgate_gemv_is_dec_gemv_on_the_experts_slice(K, kind):
    """Row block j of dec_gemv_moe* equals dec_gemv* mode 2 on expert ids[j]'s rows bit for bit (one loop text),
    with and without the fused RMSNorm; the row after the k blocks keeps its sentinel."""
    import torch
    L = _lib()
    g = _gen(K)
    moe = getattr(L, "dec_gemv_moe" + ("" if kind == "bf16" else "_" + kind))
    one = getattr(L, "dec_gemv" + ("" if kind == "bf16" else "_" + kind))
    for F in (16, 48, 768):
        W = (torch.randn((E4 * 2 * F, K), device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
        wo, planes = _planes(L, W, kind)
        x = torch.randn(K, device="cuda", generator=g).to(torch.bfloat16)
        rw = 1.0 + 0.1 * torch.randn(K, device="cuda", generator=g)
        for k, idl in IDS.items():
            for rms in (rw.data_ptr(), None):
                ids = torch.tensor(idl, dtype=torch.int32, device="cuda")
                out = torch.full((k + 1, F), 7.0, dtype=torch.bfloat16, device="cuda")
                assert moe(x.data_ptr(), rms, EPS, *planes, 2 * F, K, ids.data_ptr(), k, E4, out.data_ptr(), None) == 0
                want = torch.empty((k, F), dtype=torch.bfloat16, device="cuda")
                for j, e in enumerate(idl):
                    sl = _rows(wo, e * 2 * F, (e + 1) * 2 * F)
                    assert one(2, x.data_ptr(), rms, EPS, *_ptrs(sl), 2 * F, K, None, want[j].data_ptr(), None) == 0
                torch.cuda.synchronize()
                assert torch.equal(out[:k], want), (F, k, rms is not None)
                assert bool((out[k] == 7.0).all())
                assert want.float().abs().max() > 0
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.full((4, 16), 7.0, dtype=torch.bfloat16, device="cuda")
    for N, KK, k, E in ((32, K + 4, 1, 4), (48, K, 1, 4), (32, K, 9, 16), (32, K, 3, 2), (32, K, 0, 4), (32, 32768, 1, 4)):
        assert moe(x.data_ptr(), None, EPS, *planes, N, KK, ids.data_ptr(), k, E, out.data_ptr(), None) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("kind", ["bf16", "q4", "q8"])
@pytest.mark.parametrize("d", [64, 576, 2048])
def test_expert_down_gemv_against_fp64(d, kind):
    """out = bf16(res + sum_j w_j W[ids_j] f_j) within 2^-8 |ref| + a of fp64 over the values the kernel reads.
    2^-8 |ref| is one round-to-nearest to bf16; a, the fp32 arithmetic ahead of it, is measured here: twice the
    worst excess over 2^-8 |ref| of the existing dec_gemv* mode 1 on one expert's slice at the same K.  The 4- /
    8-bit planes need K % 32 == 0: F 16 and 48 are refused there, outputs untouched."""
    import torch
    L = _lib()
    g = _gen(d + 1)
    sfx = "" if kind == "bf16" else "_" + kind
    down, one = getattr(L, "dec_gemv_moe_down" + sfx), getattr(L, "dec_gemv" + sfx)
    for F in (16, 48, 768):
        W = (torch.randn((E4 * d, F), device="cuda", generator=g) / F ** 0.5).to(torch.bfloat16)
        f = torch.randn((4, F), device="cuda", generator=g).to(torch.bfloat16)
        res = torch.randn(d, device="cuda", generator=g).to(torch.bfloat16)
        if kind != "bf16" and F % 32:
            out = torch.full((d,), 7.0, dtype=torch.bfloat16, device="cuda")
            z = torch.zeros(4, dtype=torch.int32, device="cuda")
            assert down(f.data_ptr(), W.data_ptr(), z.data_ptr(), d, F, z.data_ptr(), z.data_ptr(), 1, E4,
                        res.data_ptr(), out.data_ptr(), None) == INVALID
            torch.cuda.synchronize()
            assert bool((out == 7.0).all())
            continue
        wo, planes = _planes(L, W, kind)
        Wx = _exact(wo).reshape(E4, d, F)
        # a: the existing one-expert GEMV + residual at this K against fp64
        o1 = torch.empty(d, dtype=torch.bfloat16, device="cuda")
        assert one(1, f[0].data_ptr(), None, EPS, *_ptrs(_rows(wo, d, 2 * d)), d, F, res.data_ptr(), o1.data_ptr(),
                   None) == 0
        torch.cuda.synchronize()
        r1 = res.double() + Wx[1] @ f[0].double()
        a = 2.0 * max(0.0, ((o1.double() - r1).abs() - 2.0 ** -8 * r1.abs()).max().item())
        for k, idl in IDS.items():
            ids = torch.tensor(idl, dtype=torch.int32, device="cuda")
            w = torch.softmax(torch.randn(k, device="cuda", generator=g), -1)
            out = torch.full((d + 8,), 7.0, dtype=torch.bfloat16, device="cuda")
            assert down(f.data_ptr(), *planes, d, F, ids.data_ptr(), w.data_ptr(), k, E4, res.data_ptr(),
                        out.data_ptr(), None) == 0
            torch.cuda.synchronize()
            ref = res.double()
            for j, e in enumerate(idl):
                ref = ref + w[j].double() * (Wx[e] @ f[j].double())
            err = (out[:d].double() - ref).abs()
            ratio = (err / (2.0 ** -8 * ref.abs() + a).clamp_min(1e-300)).max().item()
            excess = (err - 2.0 ** -8 * ref.abs()).max().item()
            print(f"moe_down {kind} d={d} F={F} k={k}: a {a:.3e}, worst excess {excess:.3e}, max err/bound {ratio:.3f}")
            assert bool((err <= 2.0 ** -8 * ref.abs() + a).all()), (F, k)
            assert bool((out[d:] == 7.0).all())
    z = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.full((d,), 7.0, dtype=torch.bfloat16, device="cuda")
    for dd, FF, k, E in ((d, 20, 1, 4), (d, 32768, 1, 4), (d, 768, 9, 16), (d, 768, 3, 2), (0, 768, 1, 4)):
        assert down(f.data_ptr(), *planes, dd, FF, z.data_ptr(), w.data_ptr(), k, E, res.data_ptr(), out.data_ptr(),
                    None) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------ prefill grouping --
@pytest.mark.parametrize("T,E,k", [(1, 8, 2), (5, 8, 2), (131, 8, 2), (300, 8, 2), (3, 128, 8)])
def test_plan_gather_combine(T, E, k):
    """counts / base / slot against numpy (starts multiples of 128, slots in (t, j) order, equal bits on a second
    run); gathered rows bit-equal to their sources, rows no slot names untouched; combine within one bf16
    rounding of fp64: 2^-8 |ref| + 8 * 2^-23 * (|res| + sum_j |w_j y_j|), the k + 1 <= 9 fp32 operations ahead
    of the rounding, each within 2^-24 of a partial sum that the bracket bounds."""
    import numpy as np
    import torch
    L = _lib()
    g = _gen(T * 1000 + E)
    d = 136
    ids = torch.stack([torch.randperm(E, device="cuda", generator=g)[:k] for _ in range(T)]).to(torch.int32)
    if T >= 131:
        ids[:, 0] = 5       # one expert past a 128-row tile, experts that get nothing
        ids[:, 1] = torch.where(torch.arange(T, device="cuda") % 3 == 0, 1, 6).to(torch.int32)
    runs = []
    for _ in range(2):
        counts = torch.full((E,), -1, dtype=torch.int32, device="cuda")
        base = torch.full((E,), -1, dtype=torch.int32, device="cuda")
        slot = torch.full((T, k), -1, dtype=torch.int32, device="cuda")
        assert L.dec_moe_plan(ids.data_ptr(), T, k, E, 128, counts.data_ptr(), base.data_ptr(), slot.data_ptr(),
                              None) == 0
        torch.cuda.synchronize()
        runs.append((counts.cpu().numpy(), base.cpu().numpy(), slot.cpu().numpy()))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    counts_h, base_h, slot_h = runs[0]
    flat = ids.cpu().numpy().reshape(-1)
    want_counts = np.bincount(flat, minlength=E)
    want_base = np.concatenate([[0], np.cumsum((want_counts + 127) // 128 * 128)[:-1]])
    assert np.array_equal(counts_h, want_counts) and np.array_equal(base_h, want_base) and not (base_h % 128).any()
    seen = np.zeros(E, np.int64)
    for i, e in enumerate(flat):  # stable: rank in (t, j) order
        assert slot_h.reshape(-1)[i] == want_base[e] + seen[e]
        seen[e] += 1
    rows = int(((want_counts + 127) // 128 * 128).sum())

    x = torch.full((T, d + 8), 5.0, dtype=torch.bfloat16, device="cuda")
    x[:, :d] = torch.randn((T, d), device="cuda", generator=g).to(torch.bfloat16)
    xg = torch.full((rows, d), 7.0, dtype=torch.bfloat16, device="cuda")
    assert L.dec_moe_gather(x.data_ptr(), x.stride(0), T, k, d, slot.data_ptr(), rows, xg.data_ptr(), None) == 0
    torch.cuda.synchronize()
    sl = slot.long().reshape(-1)
    assert torch.equal(xg[sl], x[:, :d].repeat_interleave(k, 0))
    pad = torch.ones(rows, dtype=torch.bool, device="cuda")
    pad[sl] = False
    assert bool((xg[pad] == 7.0).all()) and int(pad.sum()) == rows - T * k

    y = torch.randn((rows, d), device="cuda", generator=g)
    w = torch.softmax(torch.randn((T, k), device="cuda", generator=g), -1)
    res = x[:, :d].contiguous()
    out = torch.full((T, d + 8), 7.0, dtype=torch.bfloat16, device="cuda")
    assert L.dec_moe_combine(y.data_ptr(), rows, T, k, d, slot.data_ptr(), w.data_ptr(), res.data_ptr(), d,
                             out.data_ptr(), d + 8, None) == 0
    torch.cuda.synchronize()
    terms = w.double()[:, :, None] * y.double()[slot.long()]
    ref = res.double() + terms.sum(1)
    bound = 2.0 ** -8 * ref.abs() + 8 * 2.0 ** -23 * (res.double().abs() + terms.abs().sum(1))
    err = (out[:, :d].double() - ref).abs()
    print(f"combine T={T} E={E} k={k}: max err/bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()) and bool((out[:, d:] == 7.0).all())
    # refusals leave the outputs alone
    assert L.dec_moe_plan(ids.data_ptr(), T, 9, E, 128, counts.data_ptr(), base.data_ptr(), slot.data_ptr(), None) == INVALID
    assert L.dec_moe_gather(x.data_ptr(), x.stride(0), T, k, d + 4, slot.data_ptr(), rows, xg.data_ptr(), None) == INVALID
    assert L.dec_moe_combine(y.data_ptr(), rows, T, k, d + 2, slot.data_ptr(), w.data_ptr(), res.data_ptr(), d,
                             out.data_ptr(), d + 8, None) == INVALID


# ------------------------------------------------------------------ models --
# The seeds are fixed by the fp64 reference alone: of seeds 31..38 (E 8) and 40..99 (E 32), those whose 80 free
# fp64 decisions on R.prompt(40) have the fewest gaps under 0.03 between the k-th and the (k+1)-th router logit
# (at most 3 of 80).  bf16 activations and router weights move a logit of order 2 by about 0.01, so only
# such a decision can fall the other way on the GPU.
MODELS = {
    "qwen3moe_e8k2": M.spec("qwen3moe", E=8, k=2, F=64, d=128, H=2, KVH=1, hd=128, n_ctx=128, seed=37),
    "mixtral_e8k2": M.spec("llama", E=8, k=2, F=64, d=128, H=2, KVH=1, n_ctx=128, seed=33),
    "qwen3moe_e32k4": M.spec("qwen3moe", E=32, k=4, F=64, d=128, H=2, KVH=1, hd=128, n_ctx=128, seed=44),
    "mixtral_e32k4": M.spec("llama", E=32, k=4, F=64, d=128, H=2, KVH=1, n_ctx=128, seed=51),
}


@functools.lru_cache(maxsize=None)
def _file(name, twin=False):
    import os
    import tempfile
    sp = MODELS[name]
    path = os.path.join(tempfile.mkdtemp(prefix="decoder_moe_"), f"{name}{'_twin' if twin else ''}.gguf")
    if twin:
        sp = M.dense_twin(sp)
        w = R.weights(sp)
        return sp, w, R.write_gguf(path, sp, w)
    w = M.weights(sp)
    return sp, w, M.write_gguf(path, sp, w)


def _build(name, quant="bf16", twin=False):
    """A CausalLM on the GPU from the file's tensors.  quant "q4": up|gate, attention and head on Q4G32 and --
    by naming the down tensors as Q6_K -- the down projections on Q8G32, as a Q4_K_M file has them."""
    import numpy as np
    import torch
    from libsplinter_amd.models.decoder import CausalLM, config_from_gguf
    from libsplinter_amd.models.gguf import GGUFFile
    g = GGUFFile(_file(name, twin)[2])
    tensors = {n: torch.from_numpy(np.ascontiguousarray(g.to_numpy_f32(n))) for n in g.tensors}
    return CausalLM(config_from_gguf(g), tensors, "cuda", quant=quant,
                    ggml_types={n: 14 for n in g.tensors if "ffn_down" in n})


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _sets_differ(a, b):
    """Decisions (rows) of two [n, k] id tensors whose chosen SETS differ."""
    return sum(set(x) != set(y) for x, y in zip(a.tolist(), b.tolist()))


@pytest.mark.parametrize("name", list(MODELS))
def test_gpu_forward_against_forced_fp64_and_the_dense_twin(name):
    """40-token prompt through the eager GPU forward (router GEMM, dec_moe_route / plan / gather, per-expert MFMA
    GEMMs, dec_moe_combine) with route_log on; the fp64 reference FORCED to the GPU's choices.  Logit rel error at
    most twice that of the dense llama twin (same d, heads and seed, ffn = k F) against its own reference,
    measured here; and the reference's own top-k differs from the GPU's in at most 4 of the 80 decisions."""
    import torch
    ids = R.prompt(40)
    sp, w, _ = _file(name)
    m = _build(name)
    assert m.cfg.experts == sp["E"] and m.cfg.experts_used == sp["k"] and m.extras == (sp["arch"] == "qwen3moe")
    m.route_log = []
    got = m.forward(ids).cpu()
    chosen = [t.cpu().long() for t in m.route_log]
    assert len(chosen) == sp["layers"] and all(c.shape == (40, sp["k"]) for c in chosen)
    assert all(len(set(r)) == sp["k"] for c in chosen for r in c.tolist())
    ref, rl, _ = M.ref_logits(sp, w, ids, forced=chosen)
    rel = _rel(got, ref[-1])
    differ = sum(_sets_differ(c, M.route(l, sp["k"])) for c, l in zip(chosen, rl))
    tsp, tw, _ = _file(name, True)
    twin = _rel(_build(name, twin=True).forward(ids).cpu(), R.ref_logits(tsp, tw, ids)[-1])
    print(f"{name}: rel {rel:.4e}, dense twin rel {twin:.4e}, ratio {rel / twin:.3f}; decisions that differ from "
          f"the forced reference's own: {differ} of {40 * sp['layers']}")
    assert torch.isfinite(got).all()
    assert rel <= 2.0 * twin
    assert differ <= 4


PROMPT = [256] + [97 + (i * 4) % 26 for i in range(26)]  # test_decoder_arch_gpu's PROMPTS[1]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("quant", ["bf16", "q4"])
@pytest.mark.parametrize("name", ["qwen3moe_e8k2", "mixtral_e8k2"])
def test_decode_engine_steps_match_forced_eager_forward(name, quant, graph):
    """DecodeEngine (router GEMV, dec_moe_route, dec_gemv_moe*, dec_gemv_moe_down* inside the step) against the
    eager forward forced to the engine's choices, 5 teacher-forced steps: logits within the project's 3e-2; the
    eager forward's own choice differs from the engine's in at most 1 of the 10 decisions; one graph."""
    import torch
    from libsplinter_amd.models.decoder import DecodeEngine
    eager, mdl = _build(name, quant), _build(name, quant)
    k = mdl.cfg.experts_used
    eng = DecodeEngine(mdl, use_graph=graph)
    eng.first_token(PROMPT)
    eager.forward(PROMPT)
    differ = 0
    for t in (72, 101, 108, 108, 111):
        eng.st[1] = t
        eng._step()
        torch.cuda.synchronize()
        mdl.pos += 1
        picks = [i.clone().reshape(1, k) for i in eng.moe_ids]
        assert all(len(set(p[0].tolist())) == k for p in picks)
        assert all(abs(float(x.sum()) - 1.0) < 1e-5 for x in eng.moe_w)
        eager.route_force, eager.route_log = None, []
        eager.forward([t])                       # its own choice; then the same token again, forced
        differ += sum(_sets_differ(a, b) for a, b in zip(eager.route_log, picks))
        eager.pos -= 1
        eager.route_force, eager.route_log = picks, None
        ref = eager.forward([t])
        got = eng.logits[: mdl.cfg.vocab]
        rel = ((got - ref).norm() / ref.norm()).item()
        print(f"{name} {quant} graph={graph} token {t}: rel {rel:.4e}")
        assert rel < 3e-2
    print(f"{name} {quant} graph={graph}: eager's own choice differs in {differ} of 10 decisions")
    assert differ <= 1
    if graph:
        assert len(eng.graphs) == 1


@pytest.mark.parametrize("quant", ["bf16", "q4"])
def test_two_runs_give_the_same_tokens_and_bits(quant):
    """first_token + 12 next_token, twice over fresh engines on one model: tokens and every step's logits
    bit-identical (no atomics, no launch-order dependence in the route, expert GEMV and down kernels)."""
    from libsplinter_amd.models.decoder import DecodeEngine
    mdl = _build("qwen3moe_e32k4", quant)
    runs = []
    for _ in range(2):
        eng = DecodeEngine(mdl, seed=11)
        toks, lgs = [eng.first_token(PROMPT)], []
        for _ in range(12):
            toks.append(eng.next_token())
            lgs.append(eng.logits.clone())
        runs.append((toks, lgs))
    assert runs[0][0] == runs[1][0]
    assert all(bool((a == b).all()) for a, b in zip(runs[0][1], runs[1][1]))


def test_batch_falls_back_to_sequential_serving(capsys):
    from types import SimpleNamespace
    from libsplinter_amd.daemons.splainference import Splainference
    from libsplinter_amd.models.decoder import BatchDecodeEngine, DecodeEngine
    mdl = _build("mixtral_e8k2")
    with pytest.raises(ValueError, match="mixture-of-experts"):
        BatchDecodeEngine(mdl, 4)
    capsys.readouterr()
    d = Splainference(None, mdl, None, SimpleNamespace(top_p=0.9, temp=0.7, seed=1, mask=None), batch=4,
                      prefill_chunk=64, prefix_cache=True)
    assert isinstance(d.engine, DecodeEngine) and d.batch_engine is None
    assert d.prefill_chunk == 0 and not d.prefix_cache
    out = capsys.readouterr().out
    assert out.count("[Warn]") == 1 and "mixture-of-experts" in out


def test_gpu_refuses_an_expert_width_the_kernels_do_not_take():
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig
    cfg = DecoderConfig(d=128, heads=2, kv_heads=1, layers=1, experts=4, experts_used=2, expert_ffn=96)
    with pytest.raises(ValueError, match="expert_feed_forward_length 96"):
        CausalLM.random(cfg, device="cuda")
