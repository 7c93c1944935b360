"""Varlen attention (nomic_attention: k_attn3, and the fallback k_attn2) row by row.

Every case runs through one harness (`_launch`): `out` and the pad rows of `qkv` start as NaN, the
pad rows of `out` must come back untouched, every (row, head) of the real rows must be written, and
the relative L2 error over the 64 outputs of every single (row, head) is held against an fp64
reference computed per sequence from the same bf16 inputs.

The bound, 1e-2 per (row, head), is the project's global figure applied per row.  A correct kernel's
roundings (fp32 scores, P rounded to bf16 for the P V product, l summed from the unrounded P, output
rounded to bf16) give 3.5e-3 at worst on these inputs; `_emulate` is that arithmetic in torch, and
every case asserts that it stays at or below 5e-3 on its own inputs, so the bound hides no
ill-conditioned input.

A new attention form is one more entry in ATTN_VARIANTS."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ATTN_VARIANTS = [13, 6]

HD = 64
SCALE = 1.0 / 8.0
LOG2E = 1.4426950408889634
BOUND = 1e-2        # per (row, head), kernel vs fp64
EMU_BOUND = 5e-3    # per (row, head), the emulated roundings vs fp64
DEV = "cuda"


# ------------------------------------------------------------------ harness --
def _split3(qkv, T, heads):
    W = heads * HD
    x = qkv[:T].double()
    return tuple(x[:, i * W:(i + 1) * W].reshape(T, heads, HD) for i in range(3))


def _reference(qkv, cu, heads):
    """(fp64 softmax(Q K^T / 8) V, the emulated kernel roundings of the same), per sequence, [T, heads, 64]."""
    import torch
    T = int(cu[-1])
    q, k, v = _split3(qkv, T, heads)
    ref = torch.empty(T, heads, HD, dtype=torch.float64, device=qkv.device)
    emu = torch.empty_like(ref)
    for s in range(len(cu) - 1):
        a, e = int(cu[s]), int(cu[s + 1])
        sc = torch.einsum("qhd,khd->hqk", q[a:e], k[a:e])
        ref[a:e] = torch.einsum("hqk,khd->qhd", (sc * SCALE).softmax(-1), v[a:e])
        emu[a:e] = _emulate(sc, v[a:e])
    return ref, emu


def _emulate(sc, v):
    """The roundings of a correct kernel: scores in fp32, p = exp2 of the scaled distance to the row
    maximum in fp32, l summed from the unrounded p, p rounded to bf16 for the P V product (fp32
    accumulation is exact enough to be taken as fp64 here), output rounded to bf16."""
    import torch
    s32 = sc.float()
    p = torch.exp2((s32 - s32.amax(-1, keepdim=True)) * (SCALE * LOG2E))
    l = p.sum(-1)                                                     # [h, q]
    o = torch.einsum("hqk,khd->qhd", p.bfloat16().double(), v).float()
    return (o / l.T[..., None]).bfloat16().double()


def _row_err(got, ref):
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)     # [T, heads]


def _worst(err, cu):
    flat = int(err.argmax())
    row, head = divmod(flat, err.shape[1])
    seq = int(np.searchsorted(np.asarray(cu), row, side="right")) - 1
    return err.flatten()[flat].item(), (seq, row - int(cu[seq]), head)


class Case:
    """Inputs and references of one case, built once and shared by the variants (never written)."""

    def __init__(self, name, lens, heads, fill):
        import torch
        from libsplinter_amd.models.nomic import Batch
        self.name, self.lens, self.heads = name, list(lens), heads
        self.b = Batch([[0] * n for n in lens], device=DEV, qblock=128)
        self.cu = self.b.cu_host.tolist()
        T, W = self.b.T, heads * HD
        qkv = torch.full((self.b.T_pad, 3 * W), float("nan"), dtype=torch.bfloat16, device=DEV)
        q, k, v = fill(self)                                           # each [T, heads, 64] float
        qkv[:T] = torch.cat([t.reshape(T, W) for t in (q, k, v)], 1).to(torch.bfloat16)
        self.qkv = qkv
        self.ref, emu = _reference(qkv, self.cu, heads)
        self.emu_err, self.emu_at = _worst(_row_err(emu, self.ref), self.cu)


def _launch(L, variant, case):
    """One launch under the NaN sentinels -> out[:T] as fp64 [T, heads, 64]."""
    import torch
    from libsplinter_amd.models.nomic import _chk, _stream
    b, heads = case.b, case.heads
    T, W = b.T, heads * HD
    assert torch.isnan(case.qkv[T:].float()).all() and not torch.isnan(case.qkv[:T].float()).any()
    out = torch.full((b.T_pad, W), float("nan"), dtype=torch.bfloat16, device=DEV)
    sentinel = out.view(torch.int16).clone()
    prev = L.nomic_attention_set_variant(variant)
    try:
        _chk(L.nomic_attention(case.qkv.data_ptr(), out.data_ptr(), b.cu.data_ptr(), b.qblocks.data_ptr(), b.nqb,
                               heads, SCALE, _stream()), "attn")
        torch.cuda.synchronize()
    finally:
        L.nomic_attention_set_variant(prev)
    assert torch.equal(out.view(torch.int16)[T:], sentinel[T:]), "rows [T, T_pad) of out were written"
    nan = torch.isnan(out[:T].float()).reshape(T, heads, HD).any(-1)
    if nan.any():
        row, head = (int(x) for x in nan.nonzero()[0])
        seq = int(np.searchsorted(np.asarray(case.cu), row, side="right")) - 1
        raise AssertionError(f"{int(nan.sum())} (row, head) pairs unwritten or NaN, first: sequence {seq} "
                             f"(length {case.lens[seq]}) row {row - case.cu[seq]} head {head}")
    return out[:T].double().reshape(T, heads, HD)


def _check(L, variant, case):
    """The whole per-row check of one case on one variant; returns the kernel's output."""
    assert case.emu_err <= EMU_BOUND, f"{case.name}: the inputs are ill-conditioned, emulation {case.emu_err:.3e} " \
                                      f"at (sequence, row, head) {case.emu_at}"
    got = _launch(L, variant, case)
    err, at = _worst(_row_err(got, case.ref), case.cu)
    print(f"ATTN case={case.name} variant={variant} kernel={err:.3e} emulation={case.emu_err:.3e} "
          f"worst(seq,row,head)={at} len={case.lens[at[0]]}")
    assert err <= BOUND, f"{case.name} variant {variant}: relative error {err:.3e} > {BOUND} at sequence {at[0]} " \
                         f"(length {case.lens[at[0]]}) row {at[1]} head {at[2]}; emulation {case.emu_err:.3e}"
    return got


@pytest.fixture(scope="module")
def L():
    from libsplinter_amd.models.nomic import _lib
    return _lib()


def _gauss(seed):
    def fill(c):
        import torch
        g = torch.Generator(device=DEV).manual_seed(seed)
        return tuple(torch.randn(c.b.T, c.heads, HD, device=DEV, generator=g) for _ in range(3))
    return fill


# -------------------------------------------------------------------- cases --
EDGE_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 191, 193, 256, 257, 513, 1025]


@functools.lru_cache(maxsize=None)
def _case_edges():
    return Case("edges", EDGE_LENS, 12, _gauss(11))


@pytest.mark.parametrize("variant", ATTN_VARIANTS)
def test_edges(L, variant):
    """The boundaries of the 32-row wave, the 64-key tile and the 128-row q-block, 12 heads."""
    _check(L, variant, _case_edges())


@functools.lru_cache(maxsize=None)
def _case_leak():
    def fill(c):
        q, k, v = _gauss(12)(c)
        a, e = c.cu[1], c.cu[2]
        k[a:e] *= 64
        v[a:e] *= 64
        return q, k, v
    return Case("leak", [65, 1, 130], 12, fill)


@pytest.mark.parametrize("variant", ATTN_VARIANTS)
def test_neighbour_leak(L, variant):
    """A one-token sequence with K and V 64 times larger between two others: a key of a neighbouring
    sequence that reached a row of the outer sequences would put it far outside the per-row bound."""
    _check(L, variant, _case_leak())


# heads x q-block count: nqb * heads workgroups go through the XCD remap
REMAP_LENS = {3: [129, 65], 6: [257, 128, 33, 1], 7: [300, 129, 97, 5]}
REMAP_HEADS = [1, 2, 3, 5, 12]
REMAP_TABLE = [(h, n) for n in REMAP_LENS for h in REMAP_HEADS]


def _remap_coverage():
    """The table reaches every workgroup count modulo 8 and a grid of fewer than 8."""
    for n, lens in REMAP_LENS.items():
        assert sum((x + 127) // 128 for x in lens) == n
    assert {h * n % 8 for h, n in REMAP_TABLE} == set(range(8))
    assert any(h * n < 8 for h, n in REMAP_TABLE)
    assert any(h * n > 8 and h * n % 8 for h, n in REMAP_TABLE)


@functools.lru_cache(maxsize=None)
def _case_remap(heads, nqb):
    c = Case(f"remap_h{heads}_nqb{nqb}", REMAP_LENS[nqb], heads, _gauss(100 * heads + nqb))
    assert c.b.nqb == nqb
    return c


@pytest.mark.parametrize("variant", ATTN_VARIANTS)
@pytest.mark.parametrize("heads,nqb", REMAP_TABLE)
def test_heads_and_xcd_remap(L, variant, heads, nqb):
    """1, 2, 3, 5 and 12 heads over 3, 6 and 7 q-blocks: a workgroup map that is not a bijection
    leaves a (row, head) at the sentinel or computes one from another head's columns."""
    _remap_coverage()
    _check(L, variant, _case_remap(heads, nqb))


# per 64-key tile step of every row's maximum score, in log2 units (the kernels defer the rescale of
# O and l until the maximum has moved by more than 8)
RAMPS = {"up3": 3.0, "up9": 9.5, "down3": -3.0, "down9": -9.5}
RAMP_LEN = 513


@functools.lru_cache(maxsize=None)
def _case_ramp(name):
    step = RAMPS[name]

    def fill(c):
        import torch
        g = torch.Generator(device=DEV).manual_seed(13)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
        T, H = c.b.T, c.heads
        u = rnd(H, HD)
        u = u / u.norm(dim=-1, keepdim=True)
        cq = 4.0
        # score = q.k / 8 nats = cq * g / 8 * log2(e) log2 units  ->  g moves by dg per tile
        dg = abs(step) * 8.0 / (cq * LOG2E)
        tile = torch.arange(T, device=DEV) // 64
        ntile = (T + 63) // 64
        gk = dg * (tile if step > 0 else (ntile - 1 - tile)).float()
        q = 0.03 * rnd(T, H, HD) + cq * u
        k = 0.25 * rnd(T, H, HD) + gk[:, None, None] * u
        return q, k, rnd(T, H, HD)
    return Case(f"ramp_{name}", [RAMP_LEN], 12, fill)


@pytest.mark.parametrize("variant", ATTN_VARIANTS)
@pytest.mark.parametrize("ramp", list(RAMPS))
def test_rescale_paths(L, variant, ramp):
    """Every row's maximum score climbs (or falls) by a fixed step per key tile: +3 keeps the
    maximum deferred for two tiles, then rescales, with P up to 2^6 through bf16; +9.5 rescales on
    every tile; the descending ramps never rescale after the first tile and run P down to 0."""
    import torch
    c = _case_ramp(ramp)
    # the inputs do what the case says: per-tile row maxima move by the step, within 1.5 log2 units
    q, k, _ = _split3(c.qkv, c.b.T, c.heads)
    sc = torch.einsum("qhd,khd->hqk", q, k[: RAMP_LEN // 64 * 64]) * (SCALE * LOG2E)      # the 8 full tiles
    mx = sc.reshape(c.heads, RAMP_LEN, -1, 64).amax(-1)
    off = (mx.diff(dim=-1) - RAMPS[ramp]).abs().max().item()
    assert off < 1.0, off
    _check(L, variant, c)


ONEHOT_N = [64, 129, 513]


@functools.lru_cache(maxsize=None)
def _case_onehot(n):
    perm = {}

    def fill(c):
        import torch
        g = torch.Generator(device=DEV).manual_seed(1000 + n)
        H = c.heads
        s = (torch.randint(0, 2, (n, H, HD), device=DEV, generator=g) * 2 - 1).float()
        pi = torch.stack([torch.randperm(n, device=DEV, generator=g) for _ in range(H)], 1)   # [n, H]
        k = 4 * s
        q = 4 * torch.gather(s, 0, pi[:, :, None].expand(n, H, HD))
        j = torch.arange(n, device=DEV)[:, None, None]
        h = torch.arange(H, device=DEV)[None, :, None]
        d = torch.arange(HD, device=DEV)[None, None, :]
        v = ((7 * j + 3 * h + d) % 251 - 125).float()
        perm["pi"], perm["v"] = pi, v
        return q, k, v
    c = Case(f"onehot_{n}", [n], 12, fill)
    c.pi, c.v = perm["pi"], perm["v"]
    return c


@pytest.mark.parametrize("variant", ATTN_VARIANTS)
@pytest.mark.parametrize("n", ONEHOT_N)
def test_key_order_one_hot(L, variant, n):
    """One-hot attention: query i matches key pi(i) alone (128 nats, every other key at least 30
    lower), so output row i is V[pi(i)], a row of small integers, to one bf16 step.  A P fragment
    whose k-slots are not the keys the V fragment holds, or a transposed read, returns another row.
    Scores of 128 nats also overflow a softmax that does not subtract the row maximum."""
    import torch
    c = _case_onehot(n)
    H = c.heads
    q, k, v = _split3(c.qkv, n, H)
    assert torch.equal(v, c.v.double()), "V must be exact in bf16"
    sc = torch.einsum("qhd,khd->hqk", q, k) * SCALE                      # [H, n, n] nats
    hit = torch.zeros_like(sc, dtype=torch.bool)
    hit.scatter_(2, c.pi.T[:, :, None], True)
    assert (sc[hit] == 128.0).all()
    assert sc[~hit].max().item() <= 128.0 - 30.0, sc[~hit].max().item()
    got = _check(L, variant, c)
    want = torch.gather(c.v.double(), 0, c.pi[:, :, None].expand(n, H, HD))
    bad = (got - want).abs() > want.abs() * 2.0 ** -7 + 1e-6
    if bad.any():
        i, h, d = (int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"variant {variant} n {n}: {int(bad.sum())} outputs differ from V[pi(i)], first at row "
                             f"{i} head {h} d {d}: got {got[i, h, d].item()}, want {want[i, h, d].item()} "
                             f"(key {int(c.pi[i, h])})")
