"""Tail split of the 256^2 GEMM (half-tile workgroups for a last round that fills at most half the
CUs) and the 16-byte epilogue forms of the residual+LayerNorm kernel: same bits as the unsplit /
8-byte forms, fp32 bounds of the existing GEMM tests, row tails untouched, repeatable bits."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def _rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401
    from libsplinter_amd.models.nomic import _lib
    return _lib()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def rope_tab():
    import torch
    from libsplinter_amd.models.nomic import NomicConfig
    cfg = NomicConfig()
    inv = cfg.rope_base ** (-np.arange(0, 64, 2) / 64)
    ang = np.arange(8192)[:, None] * inv[None, :]
    return torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32).reshape(8192, -1)).cuda()


def _split_tiles(T, cus):
    R = T % cus
    return R if 0 < R <= cus // 2 else 0


def _run(L, mode, split, x, w, M, N, K, out, ldo, tab=None, pos=None, rope_cols=0):
    """One launch on the 256^2 kernel with the tail split on / off."""
    import torch
    from libsplinter_amd.models.nomic import _chk, _stream
    pv = L.nomic_gemm_set_variant(256)
    ps = L.nomic_gemm_set_tail_split(1 if split else 0)
    try:
        grid = L.nomic_gemm256_grid(M, N)
        _chk(L.nomic_gemm(mode, x.data_ptr(), K, w.data_ptr(), K, M, N, K, out.data_ptr(), ldo, None, 0,
                          tab.data_ptr() if tab is not None else None, pos.data_ptr() if pos is not None else None,
                          rope_cols, _stream()), "gemm256")
        torch.cuda.synchronize()
    finally:
        L.nomic_gemm_set_tail_split(ps)
        L.nomic_gemm_set_variant(pv)
    return grid


def _check_split(L, cus, mode, M, N, K, ref_fn, ocols, seed, rope_tab=None, rope_cols=0, expect_split=True):
    import torch
    torch.manual_seed(seed)
    Mp = (M + 255) // 256 * 256
    T = (Mp // 256) * (N // 256)
    R = _split_tiles(T, cus)
    assert (R > 0) == expect_split, f"shape does not exercise what the case is about: T {T}, CUs {cus}"
    x = torch.randn(Mp, K, device="cuda").bfloat16()
    pos = torch.randint(0, 2000, (Mp,), device="cuda", dtype=torch.int32) if mode == 3 else None
    w, ref = ref_fn(x[:M].float(), pos[:M].long() if pos is not None else None)
    outs = []
    for split in (True, False, True, True):
        out = torch.full((Mp, ocols), SENTINEL, device="cuda", dtype=torch.bfloat16)
        grid = _run(L, mode, split, x, w, M, N, K, out, ocols, rope_tab if mode == 3 else None, pos, rope_cols)
        assert grid == T + (R if split else 0)
        outs.append(out)
    on, off = outs[0], outs[1]
    assert torch.equal(on, off), "split and unsplit launches must give the same bits"
    err = _rel(on[:M].float(), ref)
    print(f"mode {mode} M {M} N {N} K {K}: tiles {T} split {R} rel {err:.3e}")
    assert err < 1e-2
    assert (on[M:].float() == SENTINEL).all(), "rows past M must not be written"
    assert torch.equal(outs[2], on) and torch.equal(outs[3], on), "repeated launches must give the same bits"


def _rope_ref(N, K, rope_cols):
    import torch
    from libsplinter_amd.models.nomic import NomicConfig, NomicReference, pack_qkv

    def fn(xf, pos):
        wq = (torch.randn(N, K, device="cuda") * 0.03).bfloat16()
        raw = xf @ wq.float().T
        rot = NomicReference(NomicConfig(), {}, "cuda").rope(raw[:, :rope_cols].reshape(-1, rope_cols // 64, 64), pos)
        return pack_qkv(wq), torch.cat([rot.reshape(-1, rope_cols), raw[:, rope_cols:]], 1)
    return fn


def _store_ref(N, K):
    import torch

    def fn(xf, pos):
        w = (torch.randn(N, K, device="cuda") * 0.05).bfloat16()
        return w, xf @ w.float().T
    return fn


def _mixed_m(cus, want_split):
    """Row-tile count m of an N = 2304 grid (9 m tiles): a small remainder r = 9 m mod CUs > 0 (whole
    and half tiles in one launch), or a remainder the launch rule leaves alone (0 or > CUs / 2)."""
    for m in range(cus // 9 + 1, 4 * cus):
        R = 9 * m % cus
        if want_split and 0 < R <= min(8, cus // 2):
            return m
        if not want_split and (R == 0 or R > cus // 2):
            return m
    raise AssertionError("no such grid")


def test_tail_split_every_tile_rope_row_tail(L, cus, rope_tab):
    """Case a: 12 tiles, all split; rotated and unrotated heads; M = 1000 leaves a row tail."""
    _check_split(L, cus, 3, 1000, 768, 768, _rope_ref(768, 768, 512), 768, 11, rope_tab, 512)


@pytest.mark.parametrize("mode", [3, 0], ids=["rope", "store"])
def test_tail_split_whole_and_half_tiles(L, cus, rope_tab, mode):
    """Case b: whole tiles and a few split tiles in one launch (256 CUs: m = 29, 261 tiles, 5 split)."""
    m = _mixed_m(cus, True)
    ref = _rope_ref(2304, 768, 1536) if mode == 3 else _store_ref(2304, 768)
    _check_split(L, cus, mode, 256 * m - 100, 2304, 768, ref, 2304, 12 + mode, rope_tab, 1536)


def test_tail_split_swiglu(L, cus):
    """Case c: the SwiGLU epilogue on half tiles (32 tiles, all split)."""
    import torch
    from libsplinter_amd.models.nomic import pack_upgate
    K, F = 768, 1024

    def fn(xf, pos):
        up = torch.randn(F, K, device="cuda") * 0.03
        gate = torch.randn(F, K, device="cuda") * 0.03
        ref = (xf @ up.bfloat16().float().T) * torch.nn.functional.silu(xf @ gate.bfloat16().float().T)
        return pack_upgate(up, gate).bfloat16(), ref
    _check_split(L, cus, 2, 1000, 2 * F, K, fn, F, 13)


def test_tail_split_leaves_other_grids_alone(L, cus):
    """Case d: a remainder of 0 or of more than half the CUs keeps one block per tile."""
    m = _mixed_m(cus, False)
    _check_split(L, cus, 0, 256 * m - 100, 2304, 768, _store_ref(2304, 768), 2304, 14, expect_split=False)
    # the SwiGLU GEMM of the shipped shape (32768 x 6144: 3072 tiles on 256 CUs) is such a grid
    ps = L.nomic_gemm_set_tail_split(1)
    try:
        T = 128 * 24
        assert L.nomic_gemm256_grid(32768, 6144) == T + _split_tiles(T, cus)
        if cus == 256:
            assert L.nomic_gemm256_grid(32768, 6144) == 3072
            assert L.nomic_gemm256_grid(32768, 2304) == 1152 + 128
    finally:
        L.nomic_gemm_set_tail_split(ps)


# ---- residual + LayerNorm kernel: 16-byte epilogue forms ------------------------------------------

# (form, the 8-byte form it must match bit for bit): 242 = 222 with 16-B residual loads and stores
RLN_FORMS = [(242, 222)]


def _rln_operands(M, K, ld):
    import torch
    torch.manual_seed(M + K)
    N = 768
    Mp = (M + 127) // 128 * 128 + 128
    A = (torch.rand(Mp, K, device="cuda") * 2 - 1).bfloat16()
    W = ((torch.rand(N, K, device="cuda") * 2 - 1) * (1.0 / math.sqrt(K))).bfloat16()
    X = torch.zeros(Mp, ld, device="cuda", dtype=torch.bfloat16)
    X[:, :N] = (torch.randn(Mp, N, device="cuda") + torch.linspace(-2, 2, N, device="cuda")).bfloat16()
    g = (1 + 0.3 * torch.randn(N, device="cuda")).bfloat16()
    b = (0.1 * torch.randn(N, device="cuda")).bfloat16()
    ref = torch.nn.functional.layer_norm(A[:M].float() @ W.float().T + X[:M, :N].float(), (N,), g.float(), b.float(),
                                         1e-12)
    return A, W, X, g, b, ref


def _rln(L, variant, A, W, K, M, res, out, g, b):
    import torch
    from libsplinter_amd.models.nomic import _stream
    prev = L.nomic_gemm_res_ln_set_variant(variant)
    try:
        rc = L.nomic_gemm_res_ln(A.data_ptr(), K, W.data_ptr(), K, M, 768, K, res.data_ptr(), res.stride(0),
                                 g.data_ptr(), b.data_ptr(), 1e-12, out.data_ptr(), out.stride(0), _stream())
        torch.cuda.synchronize()
    finally:
        L.nomic_gemm_res_ln_set_variant(prev)
    return rc


@pytest.mark.parametrize("form,base", RLN_FORMS, ids=[f"rln{f}" for f, _ in RLN_FORMS])
@pytest.mark.parametrize("M,K", [(1, 768), (128, 768), (300, 768), (257, 3072)])
def test_rln_wide_epilogue_matches_8_byte_form(L, M, K, form, base):
    import torch
    A, W, X0, g, b, ref = _rln_operands(M, K, 768)
    got = {}
    for v in (base, form, form, form):
        # in place (out == res), then out of place from the same residual
        X = X0.clone()
        assert _rln(L, v, A, W, K, M, X, X, g, b) == 0
        Y = torch.full_like(X0, SENTINEL)
        assert _rln(L, v, A, W, K, M, X0, Y, g, b) == 0
        assert torch.equal(X[M:], X0[M:]), "rows past M must not be written"
        assert (Y[M:].float() == SENTINEL).all(), "rows past M must not be written"
        assert torch.equal(X[:M], Y[:M]), "in place and out of place must give the same bits"
        got.setdefault(v, []).append(X)
    want = got[base][0]
    assert _rel(want[:M].float(), ref) < 6e-3 and (want[:M].float() - ref).abs().max().item() < 0.08
    for X in got[form]:
        assert torch.equal(X, want), f"form {form} must give the bits of form {base}, launch after launch"


@pytest.mark.parametrize("form", [f for f, _ in RLN_FORMS])
def test_rln_rows_not_16_byte_aligned_run_the_8_byte_form(L, form):
    """ldr = ldo = 772 (a multiple of 4, not of 8): every other row starts 8 bytes off a 16-byte
    boundary; the call is taken and runs the 8-byte epilogue."""
    import torch
    M, K = 130, 768
    A, W, X, g, b, ref = _rln_operands(M, K, 772)
    tail, pad = X[M:].clone(), X[:, 768:].clone()
    assert _rln(L, form, A, W, K, M, X, X, g, b) == 0
    assert _rel(X[:M, :768].float(), ref) < 6e-3
    assert (X[:M, :768].float() - ref).abs().max().item() < 0.08
    assert torch.equal(X[M:], tail) and torch.equal(X[:, 768:], pad)


@pytest.mark.parametrize("K", [32, 64, 96, 128])
@pytest.mark.parametrize("M", [1, 129])
def test_rln_ring_edges_of_the_k_loop(L, M, K):
    """The shortest K walks of the ring loop k_gemm_rln shares with k_gemm384: 32 = one stage with
    nothing in flight behind it, 64 = the prologue issues alone, 96 = the first wrap of the W ring,
    128 = the first reuse of an A slot after a wrap; one row, and two tiles with a row tail.  Form 222
    against fp32 with the bounds of test_gemm_residual_layernorm_row_complete (a shorter K only lowers
    the error), form 242 the same bits, rows past M untouched."""
    import torch
    A, W, X0, g, b, ref = _rln_operands(M, K, 768)
    got = {}
    for v in (222, 242):
        X = X0.clone()
        assert _rln(L, v, A, W, K, M, X, X, g, b) == 0
        assert torch.equal(X[M:], X0[M:]), "rows past M must not be written"
        got[v] = X
    rel, err = _rel(got[222][:M].float(), ref), (got[222][:M].float() - ref).abs().max().item()
    print(f"rln ring edge M={M} K={K}: rel {rel:.3e} max abs {err:.3e}")
    assert rel < 6e-3 and err < 0.08
    assert torch.equal(got[242], got[222]), "form 242 must give the bits of form 222"
