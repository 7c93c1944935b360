"""The 64-wide K stages of the 256x384 GEMM (gemm384.hip, nomic_gemm384_set_bk) at the smallest shapes at
which the two-slot ring can go wrong.  Every case is held against fp32 with the tolerances of
test_gemm384_gpu.py and must write the bits of the 32-wide loop: both accumulate every element in ascending
k, one 16x16x32 MFMA per 32, and share the epilogue code."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401
    from libsplinter_amd.models.nomic import _lib
    return _lib()


def _gemm(L, bk, mode, A, W, M, out, ldo, tab=None, pos=None, rope_cols=0):
    """One nomic_gemm launch on the 256x384 kernel with the stage-width knob at `bk`; the HIP status."""
    import torch
    from libsplinter_amd.models.nomic import _stream
    N, K = W.shape
    prev = L.nomic_gemm_set_variant(384)
    prev_bk = L.nomic_gemm384_set_bk(bk)
    try:
        rc = L.nomic_gemm(mode, A.data_ptr(), A.stride(0), W.data_ptr(), K, M, N, K, out.data_ptr(), ldo, None, 0,
                          tab.data_ptr() if tab is not None else None, pos.data_ptr() if pos is not None else None,
                          rope_cols, _stream())
        torch.cuda.synchronize()
    finally:
        L.nomic_gemm384_set_bk(prev_bk)
        L.nomic_gemm_set_variant(prev)
    return rc


def _operands(M, N, K, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    W = (torch.randn(N, K, device="cuda", generator=g) * 0.05).bfloat16()
    return A, W


def test_set_bk_returns_previous(L):
    prev = L.nomic_gemm384_set_bk(32)
    try:
        assert prev in (32, 64)
        assert L.nomic_gemm384_set_bk(64) == 32
        assert L.nomic_gemm384_set_bk(64) == 64
    finally:
        L.nomic_gemm384_set_bk(prev)


@pytest.mark.parametrize("K", [64, 128, 192])
def test_ring_edges_store(L, K):
    """One tile; K = 64 is the prologue stage alone, 128 fills both slots, 192 reuses the first."""
    import torch
    M, N = 256, 384
    A, W = _operands(M, N, K, 20 + K)
    ref = A.float() @ W.float().T
    out = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 64, 0, A, W, M, out, N) == 0
    assert _rel(out.float(), ref) < 5e-3
    o32 = torch.zeros_like(out)
    assert _gemm(L, 32, 0, A, W, M, o32, N) == 0
    assert torch.equal(out, o32)


def test_tiles_and_row_tail(L):
    """Two m-tiles with a row tail, two n-tiles; rows >= M of a pre-filled output stay untouched."""
    import torch
    M, N, K = 300, 768, 128
    A, W = _operands(512, N, K, 2)
    ref = A[:M].float() @ W.float().T
    out = torch.full((512, N), 7.0, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 64, 0, A, W, M, out, N) == 0
    assert _rel(out[:M].float(), ref) < 5e-3
    assert (out[M:].float() == 7.0).all(), "rows past M must not be written"
    o32 = torch.full_like(out, 7.0)
    assert _gemm(L, 32, 0, A, W, M, o32, N) == 0
    assert torch.equal(out, o32)


def test_swiglu(L):
    """pack_upgate weights, an output leading dimension larger than F; the columns past F stay untouched."""
    import torch
    from libsplinter_amd.models.nomic import pack_upgate
    torch.manual_seed(3)
    M, K, F, ldo = 256, 128, 384, 392
    x = torch.randn(M, K, device="cuda").bfloat16()
    up = torch.randn(F, K, device="cuda") * 0.05
    gate = torch.randn(F, K, device="cuda") * 0.05
    ug = pack_upgate(up, gate).bfloat16().contiguous()
    xf = x.float()
    ref = (xf @ up.bfloat16().float().T) * torch.nn.functional.silu(xf @ gate.bfloat16().float().T)
    out = torch.full((M, ldo), 7.0, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 64, 2, x, ug, M, out, ldo) == 0
    assert _rel(out[:, :F].float(), ref) < 1e-2
    assert (out[:, F:].float() == 7.0).all()
    o32 = torch.full_like(out, 7.0)
    assert _gemm(L, 32, 2, x, ug, M, o32, ldo) == 0
    assert torch.equal(out, o32)


def test_rope(L):
    """pack_qkv weights, non-monotonic positions, rope_cols = 384: one rotated tile and one plain, a row
    tail in the second m-tile."""
    import torch
    from libsplinter_amd.models.nomic import NomicConfig, NomicReference, pack_qkv
    torch.manual_seed(4)
    M, N, K, rope_cols = 320, 768, 128, 384
    x = torch.randn(512, K, device="cuda").bfloat16()
    w = (torch.randn(N, K, device="cuda") * 0.05).bfloat16()
    pos = ((torch.arange(512, device="cuda") * 37 + 11) % 1999).to(torch.int32).contiguous()
    cfg = NomicConfig()
    inv = cfg.rope_base ** (-np.arange(0, 64, 2) / 64)
    ang = np.arange(2048)[:, None] * inv[None, :]
    tab = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32).reshape(2048, -1)).cuda()
    wpk = pack_qkv(w).contiguous()
    raw = x[:M].float() @ w.float().T
    rot = NomicReference(cfg, {}, "cuda").rope(raw[:, :rope_cols].reshape(M, rope_cols // 64, 64), pos[:M].long())
    ref = torch.cat([rot.reshape(M, rope_cols), raw[:, rope_cols:]], 1)
    out = torch.full((512, N), 7.0, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 64, 3, x, wpk, M, out, N, tab, pos, rope_cols) == 0
    assert _rel(out[:M].float(), ref) < 1e-2
    assert _rel(out[:M, :rope_cols].float(), ref[:, :rope_cols]) < 1e-2
    assert _rel(out[:M, rope_cols:].float(), ref[:, rope_cols:]) < 1e-2
    assert (out[M:].float() == 7.0).all()
    o32 = torch.full_like(out, 7.0)
    assert _gemm(L, 32, 3, x, wpk, M, o32, N, tab, pos, rope_cols) == 0
    assert torch.equal(out, o32)


def test_k96_keeps_the_32_wide_loop(L):
    """K = 96 is no multiple of 64: with the knob at 64 the launch succeeds on the 32-wide loop and writes
    the bits it writes with the knob at 32."""
    import torch
    M, N, K = 256, 384, 96
    A, W = _operands(M, N, K, 8)
    ref = A.float() @ W.float().T
    out = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 64, 0, A, W, M, out, N) == 0
    assert _rel(out.float(), ref) < 5e-3
    o32 = torch.zeros_like(out)
    assert _gemm(L, 32, 0, A, W, M, o32, N) == 0
    assert torch.equal(out, o32)


def test_launch_repeatability(L):
    """20 launches on the same operands write the same bits: a screen for a stage read before it landed
    or restaged before its last read."""
    import torch
    M, N, K = 256, 384, 768
    A, W = _operands(M, N, K, 5)
    first = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 64, 0, A, W, M, first, N) == 0
    assert _rel(first.float(), A.float() @ W.float().T) < 5e-3
    o32 = torch.zeros_like(first)
    assert _gemm(L, 32, 0, A, W, M, o32, N) == 0
    assert torch.equal(first, o32)
    for i in range(20):
        out = torch.zeros_like(first)
        assert _gemm(L, 64, 0, A, W, M, out, N) == 0
        assert torch.equal(out, first), f"launch {i} differs"
