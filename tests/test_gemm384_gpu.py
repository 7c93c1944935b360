"""The 256x384 register-epilogue GEMM (gemm384.hip, NOMIC_GEMM=384) at the smallest shapes at which it
can go wrong: ring edges, tiles and row tails, the SwiGLU and RoPE epilogues, launch repeatability and
the launcher's fall-back.  Tolerances are those of the GEMM tests in test_nomic_gpu.py for each mode."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HIP_ERROR_INVALID_VALUE = 1


def _rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401
    from libsplinter_amd.models.nomic import _lib
    return _lib()


def _gemm(L, variant, mode, A, W, M, out, ldo, tab=None, pos=None, rope_cols=0):
    """One nomic_gemm launch on the forced kernel `variant`; returns the HIP status."""
    import torch
    from libsplinter_amd.models.nomic import _stream
    N, K = W.shape
    prev = L.nomic_gemm_set_variant(variant)
    try:
        rc = L.nomic_gemm(mode, A.data_ptr(), A.stride(0), W.data_ptr(), K, M, N, K, out.data_ptr(), ldo, None, 0,
                          tab.data_ptr() if tab is not None else None, pos.data_ptr() if pos is not None else None,
                          rope_cols, _stream())
        torch.cuda.synchronize()
    finally:
        L.nomic_gemm_set_variant(prev)
    return rc


def _operands(M, N, K, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    W = (torch.randn(N, K, device="cuda", generator=g) * 0.05).bfloat16()
    return A, W


@pytest.mark.parametrize("K", [64, 96, 768])
def test_ring_edges_store(L, K):
    """One tile; K = 64 is the prologue's two stages alone, 96 the first ring wrap.  Against fp32, and
    the same bits as the 128^2 kernel (both accumulate every element in ascending k, one 16x16x32
    MFMA per 32)."""
    import torch
    M, N = 256, 384
    A, W = _operands(M, N, K, 10 + K)
    ref = A.float() @ W.float().T
    out = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 384, 0, A, W, M, out, N) == 0
    assert _rel(out.float(), ref) < 5e-3
    if K % 64 == 0:  # the 128^2 kernel's K step
        o128 = torch.zeros_like(out)
        assert _gemm(L, 128, 0, A, W, M, o128, N) == 0
        d = (out.float() - o128.float()).abs().max().item()
        print(f"K={K}: max |gemm384 - gemm128| = {d}")
        assert torch.equal(out, o128)


def test_tiles_and_row_tail(L):
    """Two m-tiles with a row tail, two n-tiles; rows >= M of a pre-filled output stay untouched."""
    import torch
    M, N, K = 300, 768, 128
    A, W = _operands(512, N, K, 2)
    ref = A[:M].float() @ W.float().T
    out = torch.full((512, N), 7.0, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 384, 0, A, W, M, out, N) == 0
    assert _rel(out[:M].float(), ref) < 5e-3
    assert (out[M:].float() == 7.0).all(), "rows past M must not be written"
    o128 = torch.zeros_like(out)
    assert _gemm(L, 128, 0, A, W, M, o128, N) == 0
    assert torch.equal(out[:M], o128[:M])


def test_swiglu(L):
    """pack_upgate weights, an output leading dimension larger than N / 2; the columns past N / 2 of
    the pre-filled output stay untouched."""
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
    assert _gemm(L, 384, 2, x, ug, M, out, ldo) == 0
    assert _rel(out[:, :F].float(), ref) < 1e-2
    assert (out[:, F:].float() == 7.0).all()
    o128 = torch.full_like(out, 7.0)
    assert _gemm(L, 128, 2, x, ug, M, o128, ldo) == 0
    d = (out.float() - o128.float()).abs().max().item()
    print(f"swiglu: max |gemm384 - gemm128| = {d}")
    assert _rel(out[:, :F].float(), o128[:, :F].float()) < 1e-2


def test_rope(L):
    """pack_qkv weights, non-monotonic positions, rope_cols = 384: one rotated tile and one plain, a
    row tail in the second m-tile."""
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
    assert _gemm(L, 384, 3, x, wpk, M, out, N, tab, pos, rope_cols) == 0
    assert _rel(out[:M].float(), ref) < 1e-2
    assert _rel(out[:M, :rope_cols].float(), ref[:, :rope_cols]) < 1e-2
    assert _rel(out[:M, rope_cols:].float(), ref[:, rope_cols:]) < 1e-2
    assert (out[M:].float() == 7.0).all()
    o128 = torch.full_like(out, 7.0)
    assert _gemm(L, 128, 3, x, wpk, M, o128, N, tab, pos, rope_cols) == 0
    d = (out[:M].float() - o128[:M].float()).abs().max().item()
    print(f"rope: max |gemm384 - gemm128| = {d}")
    assert _rel(out[:M].float(), o128[:M].float()) < 1e-2


def test_launch_repeatability(L):
    """20 launches on the same operands write the same bits: a screen for a synchronisation slip in
    the ring (a stage read before it landed, or restaged before its last read)."""
    import torch
    M, N, K = 256, 384, 768
    A, W = _operands(M, N, K, 5)
    first = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 384, 0, A, W, M, first, N) == 0
    for i in range(20):
        out = torch.zeros_like(first)
        assert _gemm(L, 384, 0, A, W, M, out, N) == 0
        assert torch.equal(out, first), f"launch {i} differs"


def test_launcher_fallback_and_errors(L):
    """N = 512 is no multiple of 384: NOMIC_GEMM=384 runs the next kernel that takes the shape and
    matches; a K that no kernel takes is an error, not a launch."""
    import torch
    M, N, K = 256, 512, 128
    A, W = _operands(M, N, K, 6)
    ref = A.float() @ W.float().T
    out = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, 384, 0, A, W, M, out, N) == 0
    assert _rel(out.float(), ref) < 5e-3
    o128 = torch.zeros_like(out)
    assert _gemm(L, 128, 0, A, W, M, o128, N) == 0
    assert torch.equal(out, o128)
    A2, W2 = _operands(256, 384, 48, 7)
    assert _gemm(L, 384, 0, A2, W2, 256, torch.zeros(256, 384, device="cuda", dtype=torch.bfloat16), 384) \
        == HIP_ERROR_INVALID_VALUE
