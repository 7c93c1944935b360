"""Causal prefill attention over the KV cache (dec_attn_prefill_kv and dec_attn_prefill_kv_seg:
k_prefill_attn<64|128> and its PrefillSegs form) against fp64, every (row, head) on its own.

The cases, the fp64 reference, the emulated roundings and the check are those of tests/decoder_attn_ref.py;
tests/test_decoder_attn_ref_cpu.py shows that the same check rejects a causal mask that is off by one either
way.  Every launch runs under sentinels: `out` starts as NaN, its pad rows and pad columns must keep their
bits, q sits inside a wider row whose other columns are NaN, and the cache rows past the chunk hold NaN.

The geometry behind the case list: 128-row q-blocks of 4 waves x 32 rows (two 16-row halves), key tiles of
64 (head dim 64) and 32 (head dim 128) keys, the diagonal test at wave granularity, the deferred rescale
(the running maximum moves only past a margin of 8 log2 units) and the grid pushed through the XCD remap."""
import pytest

import decoder_attn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD_ROWS, PAD_COLS, GUARD = 3, 64, 8


@pytest.fixture(scope="module")
def lib():
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig
    return CausalLM.random(DecoderConfig(layers=1), seed=1, device=DEV).L


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


def _bits(t):
    import torch
    return t.view(torch.int16)


def _sync(name):
    """A fault ends the session: nothing more is started on a GPU that reported one."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{name}: the GPU reported '{e}'", 3)


def _run(lib, c):
    """One dec_attn_prefill_kv launch under the sentinels -> fp64 [n, H, hd]."""
    import torch
    n, H, KVH, hd, Lk = c.n, c.H, c.KVH, c.hd, c.pos0 + c.n
    W, ldq = H * hd, (H + 2 * KVH) * hd                     # q inside a fused q | k | v row
    qkv = _nan(n + PAD_ROWS, ldq)
    qkv[:n, :W] = c.q.reshape(n, W)
    kv = _nan(2, Lk + GUARD, KVH, hd)
    kv[0, :Lk], kv[1, :Lk] = c.K, c.V
    out = _nan(n + PAD_ROWS, W + PAD_COLS)
    sentinel = _bits(out).clone()
    rc = lib.dec_attn_prefill_kv(qkv.data_ptr(), ldq, kv[0].data_ptr(), kv[1].data_ptr(), KVH * hd, n, c.pos0, H, KVH,
                                 hd, c.scale, out.data_ptr(), W + PAD_COLS, None)
    assert rc == 0, (c.name, rc)
    _sync(c.name)
    assert torch.equal(_bits(out)[n:], sentinel[n:]), f"{c.name}: rows past the chunk were written"
    assert torch.equal(_bits(out)[:, W:], sentinel[:, W:]), f"{c.name}: pad columns of out were written"
    return out[:n, :W].double().reshape(n, H, hd)


@pytest.mark.parametrize("fill", R.PREFILL_FILLS)
@pytest.mark.parametrize("hd,H,KVH", R.PREFILL_SHAPES)
def test_chunks(lib, hd, H, KVH, fill):
    """The 14 (n, pos0) chunks round the 16 / 32-row and 128-row query edges and the key-tile edges, groups of
    1 and 4.  One-hot targets: the row's own position (the diagonal key must be seen: exact), p + 1 (it must
    not be: the reference is the softmax over the allowed keys, a leak lands on code(p + 1)), key 0, and the
    first key of the row's last key tile."""
    for n, pos0 in R.PREFILL_NP:
        c = R.prefill_case(fill, hd, H, KVH, n, pos0, DEV)
        c.check(_run(lib, c))


@pytest.mark.parametrize("ramp", list(R.PREFILL_RAMPS))
@pytest.mark.parametrize("hd,H,KVH", R.PREFILL_SHAPES)
def test_deferred_rescale(lib, hd, H, KVH, ramp):
    """Every row's maximum score rises by just under 8 log2 units per key tile (the rescale of O and l is put off
    for a tile, P reaches 2^7.5 in bf16), by just over 8 (it happens on every tile), or falls."""
    lo, hi = {"under8": (7.0, 8.0), "over8": (8.0, 9.0), "falling": (-8.0, -7.0)}[ramp]
    for n, pos0 in R.PREFILL_RAMP_NP:
        c = R.prefill_ramp_case(ramp, hd, H, KVH, n, pos0, DEV)
        d = R.tile_steps(c)       # from the inputs: the case sits on its side of the margin
        assert lo < d.min().item() and d.max().item() < hi, (ramp, d.min().item(), d.max().item())
        c.check(_run(lib, c))


@pytest.mark.parametrize("heads,nqb", R.REMAP_TABLE)
def test_heads_and_xcd_remap(lib, heads, nqb):
    """1, 2, 3, 5 and 12 heads over 3, 6 and 7 q-blocks: heads x q-blocks workgroups reach every residue modulo 8
    and one grid below 8.  A workgroup map that is not a bijection leaves a (row, head) at the sentinel or
    answers it from another block's rows, which the one-hot rows (target = own position) show exactly."""
    R.remap_coverage()
    n = 128 * nqb - 28
    assert (n + 127) // 128 == nqb
    for fill in ("gauss", "onehot_self"):
        c = R.prefill_case(fill, 64, heads, heads, n, 5, DEV)
        c.check(_run(lib, c))


@pytest.mark.parametrize("fill", ["gauss", "onehot_self"])
@pytest.mark.parametrize("hd,H,KVH", R.PREFILL_SHAPES)
def test_segments(lib, hd, H, KVH, fill):
    """dec_attn_prefill_kv_seg: three segments of 1, 129 and 33 rows in slots 3, 0 and 2 (slot 1 unused), packed
    with gaps, each against its own fp64 reference; one-hot caches carry the slot's code offset.  (Bit identity
    with the single-chunk kernel is tests/test_prefill_batch_gpu.py.)"""
    import numpy as np
    import torch
    cases = [R.prefill_case(fill, hd, H, KVH, n, pos0, DEV, offset=R.SLOT_CODE_STEP * slot, seed=slot)
             for _, n, pos0, slot in R.SEGS]
    W, ldq, T = H * hd, (H + 2 * KVH) * hd, R.SEG_T
    qkv = _nan(T, ldq)
    kv = _nan(R.SEG_SLOTS, 2, R.SEG_CTX, KVH, hd)
    owned = torch.zeros(T, dtype=torch.bool, device=DEV)
    for c, (row0, n, pos0, slot) in zip(cases, R.SEGS):
        qkv[row0:row0 + n, :W] = c.q.reshape(n, W)
        kv[slot, 0, :pos0 + n], kv[slot, 1, :pos0 + n] = c.K, c.V
        assert not owned[row0:row0 + n].any()
        owned[row0:row0 + n] = True
    assert not owned[0] and not owned[-1] and int(owned.int().diff().abs().sum()) == 2 * len(R.SEGS), "no gaps"
    out = _nan(T, W + PAD_COLS)
    sentinel = _bits(out).clone()
    tb = np.ascontiguousarray(np.array(R.SEGS, dtype=np.int32).reshape(-1, 4))
    rc = lib.dec_attn_prefill_kv_seg(qkv.data_ptr(), ldq, T, tb.ctypes.data, len(R.SEGS), kv[0, 0].data_ptr(),
                                     kv[0, 1].data_ptr(), KVH * hd, kv.stride(0), R.SEG_SLOTS, R.SEG_CTX, H, KVH, hd,
                                     hd ** -0.5, out.data_ptr(), W + PAD_COLS, None)
    assert rc == 0, rc
    _sync("segments")
    assert torch.equal(_bits(out)[~owned], sentinel[~owned]), "a gap row of out was written"
    assert torch.equal(_bits(out)[:, W:], sentinel[:, W:]), "pad columns of out were written"
    for c, (row0, n, pos0, slot) in zip(cases, R.SEGS):
        c.check(out[row0:row0 + n, :W].double().reshape(n, H, hd), f"seg_slot{slot}_{c.name}")
