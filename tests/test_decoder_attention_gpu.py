"""Decode attention (dec_attn_decode / _st / _ws and dec_attn_decode_b: k_attn_decode_g, k_attn_decode,
k_attn_decode_split, k_attn_combine and their slot forms) against fp64, head by head.

The cases, the fp64 reference, the emulated roundings and the per-(row, head) check are those of
tests/decoder_attn_ref.py; tests/test_decoder_attn_ref_cpu.py shows on the CPU that the same check rejects a
dropped key, chunk or split, a key past the length, a neighbour's KV head, swapped heads and shifted V rows.

Every launch runs under sentinels: `out` starts as NaN and every real (row, head) must come back finite;
the rows and pad columns of `out` no launch owns must keep their bits; the cache rows at and past the length
hold NaN, so no value from them may reach an output.  The lengths sit on the kernels' strides: the 256 / 128 /
64-key pass of k_attn_decode_g, the 64-key wave chunk, the 4 x 64 and 16 x 64 workgroup strides, the 512-key
limit of the single workgroup and chunk = roundup64(ceil(L / S)) of the splits."""
import pytest

import decoder_attn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ST = 8      # int32 words of a slot's state record: pos, token, step, active, seed lo, seed hi, 0, 0
GUARD = 8   # NaN cache rows past the last row a launch may read


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


def _run_single(lib, c, cap=None):
    """Every launch of a single-slot case through dec_attn_decode (host-side length), or dec_attn_decode_st
    with the length on the device and the launch sized for `cap` rows -> fp64 [launches, 1, H, hd]."""
    import torch
    K, V, L = c.slots[0]
    H, KVH, hd = c.H, c.KVH, c.hd
    kv = _nan(2, (cap or L) + GUARD, KVH, hd)
    kv[0, :L], kv[1, :L] = K[:L], V[:L]
    q = c.q[:, 0].contiguous()
    out = _nan(c.nl, 2, H * hd)                 # row 0: the launch's output, row 1: must stay as it is
    sentinel = _bits(out).clone()
    st = torch.tensor([L - 1, 0, 0, 0], dtype=torch.int32, device=DEV)
    for i in range(c.nl):
        if cap is None:
            rc = lib.dec_attn_decode(q[i].data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), KVH * hd, L, H, KVH, hd,
                                     c.scale, out[i].data_ptr(), None)
        else:
            rc = lib.dec_attn_decode_st(q[i].data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), KVH * hd, cap, H, KVH, hd,
                                        c.scale, out[i].data_ptr(), st.data_ptr(), None)
        assert rc == 0, (c.name, i, rc)
    _sync(c.name)
    assert torch.equal(_bits(out)[:, 1], sentinel[:, 1]), f"{c.name}: the row after the output row was written"
    assert bool(kv[:, L:].isnan().all()), f"{c.name}: cache rows past the length were written"
    return out[:, :1].double().reshape(c.nl, 1, H, hd)


def _state(rows):
    import torch
    st = torch.zeros((len(rows), ST), dtype=torch.int32)
    for b, (pos, act) in enumerate(rows):
        st[b, 0], st[b, 3] = pos, act
    return st.to(DEV)


def _run_batch(lib, c, span):
    """Every launch of a batched case through dec_attn_decode_b sized for `span` keys; q and out rows are
    64 elements wider than H * hd and out has one row more than there are slots."""
    import torch
    H, KVH, hd, ns = c.H, c.KVH, c.hd, c.ns
    W = H * hd
    kv = _nan(ns, 2, span + GUARD, KVH, hd)
    for b, s in enumerate(c.slots):
        if s is not None:
            kv[b, 0, :s[2]], kv[b, 1, :s[2]] = s[0][:s[2]], s[1][:s[2]]
    q = _nan(c.nl, ns, W + 64)
    q[:, :, :W] = c.q.reshape(c.nl, ns, W)
    out = _nan(c.nl, ns + 1, W + 64)
    sentinel = _bits(out).clone()
    st = _state([(s[2] - 1, 1) if s is not None else (99, 0) for s in c.slots])
    ws = torch.empty(lib.dec_attn_b_ws_floats(ns, H, hd), dtype=torch.float32, device=DEV)
    for i in range(c.nl):
        rc = lib.dec_attn_decode_b(q[i].data_ptr(), W + 64, kv[0, 0].data_ptr(), kv[0, 1].data_ptr(), KVH * hd,
                                   kv.stride(0), span, ns, H, KVH, hd, c.scale, out[i].data_ptr(), W + 64,
                                   st.data_ptr(), ws.data_ptr(), None)
        assert rc == 0, (c.name, i, rc)
    _sync(c.name)
    assert torch.equal(_bits(out)[:, :, W:], sentinel[:, :, W:]), f"{c.name}: pad columns of out were written"
    assert torch.equal(_bits(out)[:, ns], sentinel[:, ns]), f"{c.name}: the row after the last slot was written"
    dead = [b for b in range(ns) if c.slots[b] is None]
    assert dead and torch.equal(_bits(out)[:, dead], sentinel[:, dead]), f"{c.name}: an inactive slot's row was written"
    return out[:, :ns, :W].double().reshape(c.nl, ns, H, hd)


# -------------------------------------------------------------------- tests --
@pytest.mark.parametrize("hd,g", R.GROUPED + R.WALKING)
def test_short_caches(lib, hd, g):
    """Up to 512 keys: k_attn_decode_g<D, G, false> for the twelve grouped shapes, k_attn_decode<D> for head dim
    192 and a group of 3.  Gaussian inputs, and one-hot probes of EVERY key of the cache (128 query heads a
    launch), at the 22 lengths round the kernels' strides; V rows shifted by one code at 257 keys."""
    for c in R.short_cases(hd, g, DEV):
        c.check(_run_single(lib, c))


@pytest.mark.parametrize("hd,g", R.GROUPED + R.WALKING)
def test_split_form(lib, hd, g):
    """Past 512 keys: k_attn_decode_g<D, G, true> + k_attn_combine up to 16384 keys, k_attn_decode_split<D, G>
    beyond (chunks longer than 512 keys) and at every length for head dim 192 and a group of 3.  Gaussian,
    peaked, rising and falling scores; one-hot probes of every key up to 2048 keys, of the split edges beyond."""
    ranges = R.split_ranges(8193)
    assert len(ranges) == 32 and any(a >= 8193 for a, _ in ranges), "8193 keys must leave a split that starts past L"
    for c in R.split_cases(hd, g, DEV):
        c.check(_run_single(lib, c))


@pytest.mark.parametrize("hd,g", R.GROUPED + R.WALKING)
def test_device_side_length(lib, hd, g):
    """dec_attn_decode_st: the length is read on the device, the launch is sized for the capacity, and the NaN
    rows between the two lie inside the range the launch was sized for."""
    for c, cap in R.devlen_cases(hd, g, DEV):
        c.check(_run_single(lib, c, cap))


def test_more_than_128_heads(lib):
    """136 heads over 17 KV heads: no split workspace for more than 128 heads, so caches past 512 keys run the
    16-wave walking kernel, whose waves then stride past 1024 keys."""
    for c in R.wide_cases(DEV):
        c.check(_run_single(lib, c))


@pytest.mark.parametrize("span", list(R.BATCH_SPANS))
@pytest.mark.parametrize("hd,H,KVH", R.BATCH_SHAPES)
def test_batched(lib, hd, H, KVH, span):
    """dec_attn_decode_b, seven slots with one inactive between live ones, every slot against its own fp64
    reference: gaussian caches, and one-hot caches with the slot's own code offset (a slot answering from
    another slot's cache fails the equality)."""
    for fill in ("gauss", "onehot"):
        c = R.batch_case(fill, hd, H, KVH, span, DEV)
        assert [s[2] if s else None for s in c.slots] == R.BATCH_SPANS[span]
        c.check(_run_batch(lib, c, span))


def test_refusals_launch_nothing(lib):
    """Every refusal the launchers make returns non-zero and leaves `out` as it was."""
    import torch
    hd, H, KVH, L = 64, 8, 2, 100
    kv = _nan(2, L + 1, KVH, hd)
    kv[:, :L] = 1.0
    q = torch.ones(2, H * hd + 64, dtype=torch.bfloat16, device=DEV)
    out = _nan(2, H * hd + 64)
    sentinel = _bits(out).clone()
    k, v, qp, op = kv[0].data_ptr(), kv[1].data_ptr(), q.data_ptr(), out.data_ptr()

    def single(q_=qp, k_=k, v_=v, ldkv=KVH * hd, H_=H, KVH_=KVH, hd_=hd):
        return lib.dec_attn_decode(q_, k_, v_, ldkv, L, H_, KVH_, hd_, 0.125, op, None)

    bad = {"head dim 96": single(hd_=96), "H % KVH": single(H_=7), "ldkv < KVH * hd": single(ldkv=KVH * hd - 8),
           "ldkv % 8": single(ldkv=KVH * hd + 4), "misaligned k": single(k_=k + 2), "misaligned v": single(v_=v + 8),
           "misaligned q": single(q_=qp + 2),
           "L = 0": lib.dec_attn_decode(qp, k, v, KVH * hd, 0, H, KVH, hd, 0.125, op, None)}
    st = _state([(L - 1, 1), (L - 1, 1)])
    ws = torch.empty(lib.dec_attn_b_ws_floats(16, H, hd), dtype=torch.float32, device=DEV)

    def batch(nseq=2, st_=st.data_ptr(), ws_=ws.data_ptr(), q_=qp, hd_=hd):
        return lib.dec_attn_decode_b(q_, q.stride(0), k, v, KVH * hd, 0, L, nseq, H, KVH, hd_, 0.125, op, out.stride(0),
                                     st_, ws_, None)

    bad.update({"batch: nseq 0": batch(nseq=0), "batch: nseq 17": batch(nseq=17), "batch: null st": batch(st_=None),
                "batch: null ws": batch(ws_=None), "batch: misaligned q": batch(q_=qp + 2),
                "batch: head dim 96": batch(hd_=96)})
    torch.cuda.synchronize()
    for what, rc in bad.items():
        assert rc != 0, f"{what}: not refused"
    assert torch.equal(_bits(out), sentinel), "a refused call wrote to out"
    assert single() == 0 and batch() == 0     # the same arguments without the fault are accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:, : H * hd].float()).all())
