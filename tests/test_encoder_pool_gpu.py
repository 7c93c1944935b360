"""Mean pool with the fused slot write (nomic_mean_pool, k_pool) called directly.

Numerics against the fp64 mean of the same bf16 inputs, under the bound of fp32 summation in ANY
order (so it does not lean on the kernel's wave tree): for a document of n rows, component c,

    |got - ref| <= n 2^-24 mean_t |x[t, c]|  +  4 2^-24 |ref|

(n - 1 additions of relative error 2^-24 each on partial sums no larger than sum_t |x|, divided by
n; the 1 / n and its product are two more roundings).  A dropped or doubled row of the 1000-row
document is about 16 times that.

The fused slot write is checked for its statuses and for what a refused slot keeps.  Status -11 (a
slot caught with an odd epoch) needs a writer holding the slot while the kernel runs; it is left
out here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 768
U = 2.0 ** -24
# around the kernel's stride of 16 waves x 4 unrolled rows
DOC_LENS = [1, 15, 16, 17, 63, 64, 65, 127, 1000]


def _pool(x, cu, normalize, arena=None, slots=None, hashes=None):
    import torch
    from libsplinter_amd import _native as N
    from libsplinter_amd.models.nomic import _chk, _lib, _stream
    B = cu.numel() - 1
    out = torch.full((B, D), float("nan"), dtype=torch.float32, device="cuda")
    status = torch.full((B,), 77, dtype=torch.int32, device="cuda") if arena is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _chk(_lib().nomic_mean_pool(x.data_ptr(), cu.data_ptr(), B, out.data_ptr(), int(normalize),
                                arena.desc if arena is not None else N.Arena(), ptr(slots), ptr(hashes), ptr(status),
                                _stream()), "mean_pool")
    torch.cuda.synchronize()
    return (out, status) if arena is not None else out


def _inputs(lens, seed):
    """bf16 x [T + 1, 768] with a per-column offset and a NaN row after the last document; cu by hand."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    T = sum(lens)
    x = torch.randn(T + 1, D, device="cuda", generator=g) + torch.linspace(-3, 3, D, device="cuda")
    x = x.to(torch.bfloat16)
    x[T] = float("nan")
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")
    return x, cu


def _ref(x, lens):
    """fp64 (mean, mean |x|) per document; an empty document has mean 0."""
    import torch
    ref = torch.zeros(len(lens), D, dtype=torch.float64, device="cuda")
    mabs = torch.zeros_like(ref)
    t = 0
    for i, n in enumerate(lens):
        if n:
            ref[i] = x[t:t + n].double().mean(0)
            mabs[i] = x[t:t + n].double().abs().mean(0)
        t += n
    return ref, mabs


def _check_numerics(lens, seed):
    import torch
    x, cu = _inputs(lens, seed)
    ref, mabs = _ref(x, lens)
    n = torch.tensor(lens, dtype=torch.float64, device="cuda")[:, None]
    tol = n * U * mabs + 4 * U * ref.abs()
    got = _pool(x, cu, 0).double()
    assert torch.isfinite(got).all(), "a NaN reached the output (a row past the last document was read?)"
    frac = ((got - ref).abs() / tol.clamp_min(1e-300)).max(1).values
    frac = torch.where(n[:, 0] > 0, frac, torch.zeros_like(frac))
    print(f"POOL lens={lens} normalize=0 worst error / bound per document: "
          f"{[round(f, 3) for f in frac.tolist()]}")
    assert ((got - ref).abs() <= tol).all(), f"worst error / bound per document {frac.tolist()} (lens {lens})"
    gotn = _pool(x, cu, 1).double()
    assert torch.isfinite(gotn).all()
    live = n[:, 0] > 0
    nrm = ref.norm(dim=1, keepdim=True)
    refn = ref / nrm.clamp_min(1e-300)
    toln = tol / nrm.clamp_min(1e-300) + 8 * U * refn.abs()
    fracn = ((gotn - refn).abs() / toln.clamp_min(1e-300)).max(1).values
    fracn = torch.where(live, fracn, torch.zeros_like(fracn))
    print(f"POOL lens={lens} normalize=1 worst error / bound per document: "
          f"{[round(f, 3) for f in fracn.tolist()]}; | ||v|| - 1 | max "
          f"{(gotn[live].norm(dim=1) - 1).abs().max().item():.2e}")
    assert ((gotn[live].norm(dim=1) - 1).abs() <= 1e-6).all(), gotn.norm(dim=1).tolist()
    assert ((gotn - refn).abs() <= toln)[live].all(), f"worst error / bound per document {fracn.tolist()}"
    return got, gotn, frac.max().item(), fracn.max().item()


def test_pool_numerics_document_lengths():
    """Lengths around the 16-wave x 4-row stride, and 1000 rows, in one launch; plain and normalised."""
    _check_numerics(DOC_LENS, 21)


def test_pool_empty_document():
    """cu with an empty document between two others (Batch forbids it; the kernel has an inv = 0
    arm): a finite all-zero row, plain and normalised, and the neighbours unharmed."""
    got, gotn, _, _ = _check_numerics([5, 0, 17], 22)
    assert (got[1] == 0).all() and (gotn[1] == 0).all()


def _arena_batch(a, n=6):
    """n keys set in the arena with a one-byte value; -> (keys, slot indices, hashes)."""
    import torch
    from libsplinter_amd.ops.arena import pack_keys, pack_values
    from libsplinter_amd.parallel.sharded import GpuShard
    K = pack_keys([f"pool{i}" for i in range(n)], 16)
    V, Ln = pack_values([b"v%d" % i for i in range(n)], 16)
    assert (a.set(K, V, Ln) == 0).all()
    st, idx = a.meta("find", K)
    hashes = GpuShard(a).hash_keys(K)
    torch.cuda.synchronize()
    assert (st == 0).all() and (idx >= 0).all()
    return K, idx, hashes


def test_pool_fused_slot_write_statuses(uniq):
    """Six documents: four with their slot and hash, one with slot -1, one with a wrong hash.  0 for
    the four, whose slot vectors are the returned vectors bit for bit; -2 for the two, and the
    wrong-hash key keeps its value and its vector and is left with an even epoch (a set and a get
    on it succeed).  (-11, a slot caught with an odd epoch, is not provoked here.)"""
    import torch
    from libsplinter_amd.ops.arena import HbmArena, pack_values, unpack
    a = HbmArena.create(uniq, slots=256, max_val=64, embeddings=True)
    try:
        K, idx, hashes = _arena_batch(a)
        known = torch.arange(2 * D, device="cuda", dtype=torch.float32).reshape(2, D) / 64 - 3
        assert (a.set_embeddings(K[4:], known) == 0).all()
        slots = idx.clone()
        slots[4] = -1
        bad = hashes.clone()
        bad[5] ^= 1
        _, ep0 = a.meta("epoch", K)
        for normalize in (0, 1):
            x, cu = _inputs([3, 70, 1, 16, 9, 20], 23)
            row4 = a.slot_view()[int(idx[4])].clone()
            vec, status = _pool(x, cu, normalize, a, slots, bad)
            assert status.tolist() == [0, 0, 0, 0, -2, -2], status.tolist()
            assert torch.equal(a.slot_view()[int(idx[4])], row4), "the slot of a document passed slot -1 changed"
            st, back = a.get_embeddings(K)
            torch.cuda.synchronize()
            assert (st == 0).all(), st.tolist()
            assert torch.equal(back[:4], vec[:4]), "slot vectors differ from the returned vectors"
            assert torch.equal(back[4:], known), "a refused slot's vector was written"
            ref, _ = _ref(x, [3, 70, 1, 16, 9, 20])
            if normalize:
                ref = ref / ref.norm(dim=1, keepdim=True)
            assert (vec.double() - ref).abs().max().item() < 1e-5      # the refused rows are still returned
        st, ep = a.meta("epoch", K)
        torch.cuda.synchronize()
        assert (st == 0).all() and (ep % 2 == 0).all(), ep.tolist()
        assert (ep[:4] > ep0[:4]).all() and ep[4] == ep0[4]
        st, val, ln = a.get(K)
        torch.cuda.synchronize()
        assert (st == 0).all() and unpack(val, ln) == [b"v%d" % i for i in range(6)]
        V, Ln = pack_values([b"again"], 16)
        assert (a.set(K[5:], V, Ln) == 0).all()
        st, val, ln = a.get(K[5:])
        torch.cuda.synchronize()
        assert (st == 0).all() and unpack(val, ln) == [b"again"]
    finally:
        a.close()


def test_pool_arena_without_embeddings_refuses(uniq):
    """An arena created without embeddings: -2 for every document, no byte of the slot array moves,
    and the pooled vectors are still returned."""
    import torch
    from libsplinter_amd.ops.arena import HbmArena
    a = HbmArena.create(uniq, slots=256, max_val=64, embeddings=False)
    try:
        assert not a.embeddings
        K, idx, hashes = _arena_batch(a, 4)
        before = a.slot_view().clone()
        x, cu = _inputs([2, 33, 64, 5], 24)
        vec, status = _pool(x, cu, 0, a, idx, hashes)
        assert status.tolist() == [-2] * 4, status.tolist()
        assert torch.equal(a.slot_view(), before), "a slot of an arena without embeddings was written"
        ref, _ = _ref(x, [2, 33, 64, 5])
        assert (vec.double() - ref).abs().max().item() < 1e-5
    finally:
        a.close()
