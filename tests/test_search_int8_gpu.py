"""The opt-in int8 candidate copy of an HBM arena (SPLINTER_HBM_VEC8=1; csrc/include/splinter_layout.hpp,
csrc/hip/search_kernels.hip side::OpInt8): every vector writer keeps the int8 row and its rigorous per-row
error bound in step with the fp32 vector, the int8 MFMA pass computes exactly the integer dot
products and the bound the layout defines, and the batched search on it returns the exact fp32
kernel's result -- from Python, from the C ABI and from a node whose shards do not all carry the copy."""
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
SLACK = 4e-4 + 2e-6  # the epilogue's constant terms of B


def _keys(ids):
    import torch
    from libsplinter_amd.ops.arena import format_keys
    return format_keys(len(ids), "c", 9, 16, ids=torch.as_tensor(ids, device="cuda"))


def _key_str(K, i):
    return bytes(K[i].cpu().numpy()).split(b"\0", 1)[0].decode()


def _clustered(n, g, centers=64, noise=0.35):
    import torch
    c = torch.randn(centers, 768, generator=g)
    lab = torch.randint(0, centers, (n,), generator=g)
    return c[lab] + noise * torch.randn(n, 768, generator=g)


def _check_copy(ar, slots, what):
    """The int8 rows of `slots` against the fp32 vectors the same slots hold, in float64: the code
    range, the rounding of every code, and the stored bound -- never below the true error (the
    property the search's exactness rests on), and not wastefully above it."""
    import torch
    torch.cuda.synchronize()
    meta, v8 = ar.vec8_view()
    sl = torch.as_tensor(np.asarray(slots), device="cuda").long()
    v = ar.embedding_matrix()[sl].double().cpu().numpy()
    c = v8[sl].cpu().numpy().astype(np.float64)
    rs = meta[sl, 0].double().cpu().numpy()
    err = meta[sl, 1].double().cpu().numpy()
    vh = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert np.abs(c).max() <= 127, what
    assert (rs > 0).all(), what
    step = np.abs(c * rs[:, None] - vh)
    assert (step <= 0.5 * rs[:, None] * (1 + 1e-3) + 1e-7).all(), (what, float(step.max()))
    true = np.linalg.norm(vh - c * rs[:, None], axis=1)
    assert (err >= true).all(), (what, float((true - err).max()))
    assert (err <= 1.01 * true + 2e-6).all(), (what, float((err - 1.01 * true).max()))


def _meta_of(ar, slots):
    import torch
    torch.cuda.synchronize()
    meta, _ = ar.vec8_view()
    return meta[torch.as_tensor(np.asarray(slots), device="cuda").long()].cpu().numpy()


def test_int8_copy_follows_every_vector_writer(uniq, monkeypatch):
    import torch
    from libsplinter_amd.models.nomic import smoke_embed
    from libsplinter_amd.ops.arena import HbmArena, format_values
    monkeypatch.setenv("SPLINTER_HBM_VEC8", "1")
    ar = HbmArena.create(f"{uniq}", slots=4096, max_val=64, embeddings=True)
    try:
        assert ar.has_vec8 and ar.has_vec16
        meta, v8 = ar.vec8_view()
        assert meta.shape == (4096, 2) and v8.shape == (4096, 768) and v8.dtype == torch.int8
        torch.cuda.synchronize()
        assert bool((meta[:, 0] == 0).all()) and bool((meta[:, 1] == -1).all())  # a fresh arena: no vector anywhere
        ids = np.arange(300)
        K = _keys(ids)
        V, Lv = format_values(300, 1, 32, 64, ids=torch.as_tensor(ids, device="cuda"))
        assert int((ar.set(K, V, Lv) != 0).sum()) == 0
        g = torch.Generator().manual_seed(5)
        vec = torch.randn(300, 768, generator=g) * torch.rand(300, 1, generator=g) * 4 + 0.1
        vec[40:50, ::97] *= 40.0  # outlier dimensions: a coarse scale, a large error bound
        vec[3] = 0
        vec[4] = 1e-8  # below the exact kernel's norm floor
        vec = vec.cuda()
        assert int((ar.set_embeddings(K, vec) != 0).sum()) == 0  # batched writer (k_embed_set)
        st, idx = ar.meta("find", K)
        torch.cuda.synchronize()
        sl = idx.long().cpu().numpy()
        good = np.setdiff1d(np.arange(300), [3, 4])
        assert torch.equal(ar.embedding_matrix()[idx.long()], vec)
        _check_copy(ar, sl[good], "batched writer")
        assert _meta_of(ar, sl[[3, 4]]).tolist() == [[0.0, -1.0], [0.0, 2.0]]
        # per-call writer (the ring worker) through the Store API
        s = ar.store
        one = (np.random.default_rng(1).standard_normal(768) * 3 + 0.5).astype(np.float32)
        s.set_embedding(_key_str(K, 7), one)
        torch.cuda.synchronize()
        assert np.array_equal(ar.embedding_matrix()[sl[7]].cpu().numpy(), one)
        _check_copy(ar, sl[[7]], "ring writer")
        s.set_embedding(_key_str(K, 8), np.full(768, 1e-8, np.float32))
        s.set_embedding(_key_str(K, 6), np.zeros(768, np.float32))
        assert _meta_of(ar, sl[[6, 8]]).tolist() == [[0.0, -1.0], [0.0, 2.0]]
        # the encoder's fused mean-pool write-back
        smoke_embed(ar, K[20:24])
        _check_copy(ar, sl[20:24], "encoder pool writer")
        # unset and retrain leave "no vector"
        assert int((ar.unset(K[:5]) < 0).sum()) == 0
        assert s.retrain(_key_str(K, 9))
        assert (_meta_of(ar, np.r_[sl[:5], sl[9]]) == np.array([0.0, -1.0], np.float32)).all()
        # checkpoint / restore rebuilds the copy from the restored vectors (it is not in the file)
        path = os.path.join(tempfile.mkdtemp(), "ck.spl")
        ar.checkpoint(path)
        meta.fill_(7.0)
        v8.zero_()
        ar.restore(path)
        live = np.r_[7, np.arange(10, 300)]  # keys 0-4 unset, 6 zero, 8 tiny, 9 retrained
        _check_copy(ar, sl[live], "restore")
        assert (_meta_of(ar, np.r_[sl[:5], sl[6], sl[9]]) == np.array([0.0, -1.0], np.float32)).all()
        assert _meta_of(ar, sl[[8]]).tolist() == [[0.0, 2.0]]
        # online rehash after unsetting a third of the keys: moved keys keep a valid copy
        gone = np.arange(10, 300, 3)
        assert int((ar.unset(K[torch.as_tensor(gone, device="cuda")]) < 0).sum()) == 0
        keep = np.setdiff1d(live, gone)
        before = ar.embedding_matrix()[torch.as_tensor(sl[keep], device="cuda")].clone()
        ar.store.rehash()
        st, idx2 = ar.meta("find", K[torch.as_tensor(keep, device="cuda")])
        torch.cuda.synchronize()
        assert bool((st == 0).all())
        sl2 = idx2.long().cpu().numpy()
        assert torch.equal(ar.embedding_matrix()[idx2.long()], before)
        _check_copy(ar, sl2, "rehash")
        # ... and every slot without a key says "no vector"
        h = ar.slot_view()[:, :8].contiguous().cpu().numpy().view(np.uint64).ravel()
        assert (_meta_of(ar, np.nonzero(h == 0)[0]) == np.array([0.0, -1.0], np.float32)).all()
        # the exclusive full rebuild carries rows and meta with the keys too
        ar.store.rehash(full=True)
        st, idx3 = ar.meta("find", K[torch.as_tensor(keep, device="cuda")])
        torch.cuda.synchronize()
        assert bool((st == 0).all())
        _check_copy(ar, idx3.long().cpu().numpy(), "full rebuild")
        h = ar.slot_view()[:, :8].contiguous().cpu().numpy().view(np.uint64).ravel()
        assert (_meta_of(ar, np.nonzero(h == 0)[0]) == np.array([0.0, -1.0], np.float32)).all()
    finally:
        ar.close()


def test_int8_pass_operand_map_and_epilogue_exact(uniq, monkeypatch):
    """The threshold-sample pass against the integer dot products of the stored codes: every per-tile
    maximum of approx - B, over a partial last tile, rows without codes and asymmetric data from
    different seeds.  A wrong lane map, or rows and queries swapped, cannot reproduce them."""
    import torch
    from libsplinter_amd.ops.arena import HbmArena, format_values
    from libsplinter_amd.ops.search import VectorSearch
    monkeypatch.setenv("SPLINTER_HBM_VEC8", "1")
    slots, n, nq = 1024 + 37, 600, 48
    ar = HbmArena.create(f"{uniq}", slots=slots, max_val=32, embeddings=True)
    try:
        ids = np.arange(n)
        K = _keys(ids)
        V, Lv = format_values(n, 1, 16, 32, ids=torch.as_tensor(ids, device="cuda"))
        assert int((ar.set(K, V, Lv) != 0).sum()) == 0
        g = torch.Generator().manual_seed(21)
        vec = torch.randn(n, 768, generator=g) + 0.3 * torch.linspace(-1, 2, 768)  # no symmetry in d
        vec[5:25, 3::131] *= 25.0  # outlier dimensions
        vec[30] = 0
        vec[31] = 1e-8
        assert int((ar.set_embeddings(K, vec.cuda()) != 0).sum()) == 0
        g2 = torch.Generator().manual_seed(77)
        q = torch.randn(nq, 768, generator=g2) * 2 - 0.2 * torch.linspace(0, 1, 768) ** 2
        q[3, ::53] *= 30.0
        q[4] = vec[100]
        vs = VectorSearch(ar)
        qf, qmeta = vs.qprep8(q)
        bmax = vs.bmax_pass8(qf, qmeta, nq, slots)
        torch.cuda.synchronize()
        # query operand: fragment order -> [query, dim], and its bound in float64
        cq = qf.permute(0, 3, 1, 2, 4).reshape(256, 768).cpu().numpy().astype(np.float64)
        qm = qmeta.double().cpu().numpy()
        assert (cq[nq:] == 0).all() and (qm[nq:] == [0.0, -1.0]).all()
        qh = q.double().numpy()
        qh /= np.linalg.norm(qh, axis=1, keepdims=True)
        assert np.abs(cq).max() <= 127
        assert (np.abs(cq[:nq] * qm[:nq, :1] - qh) <= 0.5 * qm[:nq, :1] * (1 + 1e-3) + 1e-7).all()
        tq = np.linalg.norm(qh - cq[:nq] * qm[:nq, :1], axis=1)
        assert (qm[:nq, 1] >= tq).all() and (qm[:nq, 1] <= 1.01 * tq + 2e-6).all()
        # expected maxima from the stored codes and meta
        meta, v8 = ar.vec8_view()
        m = meta.double().cpu().numpy()
        c = v8.cpu().numpy().astype(np.float64)
        h = ar.slot_view()[:, :8].contiguous().cpu().numpy().view(np.uint64).ravel()
        ok = (h != 0) & (m[:, 1] >= 0) & (m[:, 0] > 0)
        assert ok.sum() == n - 2
        dots = c @ cq[:nq].T  # exact integers
        approx = dots * m[:, :1] * qm[None, :nq, 0]
        B = m[:, 1:2] + qm[None, :nq, 1] * (1 + m[:, 1:2]) + SLACK
        val = np.where(ok[:, None], approx - B, -np.inf)
        tiles = (slots + 255) // 256
        assert bmax.shape == (tiles, nq)
        got = bmax.double().cpu().numpy()
        for t in range(tiles):
            want = val[t * 256: min(slots, (t + 1) * 256)].max(axis=0)
            empty = ~np.isfinite(want)
            assert (got[t][empty] == -FLT_MAX).all(), t
            d = np.abs(got[t][~empty] - want[~empty])
            assert d.size == 0 or d.max() <= 1e-6, (t, float(d.max()))
        # the bound holds against the real cosine for every pair (what makes the search exact)
        vh = vec.double().numpy()
        live_rows = np.nonzero(ok)[0]
        st, idx = ar.meta("find", K)
        torch.cuda.synchronize()
        sl = idx.long().cpu().numpy()
        cos = np.zeros((slots, nq))
        nv = np.linalg.norm(vh, axis=1)
        keep = nv > 1e-5
        cos[sl[keep]] = (vh[keep] / nv[keep, None]) @ qh.T
        assert (np.abs(cos[live_rows] - approx[live_rows]) <= B[live_rows] - SLACK + 1e-9).all()
    finally:
        ar.close()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("nq", [40, 300])
def test_int8_search_batch_matches_exact(uniq, monkeypatch, nq, scaled):
    """Batched search on the int8 copy == the exact fp32 kernel (shapes of
    test_search_batch_matches_exact; `scaled`: every 97th dimension x40 in rows and queries, a coarse
    quantisation step and large error bounds), without leaning on the overflow fallback."""
    import torch
    from libsplinter_amd.ops.arena import HbmArena, pack_keys, pack_values
    from libsplinter_amd.ops.search import VectorSearch
    monkeypatch.setenv("SPLINTER_HBM_VEC8", "1")
    a = HbmArena.create(uniq, slots=20011, max_val=32, embeddings=True)
    try:
        assert a.has_vec8
        n = 15000
        K = pack_keys([f"e{i}" for i in range(n)], 16)
        V, L = pack_values([b"x"] * n, 16)
        assert (a.set(K, V, L) == 0).all()
        g = torch.Generator().manual_seed(1)
        vecs = _clustered(n, g)
        if scaled:
            vecs[:, ::97] *= 40.0
        vecs[11] = 0
        vecs[12] = 1e-8  # below the exact kernel's norm floor
        assert (a.set_embeddings(K, vecs.cuda()) == 0).all()
        a.meta("set_label", K[::3], torch.full((len(range(0, n, 3)),), 1 << 5, dtype=torch.int64, device="cuda"))
        q = _clustered(nq, g) * 3.0
        if scaled:
            q[:, ::97] *= 40.0
        q[0] = vecs[100]
        vs = VectorSearch(a, grid=128)
        st, st16 = {}, {}
        for kw in ({}, {"label_mask": 1 << 5}, {"min_sim": 0.6}, {"max_dist": 30.0}):
            i1, s1, d1 = vs.search_batch(q, k=10, stats=st, **kw)
            i0, s0, d0 = vs.search(q, k=10, **kw)
            print(dict(nq=nq, scaled=scaled, kw=kw, stats=st))
            assert st["copy"] == "int8", st
            assert torch.equal(i1, i0), kw
            assert torch.equal(s1, s0) and torch.equal(d1, d0), kw
            if "max_dist" not in kw:  # bounded distance: no sample threshold, every slot is a candidate
                assert st["overflow"] == 0 and st["candidates"] < nq * 2000, (kw, st)
            i3, s3, d3 = vs.search_batch(q, k=10, stats=st16, copy="bf16", **kw)
            assert st16["copy"] == "bf16", st16
            assert torch.equal(i3, i0) and torch.equal(s3, s0) and torch.equal(d3, d0), kw
        # tiny candidate cap: every query overflows and falls back to the exact kernel
        i2, _, _ = vs.search_batch(q, k=10, capb=1, stats=st)
        assert torch.equal(i2, vs.search(q, k=10)[0]) and st["overflow"] > 0 and st["copy"] == "int8"
        # SPLINTER_SEARCH_VEC8=0 is read per call: the same arena answers from the bf16 copy
        monkeypatch.setenv("SPLINTER_SEARCH_VEC8", "0")
        i4, s4, _ = vs.search_batch(q, k=10, stats=st)
        assert st["copy"] == "bf16" and torch.equal(i4, vs.search(q, k=10)[0])
    finally:
        a.close()


def _copy_kind(store):
    import ctypes
    from libsplinter_amd import _native as N
    from libsplinter_amd.ops.arena import HbmArena
    from libsplinter_amd.ops.search import _lib
    del ctypes, N
    return _lib().spl_search_copy_kind(HbmArena(store).desc)


def test_int8_c_abi_and_mixed_node(uniq, monkeypatch):
    """spl_search_batch on an hbm: store with the int8 copy returns the exact kernel's hits; a node:
    store of two HBM shards of which only one carries the copy (the call then runs every shard on
    the bf16 path) returns the same hits."""
    import torch
    from libsplinter_amd import Store
    from libsplinter_amd.store import NODE_HBM, node_join, node_leave, node_shard_name
    from libsplinter_amd.ops.arena import HbmArena
    from libsplinter_amd.ops.search import VectorSearch
    g = torch.Generator().manual_seed(9)
    n, nq, k = 5000, 64, 10
    vecs = _clustered(n, g).numpy()
    names = [f"e{i}" for i in range(n)]
    q = _clustered(nq, g).numpy() * 2.0
    q[0] = vecs[77]
    stores, top, joined = [], None, []
    try:
        monkeypatch.setenv("SPLINTER_HBM_VEC8", "1")
        single = Store.create(f"hbm:{uniq}", slots=8209, max_val=32, embeddings=True)
        stores.append(single)
        assert int((single.set_batch(names, [b"x"] * n) != 0).sum()) == 0
        assert int((single.set_embedding_batch(names, vecs) != 0).sum()) == 0
        ar = HbmArena(single)
        assert ar.has_vec8 and _copy_kind(single) == 2
        hits = single.search_batch(q, k)
        vs = VectorSearch(ar)
        i0, s0, d0 = vs.search(torch.from_numpy(q), k=k)
        keys0 = vs.keys_of(i0)
        assert [[h.decode() for h in row] for row in hits["key"].tolist()] == keys0
        assert np.array_equal(hits["sim"], s0.cpu().numpy()) and np.array_equal(hits["dist"], d0.cpu().numpy())
        assert hits["key"][0, 0].decode() == "e77"
        # two shards, the copy on the first only
        for r in range(2):
            if r == 1:
                monkeypatch.delenv("SPLINTER_HBM_VEC8")
            st = Store.create(node_shard_name(uniq, r, NODE_HBM), slots=4099, max_val=32, embeddings=True)
            stores.append(st)
            node_join(uniq, r, 2, NODE_HBM, st.slots, 32, True)
            joined.append(r)
        assert HbmArena(stores[1]).has_vec8 and not HbmArena(stores[2]).has_vec8
        top = Store.open(f"node:{uniq}")
        assert int((top.set_batch(names, [b"x"] * n) != 0).sum()) == 0
        assert int((top.set_embedding_batch(names, vecs) != 0).sum()) == 0
        h2 = top.search_batch(q, k)
        assert (h2["key"] == hits["key"]).all()
        assert np.array_equal(h2["sim"], hits["sim"]) and np.array_equal(h2["dist"], hits["dist"])
    finally:
        if top is not None:
            top.close()
        for st in stores:
            st.close()
        for r in joined:
            node_leave(uniq, r)


def test_int8_only_arena(uniq, monkeypatch):
    """SPLINTER_HBM_VEC16=0 with SPLINTER_HBM_VEC8=1: the arena carries the int8 copy alone (its meta
    entries start right after the side header), the search streams it, and `copy="bf16"` falls back
    to the bf16 pass over the fp32 rows -- all equal to the exact kernel."""
    import torch
    from libsplinter_amd.ops.arena import HbmArena, format_values
    from libsplinter_amd.ops.search import VectorSearch
    monkeypatch.setenv("SPLINTER_HBM_VEC8", "1")
    monkeypatch.setenv("SPLINTER_HBM_VEC16", "0")
    a = HbmArena.create(uniq, slots=3001, max_val=32, embeddings=True)
    try:
        assert a.has_vec8 and not a.has_vec16
        n, nq = 2000, 40
        K = _keys(np.arange(n))
        V, Lv = format_values(n, 1, 16, 32, ids=torch.arange(n, device="cuda"))
        assert int((a.set(K, V, Lv) != 0).sum()) == 0
        g = torch.Generator().manual_seed(4)
        vecs = _clustered(n, g)
        assert int((a.set_embeddings(K, vecs.cuda()) != 0).sum()) == 0
        st, idx = a.meta("find", K)
        _check_copy(a, idx.long().cpu().numpy(), "int8-only arena")
        q = _clustered(nq, g) * 2.0
        vs = VectorSearch(a, grid=128)
        i0, s0, d0 = vs.search(q, k=10)
        stats = {}
        i1, s1, d1 = vs.search_batch(q, k=10, stats=stats)
        assert stats["copy"] == "int8" and stats["overflow"] == 0
        assert torch.equal(i1, i0) and torch.equal(s1, s0) and torch.equal(d1, d0)
        i2, s2, _ = vs.search_batch(q, k=10, stats=stats, copy="bf16")
        assert stats["copy"] == "fp32" and torch.equal(i2, i0) and torch.equal(s2, s0)
    finally:
        a.close()
