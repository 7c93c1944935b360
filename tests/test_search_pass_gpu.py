"""The raw MFMA candidate pass (csrc/hip/search_kernels.hip: k_search_side on the bf16 / int8 side
copies, mf::k_search_mma on the fp32 rows) against float64 numpy: the operand map of the bf16 pass
on both of its row sources, and blocks that walk several tiles (the ring carried from one tile into
the next), which the batched search's 256-block grid never does on a small arena."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
SLOTS, ROWS, NQ = 1024 + 37, 600, 48  # 5 tiles, the last one shifted back over 219 slots of tile 3
TILES = (SLOTS + 255) // 256
TOL16 = 4e-4          # fp32 accumulation and norm error: the last term of ops/search.py DELTA
TOL8 = 1e-6           # the fp32 roundings of the int8 epilogue (approx and B: under ten roundings of values <= 4)
CAPB = 64
ENV = {"bf16": {}, "fp32": {"SPLINTER_HBM_VEC16": "0"}, "int8": {"SPLINTER_HBM_VEC8": "1"}}


class World:
    """One arena per operand with the rows and queries of test_int8_pass_operand_map_and_epilogue_exact,
    and the float64 reference scores of every (slot, query) pair, computed once."""

    def __init__(self, operand):
        import torch
        from libsplinter_amd.ops.arena import HbmArena, format_keys, format_values
        from libsplinter_amd.ops.search import VectorSearch
        self.operand = operand
        self.kind = "int8" if operand == "int8" else "bf16"
        with pytest.MonkeyPatch.context() as mp:
            for k, v in ENV[operand].items():
                mp.setenv(k, v)
            self.ar = ar = HbmArena.create(f"t{os.getpid()}_pass_{operand}", slots=SLOTS, max_val=32, embeddings=True)
        assert ar.has_vec16 == (operand != "fp32") and ar.has_vec8 == (operand == "int8")
        ids = torch.arange(ROWS, device="cuda")
        K = format_keys(ROWS, "c", 9, 16, ids=ids)
        V, Lv = format_values(ROWS, 1, 16, 32, ids=ids)
        assert int((ar.set(K, V, Lv) != 0).sum()) == 0
        g = torch.Generator().manual_seed(21)
        vec = torch.randn(ROWS, 768, generator=g) + 0.3 * torch.linspace(-1, 2, 768)  # no symmetry in d
        vec[5:25, 3::131] *= 25.0
        vec[30] = 0
        vec[31] = 1e-8
        assert int((ar.set_embeddings(K, vec.cuda()) != 0).sum()) == 0
        g2 = torch.Generator().manual_seed(77)
        q = torch.randn(NQ, 768, generator=g2) * 2 - 0.2 * torch.linspace(0, 1, 768) ** 2
        q[3, ::53] *= 30.0
        q[4] = vec[100]
        self.vs = vs = VectorSearch(ar)
        self.qop = vs.qprep8(q) if self.kind == "int8" else (vs.qprep16(q),)
        torch.cuda.synchronize()
        self.h = ar.slot_view()[:, :8].contiguous().cpu().numpy().view(np.uint64).ravel() != 0
        assert self.h.sum() == ROWS
        if self.kind == "bf16":
            # bf16(v) . bf16(q / |q|) / sqrt(|v|^2), rounding to nearest even as torch's .to(bfloat16)
            em = ar.embedding_matrix().cpu()
            qb = (q / q.norm(dim=1, keepdim=True).clamp_min(1e-30)).to(torch.bfloat16).double().numpy()
            n2 = (em.double().numpy() ** 2).sum(axis=1).astype(np.float32).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                self.score = (em.to(torch.bfloat16).double().numpy() @ qb.T) / np.sqrt(n2)[:, None]
            self.live0 = self.h & (n2 > 2e-12)   # MODE 0 counts surely-live slots only
            self.live1 = self.h & (n2 > 0)
            self.always = np.zeros(SLOTS, bool)
            self.tol = TOL16
            assert self.live0.sum() == ROWS - 2 and self.live1.sum() == ROWS - 1
        else:
            # approx + B from the stored codes and bounds (the int8 test checks approx - B the same way)
            qf, qmeta = self.qop
            cq = qf.permute(0, 3, 1, 2, 4).reshape(256, 768).cpu().numpy().astype(np.float64)[:NQ]
            qm = qmeta.double().cpu().numpy()[:NQ]
            meta, v8 = ar.vec8_view()
            m = meta.double().cpu().numpy()
            approx = (v8.cpu().numpy().astype(np.float64) @ cq.T) * m[:, :1] * qm[None, :, 0]
            self.score = approx + m[:, 1:2] + qm[None, :, 1] * (1 + m[:, 1:2]) + (4e-4 + 2e-6)
            self.live0 = self.live1 = self.h & (m[:, 1] >= 0)
            self.always = self.live1 & (m[:, 1] >= 2)  # a vector that cannot be bounded: every query's candidate
            self.tol = TOL8
            assert self.live1.sum() == ROWS - 1 and self.always.sum() == 1
        self._thr = None

    def bmax(self, grid):
        import torch
        out = torch.full((TILES, NQ), float("nan"), dtype=torch.float32, device="cuda")
        self.vs.mma_pass(self.kind, self.qop, NQ, SLOTS, 0, bmax=out, grid=grid)
        torch.cuda.synchronize()
        return out

    def thresholds(self):
        """Per query the midpoint of two adjacent reference scores near rank 20 that lie more than
        twice the tolerance apart, as fp32: no (slot, query) pair is within tolerance of its threshold."""
        if self._thr is None:
            thr = np.empty(NQ, np.float32)
            rows = self.live1 & ~self.always
            for j in range(NQ):
                s = np.sort(self.score[rows, j])[::-1]
                gaps = s[:-1] - s[1:]
                near = [r for r in sorted(range(8, 40), key=lambda r: abs(r - 20)) if gaps[r] > 3 * self.tol]
                assert near, j
                thr[j] = 0.5 * (s[near[0]] + s[near[0] + 1])
            d = np.abs(self.score[rows] - thr.astype(np.float64)[None, :])
            assert d.min() > self.tol, float(d.min())
            self._thr = thr
        return self._thr

    def candidates(self, grid):
        """The MODE 1 pass -> per query the sorted emitted slots (cnt, cand and the rows q >= nq checked)."""
        import torch
        thr = torch.from_numpy(self.thresholds()).cuda()
        cnt = torch.zeros(256, grid, dtype=torch.int32, device="cuda")
        cand = torch.full((256, grid, CAPB), -1, dtype=torch.int32, device="cuda")
        self.vs.mma_pass(self.kind, self.qop, NQ, SLOTS, 1, thr=thr, cnt=cnt, cand=cand, capb=CAPB, grid=grid)
        torch.cuda.synchronize()
        cnt, cand = cnt.cpu().numpy(), cand.cpu().numpy()
        assert (cnt[NQ:] == 0).all() and (cand[NQ:] == -1).all()
        assert (cnt >= 0).all() and (cnt <= CAPB).all()
        assert (cnt[:, min(grid, TILES):] == 0).all()  # blocks without a tile
        got = []
        for j in range(NQ):
            seg = np.concatenate([cand[j, b, :cnt[j, b]] for b in range(grid)])
            assert (cand[j][np.arange(CAPB)[None, :] >= cnt[j][:, None]] == -1).all(), j
            assert len(set(seg.tolist())) == seg.size, j  # the shifted last tile's overlap appears once
            got.append(np.sort(seg))
        return got


_worlds = {}


@pytest.fixture(scope="module")
def world(request):
    w = _worlds.get(request.param)
    if w is None:
        w = _worlds[request.param] = World(request.param)
    return w


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _worlds.values():
        w.ar.close()
    _worlds.clear()


@pytest.mark.parametrize("world", ["bf16", "fp32"], indirect=True)
def test_bf16_pass_operand_map(world):
    """MODE 0 of the bf16 pass on the bf16 copy and on the fp32 rows: every per-tile maximum against
    float64 numpy, over a partial last tile, a zero row and a row below the norm floor.  Rows and
    queries come from different seeds without symmetry over the dimensions, so a wrong lane map,
    or rows and queries swapped, cannot reproduce them."""
    from libsplinter_amd.ops.search import COPY_KINDS, MMA_GRID
    w = world
    assert COPY_KINDS[w.vs.L.spl_search_copy_kind(w.ar.desc)] == w.operand
    got = w.bmax(MMA_GRID).double().cpu().numpy()
    val = np.where(w.live0[:, None], w.score, -np.inf)
    worst = 0.0
    for t in range(TILES):
        want = val[t * 256: min(SLOTS, (t + 1) * 256)].max(axis=0)
        empty = ~np.isfinite(want)
        assert (got[t][empty] == -FLT_MAX).all(), t
        if (~empty).any():
            worst = max(worst, float(np.abs(got[t][~empty] - want[~empty]).max()))
    print(dict(operand=w.operand, max_abs_err=worst))
    assert worst <= TOL16, worst


@pytest.mark.parametrize("world", ["bf16", "fp32", "int8"], indirect=True)
def test_pass_blocks_walk_several_tiles(world):
    """grid = 2 over 5 tiles: block 0 walks tiles 0, 2, 4 and block 1 tiles 1, 3 (the ring carried
    across tiles, the next tile's prefetch, the waits of a non-first tile).  MODE 0 equals one tile
    per block bit for bit; MODE 1 emits exactly the reference set, for both grids."""
    import torch
    from libsplinter_amd.ops.search import MMA_GRID
    w = world
    b2, b256 = w.bmax(2), w.bmax(MMA_GRID)
    assert not bool(torch.isnan(b256).any())
    assert torch.equal(b2.view(torch.int32), b256.view(torch.int32))
    thr = w.thresholds().astype(np.float64)
    keep = w.live1[:, None] & ((w.score >= thr[None, :]) | w.always[:, None])
    want = [np.nonzero(keep[:, j])[0] for j in range(NQ)]
    assert all(8 <= len(x) <= 42 for x in want), [len(x) for x in want]
    for grid in (2, MMA_GRID):
        got = w.candidates(grid)
        for j in range(NQ):
            assert np.array_equal(got[j], want[j]), (grid, j, got[j].tolist(), want[j].tolist())
