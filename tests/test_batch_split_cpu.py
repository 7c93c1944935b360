"""Batch.split (the document groups of NOMIC_SPLIT) on the CPU: the cut arithmetic, and that every
group is the Batch its own documents would make."""
import numpy as np
import pytest

LENS = {
    "varied": [5, 40, 129, 300, 77, 64, 1, 250, 33],
    "one_long": [1000, 1, 1, 1],          # duplicate cuts: an empty group is skipped
    "equal": [10] * 8,
    "long_last": [1, 1, 1, 1000],
    "qblock_edges": [127, 128, 129, 256, 257, 1],
}


def _docs(lens):
    rng = np.random.default_rng(len(lens))
    return [rng.integers(1, 30000, size=n).tolist() for n in lens]


@pytest.mark.parametrize("parts", [2, 3, 4])
@pytest.mark.parametrize("name", list(LENS))
def test_split_groups(name, parts):
    import torch
    from libsplinter_amd.models.nomic import Batch
    lens = LENS[name]
    docs = _docs(lens)
    b = Batch(docs, device="cpu")
    groups = b.split(parts)
    assert 1 <= len(groups) <= parts
    if name == "one_long" and parts > 2:
        assert len(groups) == 2, "the duplicate cuts leave two groups"
    if name == "equal" or (name == "varied" and parts < 4):   # (varied, 4): the 300-token document holds two cuts
        assert len(groups) == parts
    d0 = 0
    ids, pos = [], []
    for sb, r0 in groups:
        assert sb.B > 0
        assert r0 == int(b.cu_host[d0]), (d0, r0)          # contiguous: starts where the last one ended
        fresh = Batch(docs[d0: d0 + sb.B], device="cpu")
        assert (sb.T, sb.T_pad, sb.nqb, sb.max_len) == (fresh.T, fresh.T_pad, fresh.nqb, fresh.max_len)
        assert np.array_equal(sb.cu_host, fresh.cu_host)
        assert np.array_equal(sb.cu_host, b.cu_host[d0: d0 + sb.B + 1] - r0)
        for f in ("cu", "qblocks", "ids", "pos"):
            assert torch.equal(getattr(sb, f), getattr(fresh, f)), f
        assert sb.cu.dtype == torch.int32 and sb.qblocks.dtype == torch.int32
        # positions restart at 0 in every document
        for d in range(sb.B):
            a, e = int(sb.cu_host[d]), int(sb.cu_host[d + 1])
            assert torch.equal(sb.pos[a:e], torch.arange(e - a, dtype=torch.int32))
        # q-blocks: (document, first row) pairs, 128 rows apart, every row of every document covered
        qb = sb.qblocks.reshape(-1, 2).tolist()
        assert qb == [[d, q0] for d in range(sb.B) for q0 in range(0, lens[d0 + d], 128)]
        ids.append(sb.ids[: sb.T])
        pos.append(sb.pos[: sb.T])
        d0 += sb.B
    assert d0 == b.B, "every document in exactly one group"
    assert torch.equal(torch.cat(ids), b.ids[: b.T])
    assert torch.equal(torch.cat(pos), b.pos[: b.T])
    # about equal token counts: no cut lies further from its target than the document it falls in
    ends = np.cumsum([sb.T for sb, _ in groups])[:-1]
    if len(groups) == parts:
        for j, e in enumerate(ends, 1):
            assert abs(e - b.T * j / parts) <= max(lens), (j, e)
    again = b.split(parts)
    assert again is groups, "the second call returns the cached list"


def test_split_parts_are_cached_per_count():
    from libsplinter_amd.models.nomic import Batch
    b = Batch(_docs(LENS["varied"]), device="cpu")
    g2, g3 = b.split(2), b.split(3)
    assert g2 is not g3 and len(g2) == 2 and len(g3) == 3
    assert b.split(2) is g2 and b.split(3) is g3
    assert len(b.split(1)) == 1 and b.split(1)[0][1] == 0 and b.split(1)[0][0].T == b.T
