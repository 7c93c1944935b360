"""The batched set / get kernels (arena_kernels.hip k_kv_batch) on their own: both coherence forms
against one oracle, the edges of the lane sequence, and the get that writes nothing past its value."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5

# Runs in a fresh process: SPLINTER_ARENA_COOP / SPLINTER_ARENA_COOP_GET are read once per process.
_FORMS_CHILD = r"""
import json, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from libsplinter_amd.ops.arena import HbmArena, format_keys, format_values, pack_keys, pack_values
name, SENT = sys.argv[2], 0xA5
res = {}
rng = np.random.default_rng(11)
edge = [1, 15, 16, 17, 255, 256]


def lengths(n, shift):
    L = rng.integers(1, 257, size=n)
    for i in range(n // 7):
        L[(7 * i + shift) % n] = edge[(i + shift) % len(edge)]
    return L


for ks in (16, 32):
    a = HbmArena.create(f"{name}k{ks}", slots=4096, max_val=256, embeddings=False)
    try:
        n, nmiss = 3000, 200
        keys = [f"key-{i}-{rng.integers(1 << 20)}" for i in range(n)]
        ref = {}
        K = pack_keys(keys, ks)
        for rnd in range(2):  # insert, then update in place with other lengths
            L = lengths(n, 3 * rnd)
            vals = [bytes(rng.integers(0, 256, size=int(l), dtype=np.uint8)) for l in L]
            V, Ln = pack_values(vals, 256)
            st = a.set(K, V, Ln)
            torch.cuda.synchronize()
            assert (st == 0).all(), st[st != 0][:10]
            ref.update(zip(keys, vals))
        assert {len(v) for v in ref.values()} >= set(edge)
        allk = keys + [f"nope-{i}" for i in range(nmiss)]
        out = torch.full((n + nmiss, 256), SENT, dtype=torch.uint8, device="cuda")
        st, out, ol = a.get(pack_keys(allk, ks), out=out)
        torch.cuda.synchronize()
        st, out, ol = st.cpu().numpy(), out.cpu().numpy(), ol.cpu().numpy()
        for i, k in enumerate(allk):
            want = ref.get(k)
            if want is None:
                assert st[i] == -2 and ol[i] == 0 and (out[i] == SENT).all(), (k, st[i], ol[i])
            else:
                assert st[i] == 0 and ol[i] == len(want) and bytes(out[i, : ol[i]]) == want, (k, st[i], ol[i])
                assert (out[i, (len(want) + 15) // 16 * 16:] == SENT).all(), ("wrote past its chunks", k, len(want))
        res[f"dict_ks{ks}"] = "ok"
    finally:
        a.close()

# the hot-key race of test_arena_gpu.test_hot_keys_carried_retries, 64 keys x 8000 sets + 8000 gets
a = HbmArena.create(name + "h", slots=4096, max_val=256, embeddings=False)
try:
    n, hot = 8000, 64
    ids = torch.arange(n, device="cuda") % hot
    K = format_keys(n, "hot", 4, 16, ids=ids)
    V0, L0 = format_values(hot, 1, 150, 256, ids=torch.arange(hot, device="cuda"))
    assert (a.set(K[:hot], V0, L0) == 0).all()
    torch.cuda.synchronize()
    a.reset_stats()
    V, L = format_values(n, 5, 150, 256, ids=ids)
    sw, sr = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sw):
        sst = a.set(K, V, L, retries=64)
    with torch.cuda.stream(sr):
        gst, out, ol = a.get(K, retries=64)
    torch.cuda.synchronize()
    sst, gst = sst.cpu(), gst.cpu()
    assert bool(((sst == 0) | (sst == -11)).all()) and bool(((gst == 0) | (gst == -11)).all())
    assert int((sst == 0).sum()) >= hot
    attempts, ok, again, miss = [int(x) for x in a.stats.tolist()]
    assert ok == int((sst == 0).sum()) + int((gst == 0).sum()) and miss == 0
    assert attempts == ok + again
    o, ln, idh = out.cpu().numpy(), ol.cpu().numpy(), ids.cpu().numpy()
    checked = 0
    for i in np.nonzero(gst.numpy() == 0)[0][::7]:
        s = bytes(o[i, : ln[i]])
        head, _, rest = s.partition(b"|id:")
        ver = int(head[4:])
        assert int(rest.split(b"|")[0]) == idh[i] and ver in (1, 5)
        fill = s[s.index(b"data:") + 5:]
        assert fill == bytes([65 + ver % 26]) * len(fill), "torn value"
        checked += 1
    pend = torch.nonzero(sst.cuda() != 0).squeeze(1)
    for _ in range(200):
        if pend.numel() == 0:
            break
        r = a.set(K[pend].contiguous(), V[pend].contiguous(), L[pend].contiguous(), retries=64)
        pend = pend[r != 0]
    assert pend.numel() == 0
    st, out2, ol2 = a.get(K[:hot])
    assert (st == 0).all()
    for i in range(hot):
        assert bytes(out2[i, : ol2[i]].cpu().numpy()).startswith(b"ver:5|")
    gpend = torch.nonzero(gst.cuda() != 0).squeeze(1)
    if gpend.numel():
        st3, _, _ = a.get(K[gpend].contiguous())
        assert (st3 == 0).all()
    res.update(attempts=attempts, ok=ok, again=again, set_ok=int((sst == 0).sum()), get_ok=int((gst == 0).sum()),
               values_checked=checked)
finally:
    a.close()
print(json.dumps(res), flush=True)
"""


@pytest.mark.parametrize("form", ["fence", "default"])
def test_batch_forms_match_dict_and_survive_hot_keys(uniq, form):
    """Both coherence forms of k_kv_batch against one oracle: "fence" (SPLINTER_ARENA_COOP=1
    SPLINTER_ARENA_COOP_GET=1: plain rows + one release per round, one agent acquire per round) and the
    default (write-through rows, acquire-free sc1 reads).  kstride 16 and 32, value lengths over the
    16-B chunk edges, insert / update / get with misses against a dict, a get's output untouched past
    its last chunk, then 64 hot keys with 8000 sets racing 8000 gets: every status 0 or EAGAIN, the
    stats add up, no torn value, resubmission drains."""
    env = {k: v for k, v in os.environ.items() if k not in ("SPLINTER_ARENA_COOP", "SPLINTER_ARENA_COOP_GET")}
    if form == "fence":
        env.update(SPLINTER_ARENA_COOP="1", SPLINTER_ARENA_COOP_GET="1")
    r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, ROOT, uniq], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(form, res)
    assert res["dict_ks16"] == "ok" and res["dict_ks32"] == "ok" and res["values_checked"] > 0


# one workgroup is 512 ops (256 lanes x 2); the capped grid is 2048 workgroups, so the last n is the
# first at which a lane takes a second lap
@pytest.mark.parametrize("n", [1, 2, 511, 512, 513, 2 * 256 * 2048 + 3])
def test_batch_lane_sequence_edges(uniq, n):
    """set, then get, of n formatted rows; then a get with 3 missing keys appended: every row is served
    exactly once (statuses, lengths, bytes, and attempts == ok + miss with ok == n, miss == 3)."""
    import torch
    from libsplinter_amd.ops.arena import HbmArena, format_keys, format_values
    slots = 4096
    while slots < 2 * n:
        slots *= 2
    a = HbmArena.create(uniq, slots=slots, max_val=32, embeddings=False)
    try:
        K = format_keys(n + 3, "e", 9, 16)
        V, L = format_values(n, 1, 24, 32)
        st = a.set(K[:n], V, L)
        assert bool((st == 0).all()), st[st != 0][:10]
        col = torch.arange(32, device="cuda")[None, :]

        def check(st, out, ol, m):
            assert bool((st[:n] == 0).all()) and bool((ol[:n] == L).all())
            live = col < L[:, None]
            assert bool(((out[:n] == V) | ~live).all())
            # whole chunks are copied; nothing past them
            past = col >= ((L[:, None] + 15) // 16 * 16)
            assert bool(((out[:n] == SENTINEL) | ~past).all())
            assert st[n:].tolist() == [-2] * m and ol[n:].tolist() == [0] * m
            assert bool((out[n:] == SENTINEL).all())

        out = torch.full((n, 32), SENTINEL, dtype=torch.uint8, device="cuda")
        check(*a.get(K[:n], out=out), 0)
        a.reset_stats()
        out = torch.full((n + 3, 32), SENTINEL, dtype=torch.uint8, device="cuda")
        check(*a.get(K, out=out), 3)
        attempts, ok, again, miss = [int(x) for x in a.stats.tolist()]
        print(n, dict(attempts=attempts, ok=ok, again=again, miss=miss))
        assert ok == n and miss == 3 and attempts == ok + again + miss
    finally:
        a.close()


def test_batch_get_writes_nothing_past_its_value(uniq):
    """ostride 256, value lengths 1..200: a.get leaves every output byte past ceil(len / 16) * 16
    alone (the fused grid pads its output rows to 64 B; the batch kernel must not)."""
    import torch
    from libsplinter_amd.ops.arena import HbmArena, pack_keys, pack_values
    a = HbmArena.create(uniq, slots=4096, max_val=256, embeddings=False)
    try:
        vals = [bytes([1 + (i * 7 + j) % 250 for j in range(1 + i % 200)]) for i in range(600)]
        K = pack_keys([f"p{i:05d}" for i in range(len(vals))], 16)
        V, L = pack_values(vals, 256)
        assert bool((a.set(K, V, L) == 0).all())
        out = torch.full((len(vals), 256), SENTINEL, dtype=torch.uint8, device="cuda")
        st, out, ol = a.get(K, out=out)
        torch.cuda.synchronize()
        assert bool((st == 0).all())
        o, ln = out.cpu().numpy(), ol.cpu().numpy()
        for i, v in enumerate(vals):
            assert ln[i] == len(v) and bytes(o[i, : ln[i]]) == v
            assert (o[i, (len(v) + 15) // 16 * 16:] == SENTINEL).all(), (i, len(v))
    finally:
        a.close()
