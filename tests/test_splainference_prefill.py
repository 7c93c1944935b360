"""splainference --batch N --prefill-chunk C: WAITING requests are admitted together, C prompt tokens of each
per pass between two decode steps (BatchDecodeEngine.submit / prefill); the flag is checked at startup and
ignored where --batch falls back to sequential serving."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAITING, SERVICING, READY = 0x1000000000000000, 0x2000000000000000, 0x4000000000000000


def _daemon(name, *flags):
    return subprocess.run([sys.executable, "-m", "libsplinter_amd.daemons.splainference", "--oneshot",
                           "--random-init", *flags, name, "none.gguf", "7"], cwd=ROOT, capture_output=True,
                          text=True, timeout=300)


def _head(msg):
    return f"<user>\n{msg}\n<assistant>\n".encode()


@pytest.mark.gpu
def test_prefill_chunk_daemon_serves_waiting_keys_together(uniq):
    """Three WAITING keys under --batch 4 --prefill-chunk 16, one with a prompt of 105 tokens (7 passes, the
    others end in passes 2 and 1): each ends READY with its own prompt head and a printable completion; the
    long key served alone by a second run gets the same bytes (its chunk boundaries, seed and kernels do not
    depend on what shares its passes)."""
    from libsplinter_amd import Store, unlink
    long_msg = "a much longer question, long enough to need several prefill passes of sixteen tokens"
    reqs = {"req_a": "hello there", "req_b": long_msg, "req_c": "t"}
    assert len(_head(long_msg)) + 1 > 3 * 16  # BOS + bytes: at least 3 passes (it has 7)
    flags = ("--device", "cuda", "--batch", "4", "--prefill-chunk", "16", "--max-tokens", "48")
    s = Store.create(uniq, slots=128, max_val=512, embeddings=False)
    try:
        for k, msg in reqs.items():
            s.set(k, msg)
            s.set_label(k, WAITING)
        s.set("other", "not a request")
        r = _daemon(uniq, *flags)
        assert r.returncode == 0, r.stderr[-2000:]
        got = {}
        for k, msg in reqs.items():
            v = s.get(k)
            assert v.startswith(_head(msg)) and len(v) > len(_head(msg)), (k, v)
            assert all(32 <= c < 127 or c == 10 for c in v[len(_head(msg)):]), (k, v)
            b = s.snapshot(k)["bloom"]
            assert b & READY and not b & (WAITING | SERVICING), k
            got[k] = v
        assert not s.snapshot("other")["bloom"] & READY
        dbg = s.get("__debug").decode()
        assert all(f"[DONE]: Completion written to key: {k}" in dbg for k in reqs)
        # the long key alone
        s.set("req_b", reqs["req_b"])
        s.unset_label("req_b", READY)
        s.set_label("req_b", WAITING)
        r = _daemon(uniq, *flags)
        assert r.returncode == 0, r.stderr[-2000:]
        assert s.get("req_b") == got["req_b"]
    finally:
        s.close()
        unlink(uniq)


class _StubEngine:
    """The slot bookkeeping of BatchDecodeEngine.submit / prefill / release with no model behind it: the first
    prefill pass asks the daemon to shut down and yields no token."""

    def __init__(self, mod, S):
        self.mod, self.S, self.slots, self.released = mod, S, {}, []

    def submit(self, ids, seed=None):
        slot = min(b for b in range(self.S) if b not in self.slots)
        self.slots[slot] = list(ids)
        return slot

    def prefill(self, chunk):
        self.mod._running = False
        return {}

    def release(self, slot):
        self.released.append(slot)
        del self.slots[slot]


def test_shutdown_cancels_pending_requests_to_ready(uniq):
    """A shutdown request while two submitted prompts have no token yet: both slots are released and both keys
    go SERVICING -> READY with the formatted prompt and an empty completion; a key that was never begun stays
    WAITING."""
    from libsplinter_amd import Store, unlink
    from libsplinter_amd.daemons import splainference as mod
    from libsplinter_amd.models.decoder import ByteTokenizer, CausalLM, DecoderConfig, Sampler
    s = Store.create(uniq, slots=128, max_val=512, embeddings=False)
    try:
        for k in ("one", "two", "three"):
            s.set(k, "hello " + k)
            s.set_label(k, WAITING)
        model = CausalLM.random(DecoderConfig(layers=1), device="cpu")
        d = mod.Splainference(s, model, ByteTokenizer(), Sampler(seed=1), max_tokens=8)
        d.batch_engine, d.prefill_chunk = _StubEngine(mod, 2), 16
        try:
            assert d.serve_batch() == 2
        finally:
            mod._running = True
        assert sorted(d.batch_engine.released) == [0, 1] and not d.batch_engine.slots
        blooms = {k: s.snapshot(k)["bloom"] for k in ("one", "two", "three")}
        done = [k for k, b in blooms.items() if b & READY]
        assert len(done) == 2 and not any(b & SERVICING for b in blooms.values())
        for k, b in blooms.items():
            if k in done:
                assert not b & WAITING and s.get(k) == _head("hello " + k)
            else:
                assert b & WAITING and s.get(k) == ("hello " + k).encode()
    finally:
        s.close()
        unlink(uniq)


def test_prefill_chunk_flag_checked_and_ignored_on_cpu(uniq):
    """--prefill-chunk -1 exits 1; --batch 3 --prefill-chunk 16 on the CPU serves exactly as --batch 3 does:
    one fallback warning, the same bytes and the same labels."""
    from libsplinter_amd import Store, unlink
    reqs = (("one", "hello there"), ("two", "and another"))
    s = Store.create(uniq, slots=128, max_val=512, embeddings=False)
    try:
        assert _daemon(uniq, "--prefill-chunk", "-1", "--device", "cpu").returncode == 1
        runs = []
        for flags in (("--batch", "3", "--prefill-chunk", "16"), ("--batch", "3")):
            for k, msg in reqs:
                s.set(k, msg)
                s.unset_label(k, READY)
                s.set_label(k, WAITING)
            r = _daemon(uniq, *flags, "--device", "cpu", "--max-tokens", "8")
            assert r.returncode == 0, r.stderr[-2000:]
            assert r.stdout.count("needs the GPU decode kernels") == 1, r.stdout
            vals = []
            for k, msg in reqs:
                v = s.get(k)
                assert v.startswith(_head(msg))
                b = s.snapshot(k)["bloom"]
                assert b & READY and not b & (WAITING | SERVICING)
                vals.append(v)
            runs.append(vals)
        assert runs[0] == runs[1]
        assert any(len(v) > len(_head(msg)) for v, (_, msg) in zip(runs[0], reqs))
    finally:
        s.close()
        unlink(uniq)
