"""splainference --batch N: several requests decoded together on the GPU (BatchDecodeEngine), and the
sequential fallback with one warning where the batched step cannot run."""
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
def test_batch_daemon_serves_waiting_keys_together(uniq):
    """Three WAITING keys under --batch 4: each ends READY with its own prompt head and a printable
    completion; a key served alone by a second --batch 4 run gets the same bytes (its seed is the daemon
    seed XOR the key hash, so its tokens do not depend on what shares its steps)."""
    from libsplinter_amd import Store, unlink
    reqs = {"req_a": "hello there", "req_b": "a second, rather longer question about nothing", "req_c": "third"}
    flags = ("--device", "cuda", "--batch", "4", "--max-tokens", "48")
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
        # the same key alone
        s.set("req_b", reqs["req_b"])
        s.unset_label("req_b", READY)
        s.set_label("req_b", WAITING)
        r = _daemon(uniq, *flags)
        assert r.returncode == 0, r.stderr[-2000:]
        assert s.get("req_b") == got["req_b"]
    finally:
        s.close()
        unlink(uniq)


def test_batch_flag_on_cpu_warns_once_and_serves_sequentially(uniq):
    """--batch 3 on the CPU: one startup warning, then both keys are served as without the flag: the same
    bytes and the same labels."""
    from libsplinter_amd import Store, unlink
    reqs = (("one", "hello there"), ("two", "and another"))
    s = Store.create(uniq, slots=128, max_val=512, embeddings=False)
    try:
        runs = []
        for flags in (("--batch", "3"), ()):
            for k, msg in reqs:
                s.set(k, msg)
                s.unset_label(k, READY)
                s.set_label(k, WAITING)
            r = _daemon(uniq, *flags, "--device", "cpu", "--max-tokens", "8")
            assert r.returncode == 0, r.stderr[-2000:]
            assert r.stdout.count("needs the GPU decode kernels") == (1 if flags else 0), r.stdout
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
        assert _daemon(uniq, "--batch", "17", "--device", "cpu").returncode == 1
    finally:
        s.close()
        unlink(uniq)
