"""splainference --prefix-cache: the prompt head that the system prompt gives every request is handed to
BatchDecodeEngine.set_prefix, whose cache rows are then computed once and copied into later requests.  The
flag changes no byte of any completion; it is checked at startup and ignored where --batch falls back to
sequential serving."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAITING, SERVICING, READY = 0x1000000000000000, 0x2000000000000000, 0x4000000000000000
SYS = ("You are a terse assistant. Answer in one short sentence and never repeat the question. " + "x" * 100)[:100]


def _daemon(name, *flags):
    return subprocess.run([sys.executable, "-m", "libsplinter_amd.daemons.splainference", "--oneshot",
                           "--random-init", *flags, name, "none.gguf", "7"], cwd=ROOT, capture_output=True,
                          text=True, timeout=300)


def _head(msg, system=SYS):
    return f"<system>\n{system}\n<user>\n{msg}\n<assistant>\n".encode()


def _post(s, reqs):
    for k, msg in reqs.items():
        s.set(k, msg)
        s.unset_label(k, READY)
        s.set_label(k, WAITING)


@pytest.mark.gpu
def test_prefix_cache_daemon_reuses_the_system_prompt_rows(uniq):
    """A 100-byte system prompt: the byte tokenizer's shared head is 118 tokens, 112 of them reused with chunk
    16.  Three WAITING keys under --batch 4: the first computes the rows, the other two start from copies (2
    hits, 224 rows); every key ends READY with a printable completion, and a run without --prefix-cache writes
    the same bytes to all three."""
    from libsplinter_amd import Store, unlink
    assert len(SYS.encode()) == 100
    reqs = {"req_a": "hello there", "req_b": "a longer question that needs a few more passes than the others",
            "req_c": "t"}
    flags = ("--device", "cuda", "--batch", "4", "--prefill-chunk", "16", "--system-prompt-key", "sys",
             "--max-tokens", "48")
    s = Store.create(uniq, slots=128, max_val=1024, embeddings=False)
    try:
        s.set("sys", SYS)
        _post(s, reqs)
        r = _daemon(uniq, *flags, "--prefix-cache")
        assert r.returncode == 0, r.stderr[-2000:]
        assert "[splainference] prefix cache: 2 hits, 224 rows reused" in r.stdout, r.stdout
        got = {}
        for k, msg in reqs.items():
            v = s.get(k)
            assert v.startswith(_head(msg)) and len(v) > len(_head(msg)), (k, v)
            assert all(32 <= c < 127 or c == 10 for c in v[len(_head(msg)):]), (k, v)
            b = s.snapshot(k)["bloom"]
            assert b & READY and not b & (WAITING | SERVICING), k
            got[k] = v
        _post(s, reqs)
        r = _daemon(uniq, *flags)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "prefix cache:" not in r.stdout
        assert {k: s.get(k) for k in reqs} == got
    finally:
        s.close()
        unlink(uniq)


def test_shared_prompt_prefix_is_the_common_head():
    from libsplinter_amd.daemons.splainference import build_prompt, shared_prompt_prefix
    from libsplinter_amd.models.decoder import ByteTokenizer
    tok = ByteTokenizer()
    assert shared_prompt_prefix(tok, SYS, None) == tok.encode("<system>\n" + SYS + "\n<user>\n")
    assert len(shared_prompt_prefix(tok, SYS, None)) == 118
    assert shared_prompt_prefix(tok, "", None) == tok.encode("<user>\n")
    before_user = {"{% chatml %}<|im_start|>": f"<|im_start|>system\n{SYS}<|im_end|>\n<|im_start|>user\n",
                   "{% gemma %}<start_of_turn>": f"<start_of_turn>user\n{SYS}\n\n"}
    for template, lead in before_user.items():
        head = shared_prompt_prefix(tok, SYS, template)
        assert len(head) > len(SYS)
        assert len(head) <= len(tok.encode(lead))  # ends at or before the user text
        for msg in ("How far is the moon?", "summarise this for me, please"):
            ids = tok.encode(build_prompt(SYS, msg, template))
            assert ids[: len(head)] == head and len(ids) > len(head), (template, msg)


class _StubEngine:
    """BatchDecodeEngine's submit / prefill / release / set_prefix bookkeeping with no model behind it: a prompt
    needs two passes, the second yields EOS, and the first pass of a serve rewrites the system prompt while its
    requests are still pending."""

    def __init__(self, store, S, rewrite=None):
        self.store, self.S, self.slots, self.rewrite = store, S, {}, rewrite
        self.prefixes, self.prefix_hits, self.prefix_rows_reused = [], 0, 0

    def pending(self):
        return sorted(self.slots)

    def set_prefix(self, ids, chunk):
        assert not self.pending(), "set_prefix while requests are pending"
        self.prefixes.append((bytes(t for t in ids if t < 256).decode(), chunk))
        return len(ids) // chunk * chunk

    def submit(self, ids, seed=None):
        slot = min(b for b in range(self.S) if b not in self.slots)
        self.slots[slot] = 0
        return slot

    def prefill(self, chunk):
        if self.rewrite is not None:
            self.store.set("sys", self.rewrite)
            self.rewrite = None
        out = {}
        for slot in list(self.slots):
            self.slots[slot] += 1
            if self.slots[slot] == 2:
                del self.slots[slot]
                out[slot] = 257  # EOS: the stream ends with an empty completion
        return out

    def release(self, slot):
        self.slots.pop(slot, None)


def test_daemon_sets_the_prefix_once_per_system_prompt_value(uniq):
    """set_prefix follows the system prompt key: once for a value however many serves and requests see it, again
    after the value changes, and only while nothing is pending -- a value that changes under pending requests
    is picked up when they are through."""
    from libsplinter_amd import Store, unlink
    from libsplinter_amd.daemons import splainference as mod
    from libsplinter_amd.models.decoder import ByteTokenizer, CausalLM, DecoderConfig, Sampler
    s = Store.create(uniq, slots=128, max_val=512, embeddings=False)
    try:
        model = CausalLM.random(DecoderConfig(layers=1), device="cpu")
        d = mod.Splainference(s, model, ByteTokenizer(), Sampler(seed=1), system_prompt_key="sys", max_tokens=8)
        eng = _StubEngine(s, 2)
        d.batch_engine, d.prefill_chunk, d.prefix_cache = eng, 16, True
        head = lambda v: f"<system>\n{v}\n<user>\n"  # noqa: E731
        s.set("sys", "first")
        _post(s, {"one": "hello one", "two": "hello two", "three": "hello three"})
        assert d.serve_batch() == 3  # two admission waves under one value
        assert eng.prefixes == [(head("first"), 16)]
        _post(s, {"one": "again"})
        assert d.serve_batch() == 1
        assert eng.prefixes == [(head("first"), 16)]
        s.set("sys", "second")
        _post(s, {"one": "again"})
        assert d.serve_batch() == 1
        assert eng.prefixes == [(head("first"), 16), (head("second"), 16)]
        eng.rewrite = "third"  # changes while "one" and "two" are pending
        _post(s, {"one": "x", "two": "y"})
        assert d.serve_batch() == 2
        assert eng.prefixes == [(head("first"), 16), (head("second"), 16), (head("third"), 16)]
        for k in ("one", "two", "three"):
            b = s.snapshot(k)["bloom"]
            assert b & READY and not b & (WAITING | SERVICING), k
        assert s.get("one") == _head("x", "second")  # built before the rewrite: the engine compares ids itself
        # without the flag the engine never hears of a prefix
        d.prefix_cache = False
        s.set("sys", "fourth")
        _post(s, {"one": "x"})
        assert d.serve_batch() == 1 and len(eng.prefixes) == 3
    finally:
        s.close()
        unlink(uniq)


def test_prefix_cache_flag_checked_and_ignored_on_cpu(uniq):
    """--prefix-cache without --prefill-chunk or with --batch 1 exits 1 with an Error line; with both on the CPU
    it serves exactly as without the flag: one fallback warning, the same bytes, the same labels."""
    from libsplinter_amd import Store, unlink
    reqs = {"one": "hello there", "two": "and another"}
    s = Store.create(uniq, slots=128, max_val=512, embeddings=False)
    try:
        for flags in (("--batch", "3", "--prefix-cache"), ("--batch", "1", "--prefill-chunk", "16", "--prefix-cache"),
                      ("--prefill-chunk", "16", "--prefix-cache")):
            r = _daemon(uniq, *flags, "--device", "cpu")
            assert r.returncode == 1 and "Error: --prefix-cache" in r.stderr, (flags, r.stderr)
        s.set("sys", "be brief")
        runs = []
        for extra in (("--prefix-cache",), ()):
            _post(s, reqs)
            r = _daemon(uniq, "--batch", "3", "--prefill-chunk", "16", *extra, "--system-prompt-key", "sys",
                        "--device", "cpu", "--max-tokens", "8")
            assert r.returncode == 0, r.stderr[-2000:]
            assert r.stdout.count("needs the GPU decode kernels") == 1, r.stdout
            vals = []
            for k, msg in reqs.items():
                v = s.get(k)
                assert v.startswith(_head(msg, "be brief"))
                b = s.snapshot(k)["bloom"]
                assert b & READY and not b & (WAITING | SERVICING)
                vals.append(v)
            runs.append(vals)
        assert runs[0] == runs[1]
        assert any(len(v) > len(_head(msg, "be brief")) for v, msg in zip(runs[0], reqs.values()))
    finally:
        s.close()
        unlink(uniq)
