"""Decoder architectures on the CPU path (models/decoder.py): qwen2 (q/k/v biases, NeoX rotation), qwen3
(per-head q/k RMSNorm, key_length), llama-3 RoPE scaling (rope_freqs.weight, linear) and the tied head, each
as a synthetic GGUF against the fp64 reference of tests/decoder_arch_ref.py (the file's own convention, so
independent of the loader's row permutation); the refusal of everything else; the unchanged logits of
the files and paths that already worked; and the daemon's state machine over a qwen2 file.

Tolerance of the logit tests: max |logit - fp64| <= 1e-4.  The llama CPU path measures about 1.4e-6 against
this kind of reference on these shapes (2 layers, d 128, 24 tokens, logits of magnitude 3); before these
architectures were computed the qwen2 case missed by more than 2."""
import os
import signal

import numpy as np
import pytest

import decoder_arch_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_arch")
WAITING, SERVICING, READY = 0x1000000000000000, 0x2000000000000000, 0x4000000000000000
TOL = 1e-4

CASES = {
    "qwen2": R.spec("qwen2", d=128, H=2, KVH=1, hd=64, bias=True, rope_base=1e6, seed=1),
    "qwen3": R.spec("qwen3", d=128, H=4, KVH=2, hd=64, norm=True, rope_base=1e6, seed=2),
    "llama_rope_freqs": R.spec("llama", d=128, H=2, KVH=1, rope_freqs=True, seed=3),
    "llama_linear": R.spec("llama", d=128, H=2, KVH=1, scaling=("linear", 4.0), seed=4),
    "qwen2_tied": R.spec("qwen2", d=128, H=2, KVH=1, hd=64, bias=True, rope_base=1e6, tied=True, seed=5),
}
CASES["qwen2"]["key_length"] = False  # hd 64 = d / H: the file carries no key_length
CASES["qwen2_tied"]["key_length"] = False


def _load(tmp_path, sp, **kw):
    from libsplinter_amd.models.decoder import CausalLM
    w = R.weights(sp)
    path = R.write_gguf(tmp_path / "m.gguf", sp, w, **kw)
    m, tok = CausalLM.from_gguf(path, device="cpu")
    return m, tok, w, path


@pytest.mark.parametrize("case", list(CASES))
def test_logits_match_fp64_reference(tmp_path, case):
    import torch
    sp = CASES[case]
    m, _, w, _ = _load(tmp_path, sp)
    ids = R.prompt(24)
    got = m.forward(ids).double()
    ref = R.ref_logits(sp, w, ids)[-1]
    err = (got - ref).abs().max().item()
    print(f"{case}: max |logit - fp64| = {err:.3e}, max |logit| = {ref.abs().max().item():.2f}")
    assert err <= TOL
    assert int(got.argmax()) == int(ref.argmax())
    assert torch.isfinite(got).all()
    cfg = m.cfg
    assert cfg.arch == sp["arch"] and cfg.qkv_bias == sp["bias"] and cfg.qk_norm == sp["norm"]
    assert cfg.head_dim == sp["hd"] and cfg.q_dim == sp["H"] * sp["hd"]
    if case == "qwen3":
        assert cfg.q_dim == 256 != cfg.d and cfg.key_length == 64


@pytest.mark.parametrize("case", ["qwen2", "qwen3"])
def test_one_forward_equals_prefill_then_single_tokens(tmp_path, case):
    """20 tokens at once against 17 + 1 + 1 + 1 over the live cache: the cache convention (permuted, rotated
    k rows) is self-consistent, and every step agrees with the reference's row."""
    sp = CASES[case]
    m, _, w, _ = _load(tmp_path, sp)
    ids = R.prompt(20, k=3)
    ref = R.ref_logits(sp, w, ids)
    whole = m.forward(ids).double()
    m.reset()
    m.forward(ids[:17])
    for i in (17, 18, 19):
        step = m.forward([ids[i]]).double()
        assert (step - ref[i]).abs().max().item() <= TOL, i
    assert (step - whole).abs().max().item() <= TOL
    assert (whole - ref[19]).abs().max().item() <= TOL


def _main(argv):
    """splainference.main in this process, with the signal handlers it installs put back."""
    from libsplinter_amd.daemons import splainference
    saved = {s: signal.getsignal(s) for s in (signal.SIGINT, signal.SIGTERM)}
    try:
        return splainference.main(argv)
    finally:
        for s, h in saved.items():
            signal.signal(s, h)


@pytest.mark.parametrize("arch,extra", [("gemma2", None), ("phi3", None),
                                        ("llama", {"llama.rope.dimension_count": 32})])
def test_unsupported_files_are_refused(tmp_path, uniq, capsys, arch, extra):
    """gemma2, phi3 and a partial-rotary file (rope.dimension_count 32 of head dim 64): from_gguf raises a
    ValueError that names the architecture and the supported ones; the daemon prints it and exits 1."""
    from libsplinter_amd import Store, unlink
    from libsplinter_amd.models.decoder import CausalLM
    sp = R.spec(arch, seed=6)
    path = R.write_gguf(tmp_path / "m.gguf", sp, R.weights(sp), extra=extra)
    with pytest.raises(ValueError) as ei:
        CausalLM.from_gguf(path, device="cpu")
    msg = str(ei.value)
    assert repr(arch) in msg and all(a in msg for a in ("llama", "qwen2", "qwen3"))
    s = Store.create(uniq, slots=64, max_val=256, embeddings=False)
    try:
        s.set("req", "hello")
        s.set_label("req", WAITING)
        assert _main(["--oneshot", "--device", "cpu", uniq, path, "7"]) == 1
        assert repr(arch) in capsys.readouterr().err
        assert s.snapshot("req")["bloom"] & WAITING and s.get("req") == b"hello"  # nothing was served
    finally:
        s.close()
        unlink(uniq)


def test_yarn_file_is_served_with_the_original_context(tmp_path, capsys):
    from libsplinter_amd.models.decoder import CausalLM
    sp = R.spec("qwen2", d=128, H=2, KVH=1, bias=True, n_ctx=256, scaling=("yarn", 4.0, 64), seed=7)
    w = R.weights(sp)
    m, _ = CausalLM.from_gguf(R.write_gguf(tmp_path / "m.gguf", sp, w), device="cpu")
    assert m.cfg.n_ctx == 64 and m.cos.shape[0] == 64
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "yarn" in out and "64" in out
    ids = R.prompt(24)
    sp_plain = dict(sp, scaling=None)  # inside the original window the unscaled rotation is the model's
    assert (m.forward(ids).double() - R.ref_logits(sp_plain, w, ids)[-1]).abs().max().item() <= TOL


def _same_as_golden(got, name):
    """The fp32 CPU logits of the commit before qwen2 / qwen3 support, stored under tests/golden/decoder_arch.
    On the kind of host that wrote them the new code gives them bit for bit.  Across hosts bits cannot be
    asked of torch's CPU matrix products: that commit itself, run on the MI355X machine's host CPU, differs
    from its own stored values by 1.19e-6 (5 ulp of the largest logit, with 1 thread as with 16).  So the
    bound here is 32 ulp of the largest stored logit (1.1e-5 for logits near 3): a few reordered fp32 sums fit,
    a changed convention (0.7 and more, see the reference tests) or a changed weight do not.  The bit-for-bit
    claim is carried by the GPU goldens of test_decoder_arch_gpu.py, where the arithmetic is the same
    everywhere."""
    want = np.load(os.path.join(GOLDEN, name))
    diff = float(np.abs(got - want).max())
    bound = 32 * 2.0 ** -23 * float(np.abs(want).max())
    print(f"{name}: bit-identical {np.array_equal(got, want)}, max |diff| {diff:.3e}, bound {bound:.3e}")
    assert got.dtype == want.dtype and got.shape == want.shape and diff <= bound


def test_llama_files_and_random_init_keep_their_logits(tmp_path):
    """A file without general.architecture (served as llama) and the --random-init model against the logits
    of the commit before qwen2 / qwen3 support."""
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig
    sp = R.spec("llama", seed=11)
    m, _, _, _ = _load(tmp_path, sp, arch_key=False)
    _same_as_golden(m.forward(R.prompt(24)).numpy(), "noarch_llama_logits.npy")
    assert m.cfg.arch == "llama" and not m.cfg.qkv_bias and not m.cfg.qk_norm and m.cfg.key_length is None
    m = CausalLM.random(DecoderConfig(), device="cpu")
    _same_as_golden(m.forward([256] + list(b"hello there, decoder")).numpy(), "random_init_logits.npy")


def test_neox_permutation_is_rows_j_and_j_plus_half():
    import torch
    from libsplinter_amd.models.decoder import neox_rows_to_pairs
    t = torch.arange(2 * 8 * 3, dtype=torch.float32).reshape(16, 3)  # 2 heads of hd 8
    p = neox_rows_to_pairs(t, 8)
    for h in range(2):
        for j in range(4):
            assert torch.equal(p[h * 8 + 2 * j], t[h * 8 + j]) and torch.equal(p[h * 8 + 2 * j + 1], t[h * 8 + j + 4])
    v = torch.arange(8, dtype=torch.float32)
    assert neox_rows_to_pairs(v, 8).tolist() == [0, 4, 1, 5, 2, 6, 3, 7]


def test_state_machine_over_a_qwen2_file(tmp_path, uniq):
    """A WAITING key served from the qwen2 GGUF (byte-level BPE vocabulary, chatml template): the prompt is the
    chatml rendering, a completion follows it, the key ends READY."""
    from libsplinter_amd import Store, unlink
    sp = CASES["qwen2"]
    path = R.write_gguf(tmp_path / "m.gguf", sp, R.weights(sp), tokenizer=True)
    s = Store.create(uniq, slots=64, max_val=512, embeddings=False)
    try:
        s.set("req", "hello there")
        s.set_label("req", WAITING)
        assert _main(["--oneshot", "--device", "cpu", "--max-tokens", "12", "--seed", "5", uniq, path, "7"]) == 0
        head = b"<|im_start|>user\nhello there<|im_end|>\n<|im_start|>assistant\n"
        v = s.get("req")
        assert v.startswith(head) and len(v) > len(head)
        b = s.snapshot("req")["bloom"]
        assert b & READY and not b & (WAITING | SERVICING)
        assert "[DONE]: Completion written to key: req" in s.get("__debug").decode()
    finally:
        s.close()
        unlink(uniq)
