"""Mixture-of-experts decoders on the CPU path (models/decoder.py): synthetic qwen3moe and mixtral-style GGUFs
(tests/decoder_moe_ref.py) -- their config, the refusal by name of what is not computed, the plain-torch forward
against the fp64 reference, the quant detection over the stacked expert tensors, the lazy tensor mapping, and
the daemon over a qwen3moe file.

Tolerance of the logit tests: test_decoder_arch_cpu's TOL, max |logit - fp64| <= 1e-4 (fp32 torch against fp64 on
2 layers, d 128).  The reference is run FORCED to the model's routing and the model's routing must equal the
reference's free choice: an fp32 router against an fp64 one flips a top-2 of 8 only on a gap below ~1e-6, which
these seeds do not have."""
import numpy as np
import pytest

import decoder_arch_ref as R
import decoder_moe_ref as M
from test_decoder_arch_cpu import READY, SERVICING, TOL, WAITING, _main

CASES = {"qwen3moe": M.spec("qwen3moe", seed=21), "mixtral": M.spec("llama", seed=22)}


def _load(tmp_path, sp, w=None, **kw):
    from libsplinter_amd.models.decoder import CausalLM
    w = w or M.weights(sp)
    path = M.write_gguf(tmp_path / "m.gguf", sp, w, **kw)
    m, tok = CausalLM.from_gguf(path, device="cpu")
    return m, tok, w, path


@pytest.mark.parametrize("case", list(CASES))
def test_config_from_gguf(tmp_path, case):
    from libsplinter_amd.models.decoder import config_from_gguf
    from libsplinter_amd.models.gguf import GGUFFile
    sp = CASES[case]
    cfg = config_from_gguf(GGUFFile(M.write_gguf(tmp_path / "m.gguf", sp, M.weights(sp))))
    assert (cfg.experts, cfg.experts_used, cfg.expert_ffn) == (8, 2, 64)
    assert (cfg.d, cfg.layers, cfg.arch) == (128, 2, sp["arch"])
    assert cfg.qk_norm == (case == "qwen3moe")
    # a dense file keeps experts 0
    dsp = R.spec("llama", seed=3)
    dcfg = config_from_gguf(GGUFFile(R.write_gguf(tmp_path / "d.gguf", dsp, R.weights(dsp))))
    assert (dcfg.experts, dcfg.experts_used, dcfg.expert_ffn) == (0, 0, 0)


@pytest.mark.parametrize("case", list(CASES))
def test_logits_match_fp64_reference(tmp_path, case):
    import torch
    sp = CASES[case]
    m, _, w, _ = _load(tmp_path, sp)
    ids = R.prompt(24)
    m.route_log = []
    got = m.forward(ids).double()
    chosen = [t.long() for t in m.route_log]
    assert len(chosen) == sp["layers"] and all(c.shape == (24, 2) for c in chosen)
    ref, _, free = M.ref_logits(sp, w, ids, forced=chosen)
    err = (got - ref[-1]).abs().max().item()
    print(f"{case}: max |logit - fp64| = {err:.3e}, max |logit| = {ref.abs().max().item():.2f}")
    assert err <= TOL and torch.isfinite(got).all()
    own = M.ref_logits(sp, w, ids)[2]
    assert all(torch.equal(a, b) for a, b in zip(chosen, own))
    # more than one expert is in use, or the test shows nothing about routing
    assert len(torch.cat(chosen).unique()) > 2
    # prefill then single tokens over the live cache agree with the one forward
    m.reset()
    m.route_log = None
    m.forward(ids[:21])
    for i in (21, 22, 23):
        step = m.forward([ids[i]]).double()
        assert (step - ref[i]).abs().max().item() <= TOL, i


def test_route_force_replaces_the_choice_and_keeps_the_models_probabilities(tmp_path):
    import torch
    sp = CASES["qwen3moe"]
    m, _, w, _ = _load(tmp_path, sp)
    ids = R.prompt(9)
    forced = [torch.tensor([[(t + i) % 8, (t + i + 3) % 8] for t in range(9)]) for i in range(2)]
    m.route_force, m.route_log = forced, []
    got = m.forward(ids).double()
    assert all(torch.equal(a.long(), b) for a, b in zip(m.route_log, forced))
    ref = M.ref_logits(sp, w, ids, forced=forced)[0]
    assert (got - ref[-1]).abs().max().item() <= TOL
    m.route_force = [f + 8 for f in forced]
    m.reset()
    with pytest.raises(ValueError, match="route_force"):
        m.forward(ids)


def _refused(tmp_path, uniq, capsys, sp, w, extra, *named):
    """from_gguf raises a ValueError naming `named` and the supported architectures; the daemon prints it,
    exits 1 and serves nothing."""
    from libsplinter_amd import Store, unlink
    from libsplinter_amd.models.decoder import CausalLM
    path = M.write_gguf(tmp_path / "m.gguf", sp, w, extra=extra)
    with pytest.raises(ValueError) as ei:
        CausalLM.from_gguf(path, device="cpu")
    msg = str(ei.value)
    assert all(n in msg for n in named), msg
    assert all(a in msg for a in ("llama", "qwen2", "qwen3", "qwen3moe")) and repr(sp["arch"]) in msg
    s = Store.create(uniq, slots=64, max_val=256, embeddings=False)
    try:
        s.set("req", "hello")
        s.set_label("req", WAITING)
        assert _main(["--oneshot", "--device", "cpu", uniq, path, "7"]) == 1
        err = capsys.readouterr().err
        assert all(n in err for n in named), err
        assert s.snapshot("req")["bloom"] & WAITING and s.get("req") == b"hello"
    finally:
        s.close()
        unlink(uniq)


def _split(w):
    """Layer 0's experts as the old one-tensor-per-expert layout."""
    w = dict(w)
    for n in ("gate", "up", "down"):
        t = w.pop(f"blk.0.ffn_{n}_exps.weight")
        for e in range(t.shape[0]):
            w[f"blk.0.ffn_{n}.{e}.weight"] = t[e]
    return w


def _mixed(w, sp):
    """Layer 1 dense, layer 0 experts."""
    w = dict(w)
    for n in ("gate_inp", "gate_exps", "up_exps", "down_exps"):
        del w[f"blk.1.ffn_{n}.weight"]
    dw = R.weights(R.spec("llama", ffn=sp["F"], seed=1))
    for n in ("gate", "up", "down"):
        w[f"blk.1.ffn_{n}.weight"] = dw[f"blk.1.ffn_{n}.weight"]
    return w


REFUSALS = {
    "shared_tensor": (lambda w, sp: {**w, "blk.0.ffn_gate_shexp.weight": np.zeros((64, 128), np.float32)}, {},
                      ("shared experts", "blk.0.ffn_gate_shexp.weight")),
    "shared_count": (lambda w, sp: w, {"qwen3moe.expert_shared_count": 1}, ("shared experts", "expert_shared_count 1")),
    "split_tensors": (lambda w, sp: _split(w), {}, ("one tensor per expert", "blk.0.ffn_gate.0.weight")),
    "dense_and_moe": (_mixed, {}, ("dense layers", "blk.1", "expert layers")),
    "too_many_experts": (lambda w, sp: w, {"qwen3moe.expert_count": 257}, ("257 experts",)),
    "too_many_used": (lambda w, sp: w, {"qwen3moe.expert_used_count": 9, "qwen3moe.expert_count": 16},
                      ("16 experts", "9 used")),
    "more_used_than_experts": (lambda w, sp: w, {"qwen3moe.expert_count": 4, "qwen3moe.expert_used_count": 5},
                               ("4 experts", "5 used")),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_unsupported_expert_files_are_refused_by_name(tmp_path, uniq, capsys, case):
    mutate, extra, named = REFUSALS[case]
    sp = M.spec("qwen3moe", seed=23)
    _refused(tmp_path, uniq, capsys, sp, mutate(M.weights(sp), sp), extra, *named)


def test_a_mixtral_file_is_no_longer_a_keyerror(tmp_path):
    """Before expert support a mixtral-style file passed the architecture check and died on blk.0.ffn_gate.weight."""
    m, _, _, _ = _load(tmp_path, CASES["mixtral"])
    assert m.cfg.arch == "llama" and m.cfg.experts == 8 and "router" in m.layers[0]


def test_quant_kind_counts_the_stacked_experts(tmp_path):
    """Experts Q4_0, attention F16: nearly all weights are 4-bit, so the file is served as q4; the same file
    with F16 experts is bf16.  Counting only 2-D tensors saw the attention alone."""
    from libsplinter_amd.models.decoder import gguf_quant_kind
    from libsplinter_amd.models.gguf import GGUFFile, GGUFWriter
    sp = CASES["qwen3moe"]
    w = M.weights(sp)
    for name, et, want in (("q4.gguf", "Q4_0", "q4"), ("f16.gguf", "F16", "bf16")):
        gw = GGUFWriter(str(tmp_path / name), "qwen3moe")
        for n, a in w.items():
            gw.add_tensor(n, a, et if n.endswith("_exps.weight") else ("F16" if a.ndim == 2 else "F32"))
        gw.write()
        assert gguf_quant_kind(GGUFFile(str(tmp_path / name))) == want


def test_from_gguf_dequantises_on_access(tmp_path, monkeypatch):
    """from_gguf hands CausalLM a mapping that converts a tensor when it is taken: every tensor of the file is
    taken exactly once, and no more than one layer's experts are converted between two attention tensors."""
    from libsplinter_amd.models import gguf
    from libsplinter_amd.models.decoder import LazyTensors
    taken = []
    real = gguf.GGUFFile.to_numpy_f32
    monkeypatch.setattr(gguf.GGUFFile, "to_numpy_f32", lambda self, n: (taken.append(n), real(self, n))[1])
    sp = CASES["qwen3moe"]
    _, _, w, _ = _load(tmp_path, sp)
    assert sorted(taken) == sorted(w)
    assert [n for n in taken if "_exps" in n or n.startswith("blk.0.attn_q.") or n.startswith("blk.1.attn_q.")] == \
        ["blk.0.attn_q.weight", "blk.0.ffn_up_exps.weight", "blk.0.ffn_gate_exps.weight", "blk.0.ffn_down_exps.weight",
         "blk.1.attn_q.weight", "blk.1.ffn_up_exps.weight", "blk.1.ffn_gate_exps.weight", "blk.1.ffn_down_exps.weight"]
    lt = LazyTensors(["a"], lambda n: n.upper())
    assert lt["a"] == "A" and "a" in lt and "b" not in lt and list(lt) == ["a"] and lt.get("b") is None
    with pytest.raises(KeyError):
        lt["b"]


def test_random_weights_keep_the_dense_draws():
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig, random_decoder_weights
    dense = random_decoder_weights(DecoderConfig(d=128, heads=2, kv_heads=1, ffn=128, layers=2, vocab=384))
    cfg = DecoderConfig(d=128, heads=2, kv_heads=1, ffn=128, layers=2, vocab=384, experts=4, experts_used=2,
                        expert_ffn=32)
    moe = random_decoder_weights(cfg)
    assert moe["blk.1.ffn_gate_exps.weight"].shape == (4, 32, 128)
    assert moe["blk.1.ffn_down_exps.weight"].shape == (4, 128, 32) and moe["blk.0.ffn_gate_inp.weight"].shape == (4, 128)
    assert "blk.0.ffn_gate.weight" not in moe
    assert np.array_equal(dense["token_embd.weight"], moe["token_embd.weight"])
    assert np.array_equal(dense["blk.0.attn_q.weight"], moe["blk.0.attn_q.weight"])
    import torch
    assert torch.isfinite(CausalLM.random(cfg, device="cpu").forward([256, 1, 2, 3])).all()


def test_state_machine_over_a_qwen3moe_file(tmp_path, uniq):
    from libsplinter_amd import Store, unlink
    sp = CASES["qwen3moe"]
    path = M.write_gguf(tmp_path / "m.gguf", sp, M.weights(sp), tokenizer=True)
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
    finally:
        s.close()
        unlink(uniq)
