"""Batched decode (csrc/hip/decoder_batch.hip, models/decoder.py BatchDecodeEngine): the small GEMMs over
1..16 token rows, the slot-indexed embedding / RoPE + cache append / attention / sampler kernels against
the single-sequence kernels and fp32 references, and the engine against the eager forward."""
import pytest

pytestmark = pytest.mark.gpu

ST = 8  # int32 words of a slot's state record: pos, token, step, active, seed lo, seed hi, 0, 0


def _model(**kw):
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig
    return CausalLM.random(DecoderConfig(layers=1, **kw), seed=1, device="cuda")


def _q4_host_dequant(q, sm):
    """Host decoder of the Q4G32 planes: nibble 2j low / 2j+1 high of byte j, one bf16 (d, m) pair per
    32-k group, w = d q + m."""
    import torch
    qi = q.to(torch.int32)
    nib = torch.stack([qi & 15, qi >> 4], -1).reshape(q.shape[0], -1).float()
    smi = sm.to(torch.int64) & 0xFFFFFFFF
    d = ((smi & 0xFFFF) << 16).to(torch.int32).view(torch.float32)
    m = ((smi >> 16) << 16).to(torch.int32).view(torch.float32)
    return nib * d.repeat_interleave(32, 1) + m.repeat_interleave(32, 1)


def _q8_host_dequant(q, sm):
    """Host decoder of the Q8G32 planes: one byte u per weight, bf16 (d, m) per 32-k group, w = d u + m."""
    import torch
    smi = sm.to(torch.int64) & 0xFFFFFFFF
    d = ((smi & 0xFFFF) << 16).to(torch.int32).view(torch.float32)
    m = ((smi >> 16) << 16).to(torch.int32).view(torch.float32)
    return q.float() * d.repeat_interleave(32, 1) + m.repeat_interleave(32, 1)


def _gemm(L, w, mode, x, nseq, N, K, res, out):
    """dec_gemm_small / _q4 / _q8 by the type of ``w`` (a bf16 tensor or a Q4Weight / Q8Weight)."""
    import torch
    rp, ldr = (res.data_ptr(), res.stride(0)) if res is not None else (None, 0)
    if isinstance(w, torch.Tensor):
        return L.dec_gemm_small(mode, x.data_ptr(), x.stride(0), nseq, w.data_ptr(), N, K, rp, ldr, out.data_ptr(),
                                out.stride(0), None)
    fn = L.dec_gemm_small_q8 if w.bits == 8 else L.dec_gemm_small_q4
    return fn(mode, x.data_ptr(), x.stride(0), nseq, w.q.data_ptr(), w.sm.data_ptr(), N, K, rp, ldr, out.data_ptr(),
              out.stride(0), None)


def _swiglu_ref(y):
    import torch
    yg = y.reshape(y.shape[0], -1, 2, 16)
    u, g = yg[:, :, 0].reshape(y.shape[0], -1), yg[:, :, 1].reshape(y.shape[0], -1)
    return u * torch.nn.functional.silu(g)


def _run_modes(L, w, wug, Wf, Wugf, x, res, nseq, N, K, tol16, tol32):
    """Every mode of one small GEMM against fp32 (Wf: the fp32 weights the kernel stands for); returns the
    outputs so the caller can compare runs bit for bit."""
    import torch
    outs = {}
    xf = x[:nseq].float()
    for mode in (0, 1, 4):
        out = torch.full((nseq, N + 8), 7.0, device="cuda", dtype=torch.float32 if mode == 4 else torch.bfloat16)
        assert _gemm(L, w, mode, x, nseq, N, K, res if mode == 1 else None, out) == 0
        torch.cuda.synchronize()
        ref = xf @ Wf.T + (res[:nseq].float() if mode == 1 else 0)
        err = (out[:, :N].float() - ref).abs().max().item()
        tol = (tol32 if mode == 4 else tol16) * max(1.0, ref.abs().max().item())
        print(f"gemm_small K={K} N={N} nseq={nseq} mode={mode} err={err:.3e} tol={tol:.3e}")
        assert err < tol, (mode, nseq, err)
        assert bool((out[:, N:] == 7.0).all()), "columns past N were written"
        outs[mode] = out.clone()
    if wug is not None:
        out = torch.full((nseq, N // 2), 7.0, device="cuda", dtype=torch.bfloat16)
        assert _gemm(L, wug, 2, x, nseq, N, K, None, out) == 0
        torch.cuda.synchronize()
        ref = _swiglu_ref(xf @ Wugf.T)
        err = (out.float() - ref).abs().max().item()
        print(f"gemm_small K={K} N={N} nseq={nseq} mode=2 err={err:.3e}")
        assert err < tol16 * max(1.0, ref.abs().max().item()), (2, nseq, err)
        outs[2] = out.clone()
    return outs


@pytest.mark.parametrize("K,N", [(512, 1536), (1536, 512), (4096, 200)])
def test_gemm_small_bf16(K, N):
    """dec_gemm_small in every mode for 1, 3 and 16 token rows against fp32 torch; a row's result is
    bit-identical whatever the other rows hold and across runs; bad shapes are refused."""
    import torch
    from libsplinter_amd.models.nomic import pack_upgate
    L = _model().L
    g = torch.Generator(device="cuda").manual_seed(21)
    ldx = K + 64 if K == 512 else K  # one case with padded token rows
    x = torch.randn((16, ldx), device="cuda", generator=g).to(torch.bfloat16)[:, :K]
    W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    res = torch.randn((16, N), device="cuda", generator=g).to(torch.bfloat16)
    ug = None
    if N % 32 == 0:
        gate = (torch.randn((N // 2, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
        ug = pack_upgate(W[: N // 2], gate).contiguous()
    for nseq in (1, 3, 16):
        a = _run_modes(L, W, ug, W.float(), ug.float() if ug is not None else None, x, res, nseq, N, K, 2e-2, 2e-2)
        b = _run_modes(L, W, ug, W.float(), ug.float() if ug is not None else None, x, res, nseq, N, K, 2e-2, 2e-2)
        for mode in a:
            assert torch.equal(a[mode], b[mode]), ("not reproducible", mode, nseq)
    # row independence: row 2 of 16 with the other rows zero or random
    xz = torch.zeros_like(x)
    xz[2] = x[2]
    for mode in (0, 4) + ((2,) if ug is not None else ()):
        w, cols = (ug, N // 2) if mode == 2 else (W, N)
        o1 = torch.zeros((16, cols), device="cuda", dtype=torch.float32 if mode == 4 else torch.bfloat16)
        o2 = torch.zeros_like(o1)
        assert _gemm(L, w, mode, x, 16, N, K, None, o1) == 0 and _gemm(L, w, mode, xz, 16, N, K, None, o2) == 0
        torch.cuda.synchronize()
        assert torch.equal(o1[2], o2[2]), mode
    out = torch.zeros((16, N), device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, W, 0, x, 0, N, K, None, out) != 0
    assert _gemm(L, W, 0, x, 17, N, K, None, out) != 0
    assert _gemm(L, W, 0, x, 4, N, K - 4, None, out) != 0
    assert _gemm(L, W, 3, x, 4, N, K, None, out) != 0


@pytest.mark.parametrize("bits,K,N", [(4, 512, 1536), (4, 11008, 96), (8, 512, 1536), (8, 4096, 96)])
def test_gemm_small_q4_q8(bits, K, N):
    """dec_gemm_small_q4 / _q8 (integer codes through the MFMA, fp32 (d, m) per k-step) against the host
    decoders of the planes, mode 2 through pack_upgate, 1 / 5 / 16 token rows."""
    import torch
    from libsplinter_amd.models.decoder import Q4Weight, Q8Weight
    from libsplinter_amd.models.nomic import pack_upgate
    L = _model().L
    cls, deq = (Q4Weight, _q4_host_dequant) if bits == 4 else (Q8Weight, _q8_host_dequant)
    g = torch.Generator(device="cuda").manual_seed(22 + bits)
    W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    gate = (torch.randn((N // 2, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    qw = cls.quantize(L, W)
    qug = cls.quantize(L, pack_upgate(W[: N // 2], gate).contiguous())
    torch.cuda.synchronize()
    Wf, Wugf = deq(qw.q, qw.sm), deq(qug.q, qug.sm)
    x = torch.randn((16, K), device="cuda", generator=g).to(torch.bfloat16)
    res = torch.randn((16, N), device="cuda", generator=g).to(torch.bfloat16)
    for nseq in (1, 5, 16):
        a = _run_modes(L, qw, qug, Wf, Wugf, x, res, nseq, N, K, 1e-2, 1e-3)
        b = _run_modes(L, qw, qug, Wf, Wugf, x, res, nseq, N, K, 1e-2, 1e-3)
        for mode in a:
            assert torch.equal(a[mode], b[mode]), ("not reproducible", mode, nseq)
    out = torch.zeros((16, N), device="cuda", dtype=torch.bfloat16)
    assert _gemm(L, qw, 0, x, 4, N, K - 8, None, out) != 0  # K % 32


def _state(rows):
    """int32 [n, 8] device state from (pos, token, step, active, seed) tuples."""
    import torch
    st = torch.zeros((len(rows), ST), dtype=torch.int64)
    for b, (pos, tok, step, act, seed) in enumerate(rows):
        st[b, :6] = torch.tensor([pos, tok, step, act, seed & 0xFFFFFFFF, seed >> 32])
    st = torch.where(st >= 2 ** 31, st - 2 ** 32, st)
    return st.to(torch.int32).cuda()


@pytest.mark.parametrize("hd,H,KVH", [(128, 32, 8), (64, 8, 8), (128, 12, 4)])
def test_attn_decode_b_vs_fp32(hd, H, KVH):
    """dec_attn_decode_b: every slot over its own cache and length in one launch, the single-workgroup
    kernels at span 512 and the split form + combine at span 2048 (short slots run empty splits); an
    inactive slot's output row stays as it was."""
    import torch
    L = _model().L
    g = torch.Generator(device="cuda").manual_seed(31)
    for span, lens in ((512, [1, 63, 64, 65, 300, 512]), (2048, [1, 513, 700, 1100])):
        n = len(lens) + 1
        cap = max(lens)
        kv = torch.randn((n, 2, cap, KVH, hd), device="cuda", generator=g).to(torch.bfloat16)
        q = torch.randn((n, H * hd + 64), device="cuda", generator=g).to(torch.bfloat16)
        dead = 2  # the inactive slot sits between live ones
        order = lens[:dead] + [100] + lens[dead:]
        st = _state([(ln - 1, 0, 0, int(b != dead), 0) for b, ln in enumerate(order)])
        out = torch.full((n, H * hd), float("nan"), device="cuda").to(torch.bfloat16)
        ws = torch.empty(L.dec_attn_b_ws_floats(n, H, hd), dtype=torch.float32, device="cuda")
        assert L.dec_attn_decode_b(q.data_ptr(), q.stride(0), kv[0, 0].data_ptr(), kv[0, 1].data_ptr(), KVH * hd,
                                   kv.stride(0), span, n, H, KVH, hd, hd ** -0.5, out.data_ptr(), out.stride(0),
                                   st.data_ptr(), ws.data_ptr(), None) == 0
        torch.cuda.synchronize()
        for b, ln in enumerate(order):
            if b == dead:
                assert bool(out[b].float().isnan().all()), "inactive slot's row was written"
                continue
            qf = q[b, : H * hd].float().reshape(H, hd)
            kf = kv[b, 0, :ln].float().repeat_interleave(H // KVH, 1)
            vf = kv[b, 1, :ln].float().repeat_interleave(H // KVH, 1)
            p = torch.softmax(torch.einsum("hd,lhd->hl", qf, kf) * hd ** -0.5, -1)
            ref = torch.einsum("hl,lhd->hd", p, vf).reshape(-1)
            err = (out[b].float() - ref).abs().max().item()
            assert err < 2e-2 * max(1.0, ref.abs().max().item()), (span, ln, err)


def test_embed_tok_b_and_rope_kv_b_equal_single_sequence_kernels():
    """Three slots at different positions and one inactive: embedding rows, rotated q and the appended k / v
    rows are bit-equal to dec_embed_tok / dec_rope_kv run per slot; nothing else in the caches, the inactive
    slot's rows or the state moves."""
    import torch
    m = _model(kv_heads=2)
    cfg, L = m.cfg, m.L
    H, KVH, hd = cfg.heads, cfg.kv_heads, cfg.head_dim
    g = torch.Generator(device="cuda").manual_seed(41)
    rows = [(5, 65, 0, 1, 1), (0, 300, 3, 1, 2), (77, 9, 0, 0, 3), (1999, 257, 9, 1, 4)]
    n = len(rows)
    st = _state(rows)
    st0 = st.clone()
    x = torch.full((n, cfg.d + 8), 3.0, device="cuda", dtype=torch.bfloat16)
    assert L.dec_embed_tok_b(m.emb.data_ptr(), cfg.d, st.data_ptr(), n, x.data_ptr(), x.stride(0), None) == 0
    ld = (H + 2 * KVH) * hd
    qkv = torch.randn((n, ld), device="cuda", generator=g).to(torch.bfloat16)
    qkv0 = qkv.clone()
    kv = torch.randn((n, 2, cfg.n_ctx, KVH, hd), device="cuda", generator=g).to(torch.bfloat16)
    kv0 = kv.clone()
    assert L.dec_rope_kv_b(qkv.data_ptr(), ld, n, H, KVH, hd, m.cos.data_ptr(), m.sin.data_ptr(), st.data_ptr(),
                           kv[0, 0].data_ptr(), kv[0, 1].data_ptr(), KVH * hd, kv.stride(0), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(st, st0)
    for b, (pos, tok, _, act, _) in enumerate(rows):
        if not act:
            assert bool((x[b] == 3.0).all()) and torch.equal(qkv[b], qkv0[b]) and torch.equal(kv[b], kv0[b])
            continue
        s1 = torch.tensor([pos, tok, 0, 0], dtype=torch.int32, device="cuda")
        x1 = torch.empty(cfg.d, device="cuda", dtype=torch.bfloat16)
        assert L.dec_embed_tok(m.emb.data_ptr(), cfg.d, s1.data_ptr(), x1.data_ptr(), None) == 0
        q1, kv1 = qkv0[b].clone(), kv0[b].clone()
        assert L.dec_rope_kv(q1.data_ptr(), H, KVH, hd, m.cos.data_ptr(), m.sin.data_ptr(), s1.data_ptr(),
                             kv1[0].data_ptr(), kv1[1].data_ptr(), KVH * hd, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(x[b, : cfg.d], x1) and bool((x[b, cfg.d:] == 3.0).all())
        assert torch.equal(qkv[b], q1)
        assert torch.equal(kv[b], kv1)  # row pos appended, every other row as before
        assert not torch.equal(kv1[:, pos], kv0[b][:, pos])


@pytest.mark.parametrize("V", [384, 5000])
def test_sample_b_draws_the_single_sequence_tokens(V):
    """dec_sample_b (register form at V 384, the k_sb_* chain at V 5000): each slot's 50 draws equal
    dec_sample_ws on the same row, seed and draw index; pos / step advance for live slots only and the
    inactive slot reports -1."""
    import torch
    L = _model().L
    g = torch.Generator(device="cuda").manual_seed(51)
    n, dead, inc = 5, 3, 1
    ldl = V + 24
    logits = (torch.randn((n, ldl), device="cuda", generator=g) * 2.0).contiguous()
    mask = (torch.rand(V, device="cuda", generator=g) < 0.8).to(torch.uint8)
    mask[:4] = 1
    seeds = [0xFFFFFFFF, 1, 0x123456789ABCDEF0, 42, 0x8000000080000000]
    rows = [(10 * b, 0, 3 * b, int(b != dead), seeds[b]) for b in range(n)]
    st = _state(rows)
    host = torch.zeros(n, dtype=torch.int32).pin_memory()
    ws = torch.empty(L.dec_sample_b_ws_floats(n), dtype=torch.float32, device="cuda")
    got = []
    for _ in range(50):
        assert L.dec_sample_b(logits.data_ptr(), ldl, n, V, mask.data_ptr(), 0.9, 0.7, st.data_ptr(), inc,
                              host.data_ptr(), ws.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got.append(host.tolist())
    ws1 = torch.empty(L.dec_sample_ws_floats(), dtype=torch.float32, device="cuda")
    h1 = torch.zeros(1, dtype=torch.int32).pin_memory()
    for b, (pos, _, step, act, seed) in enumerate(rows):
        if not act:
            assert all(r[b] == -1 for r in got)
            assert st[b].tolist()[:4] == [pos, 0, step, 0]
            continue
        s1 = torch.tensor([pos, 0, step, 0], dtype=torch.int32, device="cuda")
        want = []
        for _ in range(50):
            assert L.dec_sample_ws(logits[b].data_ptr(), V, mask.data_ptr(), 0.9, 0.7, seed, s1.data_ptr(), inc,
                                   h1.data_ptr(), ws1.data_ptr(), None) == 0
            torch.cuda.synchronize()
            want.append(int(h1[0]))
        assert [r[b] for r in got] == want, b
        assert len(set(want)) > 3  # the draws move
        assert st[b].tolist()[:4] == [pos + 50 * inc, want[-1], step + 50, 1]


@pytest.mark.parametrize("quant", ["bf16", "q4"])
@pytest.mark.parametrize("graph", [False, True])
def test_engine_steps_match_eager_forward(quant, graph):
    """Three sequences (prompts of 5, 27 and 200 tokens) stepped together, teacher forced: each slot's logits
    against its own eager CausalLM.forward."""
    import torch
    from libsplinter_amd.models.decoder import BatchDecodeEngine, CausalLM, DecoderConfig
    cfg = DecoderConfig(layers=2, kv_heads=2)
    mdl = CausalLM.random(cfg, seed=4, device="cuda", quant=quant)
    eng = BatchDecodeEngine(mdl, max_seqs=4, use_graph=graph)
    prompts = [[256] + [97 + (i * (k + 3)) % 26 for i in range(n - 1)] for k, n in enumerate((5, 27, 200))]
    eagers, slots = [], []
    for ids in prompts:
        e = CausalLM.random(cfg, seed=4, device="cuda", quant=quant)
        e.forward(ids)
        eagers.append(e)
        slots.append(eng.admit(ids)[0])
    assert slots == [0, 1, 2] and mdl.kv is None and mdl.pos == 0
    for i in range(5):
        toks = [72 + i + 3 * k for k in range(3)]
        for s, t in zip(slots, toks):
            eng.set_token(s, t)
        out = eng.step()
        assert sorted(out) == slots
        for k, s in enumerate(slots):
            ref = eagers[k].forward([toks[k]])
            got = eng.logits[s, : cfg.vocab]
            rel = ((got - ref).norm() / ref.norm()).item()
            assert rel < 3e-2, (i, k, rel)
    assert int(eng.host_tok[3]) == -1
    if graph:
        assert len(eng.graphs) == 1


def _generate(eng, slot, first, n, others=None):
    """n tokens and per-step logits of ``slot`` (after ``first``)."""
    toks, lgs = [first], []
    for _ in range(n - 1):
        toks.append(eng.step()[slot])
        lgs.append(eng.logits[slot].clone())
    return toks, lgs


def test_continuous_batching_leaves_a_sequence_alone():
    """A's 24 tokens and per-step logits are bit-identical whether it runs alone or while B joins after 5
    steps, leaves after 6 more and C takes B's slot; C equals C generated alone."""
    import torch
    from libsplinter_amd.models.decoder import BatchDecodeEngine, ByteTokenizer, CausalLM, DecoderConfig
    cfg = DecoderConfig()
    mask = ByteTokenizer().printable_mask(cfg.vocab)
    mdl = CausalLM.random(cfg, seed=2, device="cuda")
    A = [256] + list(b"<user>\nhello\n<assistant>\n")
    B = [256] + list(b"<user>\nsomething longer to say here\n<assistant>\n")
    C = [256] + list(b"<user>\nthird\n<assistant>\n")
    mk = lambda: BatchDecodeEngine(mdl, max_seqs=4, seed=99, mask=mask)  # noqa: E731
    eng = mk()
    sa, fa = eng.admit(A, seed=7)
    solo_t, solo_l = _generate(eng, sa, fa, 24)
    eng = mk()
    sc, fc = eng.admit(C, seed=9)
    solo_c, _ = _generate(eng, sc, fc, 10)
    eng = mk()
    sa, fa = eng.admit(A, seed=7)
    toks, lgs, ctoks = [fa], [], []
    sb = sc = None
    for i in range(23):
        if i == 5:
            sb, _ = eng.admit(B, seed=8)
        if i == 11:
            eng.release(sb)
            sc, fc = eng.admit(C, seed=9)
            assert sc == sb
            ctoks.append(fc)
        out = eng.step()
        toks.append(out[sa])
        lgs.append(eng.logits[sa].clone())
        assert (sb in out) == (5 <= i < 11 or i >= 11)
        if sc is not None and len(ctoks) < 10:
            ctoks.append(out[sc])
    assert toks == solo_t
    assert all(torch.equal(a, b) for a, b in zip(lgs, solo_l))
    assert ctoks == solo_c
    assert len(set(solo_t)) > 3 and all(32 <= t < 127 or t in (10, 257) for t in solo_t)
    assert len(eng.graphs) == 1  # admit / release never recapture
    eng.release(sa)
    with pytest.raises(ValueError):
        eng.release(sa)


def test_engine_mixed_spans_cross_512():
    """One slot at 505 cached keys and one at 20, 16 graph-replayed steps: the long slot crosses 512 and the
    step moves from the span-512 graph to the capacity graph; both slots match eager; two graphs."""
    from libsplinter_amd.models.decoder import BatchDecodeEngine, CausalLM, DecoderConfig
    cfg = DecoderConfig(layers=2, kv_heads=2, n_ctx=2048)
    mdl = CausalLM.random(cfg, seed=6, device="cuda")
    eng = BatchDecodeEngine(mdl, max_seqs=2)
    prompts = [[256] + [int(b) for b in (b"abcdefghij" * 51)[:504]], [256] + list(b"a short prompt here")]
    assert [len(p) for p in prompts] == [505, 20]
    eagers = []
    for ids in prompts:
        e = CausalLM.random(cfg, seed=6, device="cuda")
        e.forward(ids)
        eagers.append(e)
        eng.admit(ids)
    for i in range(16):
        toks = [97 + i % 26, 65 + i % 26]
        for s in (0, 1):
            eng.set_token(s, toks[s])
        eng.step()
        for s in (0, 1):
            ref = eagers[s].forward([toks[s]])
            got = eng.logits[s, : cfg.vocab]
            rel = ((got - ref).norm() / ref.norm()).item()
            assert rel < 3e-2, (i, s, rel)
    assert len(eng.graphs) == 2
    assert eng.pos == [521, 36]


def test_engine_refuses_full_slots_and_context_overrun():
    from libsplinter_amd.models.decoder import BatchDecodeEngine, CausalLM, DecoderConfig
    cfg = DecoderConfig(layers=1, n_ctx=64)
    mdl = CausalLM.random(cfg, seed=1, device="cuda")
    with pytest.raises(ValueError):
        BatchDecodeEngine(mdl, max_seqs=17)
    eng = BatchDecodeEngine(mdl, max_seqs=2, use_graph=False)
    eng.admit([256] + [97] * 61)
    eng.admit([256, 98])
    with pytest.raises(RuntimeError):
        eng.admit([256, 99])
    eng.step()
    eng.step()  # slot 0 now holds 64 tokens: the next step would write row 64
    with pytest.raises(ValueError):
        eng.step()
