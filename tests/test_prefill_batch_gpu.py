"""Batched, chunked prompt prefill (BatchDecodeEngine.submit / prefill): the two segment kernels
(dec_attn_prefill_kv_seg in csrc/hip/decoder_kernels.hip, dec_rope_kv_seg in csrc/hip/decoder_batch.hip)
against the single-prompt kernels bit for bit and against fp32, the GEMM property the engine's co-admission
independence rests on, and the engine against the eager forward, alone and next to a live stream."""
import pytest

pytestmark = pytest.mark.gpu

N_CTX, NSLOTS = 1024, 6
# (row0, n, pos0, slot): one row, the 128-row q-block edge on both sides, key-tile edges, fresh and continued
# prompts, in shuffled slots (slot 2 stays unused) and with unowned rows between the segments
SEGS = [(3, 1, 0, 4), (8, 5, 37, 1), (16, 128, 0, 5), (150, 129, 200, 0), (290, 200, 511, 3)]
T_ROWS = 500
SHAPES = [(64, 8, 2), (128, 4, 4)]


def _model(hd, H, KVH):
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig
    return CausalLM.random(DecoderConfig(layers=1, d=H * hd, heads=H, kv_heads=KVH, n_ctx=N_CTX), seed=1, device="cuda")


def _table(segs):
    import numpy as np
    return np.ascontiguousarray(np.array(segs, dtype=np.int32).reshape(-1, 4))


def _attn_seg(L, qkv, kv, segs, H, KVH, hd, out, nslots=NSLOTS, n_ctx=N_CTX, T=T_ROWS):
    tb = _table(segs)
    return L.dec_attn_prefill_kv_seg(qkv.data_ptr(), qkv.stride(0), T, tb.ctypes.data, len(segs), kv[0, 0].data_ptr(),
                                     kv[0, 1].data_ptr(), KVH * hd, kv.stride(0), nslots, n_ctx, H, KVH, hd,
                                     hd ** -0.5, out.data_ptr(), out.stride(0), None)


@pytest.mark.parametrize("hd,H,KVH", SHAPES)
def test_attn_prefill_kv_seg_equals_single_prompt_kernel(hd, H, KVH):
    """Five segments in one launch: each equals dec_attn_prefill_kv run on it alone bit for bit and fp32 causal
    attention within 3e-2; rows no segment owns keep their sentinel; bad tables are refused with nothing
    written."""
    import torch
    L = _model(hd, H, KVH).L
    g = torch.Generator(device="cuda").manual_seed(61)
    ldq = (H + 2 * KVH) * hd
    kv = torch.randn((NSLOTS, 2, N_CTX, KVH, hd), device="cuda", generator=g).to(torch.bfloat16)
    qkv = torch.randn((T_ROWS, ldq), device="cuda", generator=g).to(torch.bfloat16)
    out = torch.full((T_ROWS, H * hd), 7.0, device="cuda", dtype=torch.bfloat16)
    assert _attn_seg(L, qkv, kv, SEGS, H, KVH, hd, out) == 0
    torch.cuda.synchronize()
    owned = torch.zeros(T_ROWS, dtype=torch.bool, device="cuda")
    for row0, n, pos0, slot in SEGS:
        owned[row0: row0 + n] = True
        one = torch.full((n, H * hd), 7.0, device="cuda", dtype=torch.bfloat16)
        q1 = qkv[row0: row0 + n]
        assert L.dec_attn_prefill_kv(q1.data_ptr(), ldq, kv[slot, 0].data_ptr(), kv[slot, 1].data_ptr(), KVH * hd, n,
                                     pos0, H, KVH, hd, hd ** -0.5, one.data_ptr(), H * hd, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[row0: row0 + n], one), (n, pos0)
        Lk = pos0 + n
        q = q1[:, : H * hd].float().reshape(n, H, hd)
        k = kv[slot, 0, :Lk].float().repeat_interleave(H // KVH, 1)
        v = kv[slot, 1, :Lk].float().repeat_interleave(H // KVH, 1)
        s = torch.einsum("qhd,khd->hqk", q, k) * hd ** -0.5
        qpos = torch.arange(pos0, Lk, device="cuda")[:, None]
        s = s.masked_fill(torch.arange(Lk, device="cuda")[None, :] > qpos, float("-inf"))
        ref = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v).reshape(n, -1)
        err = (out[row0: row0 + n].float() - ref).abs().max().item()
        print(f"attn_seg hd={hd} n={n} pos0={pos0} slot={slot} err={err:.3e}")
        assert err < 3e-2, (n, pos0, err)
    assert bool((out[~owned] == 7.0).all()), "a row outside the segments was written"
    # refused tables: non-zero return, outputs untouched
    clean = torch.full_like(out, 7.0)
    bad = {"slot >= nslots": [(0, 4, 0, NSLOTS)],
           "pos0 + n > n_ctx": [(0, 30, N_CTX - 29, 0)],
           "overlapping rows": [(0, 10, 0, 0), (9, 4, 0, 1)],
           "17 segments": [(i, 1, 0, i) for i in range(17)],
           "empty segment": [(0, 0, 0, 0)],
           "rows past T": [(T_ROWS - 3, 4, 0, 0)]}
    for what, segs in bad.items():
        out.fill_(7.0)
        ns = 32 if what == "17 segments" else NSLOTS
        assert _attn_seg(L, qkv, kv, segs, H, KVH, hd, out, nslots=ns) != 0, what
        torch.cuda.synchronize()
        assert torch.equal(out, clean), what
    assert _attn_seg(L, qkv, kv, SEGS[:2], H, KVH, 96, out) != 0  # head dim 96
    torch.cuda.synchronize()
    assert torch.equal(out, clean)


@pytest.mark.parametrize("hd,H,KVH", SHAPES)
def test_rope_kv_seg_equals_rope_plus_slice_copies(hd, H, KVH):
    """The same segment mix: rotated q rows and the cache rows written equal dec_rope followed by the two slice
    copies of CausalLM.forward bit for bit; every other qkv element and every other cache row of every slot
    stays as it was."""
    import torch
    m = _model(hd, H, KVH)
    L = m.L
    g = torch.Generator(device="cuda").manual_seed(62)
    ld = (H + 2 * KVH) * hd
    qc, kc = H * hd, KVH * hd
    qkv0 = torch.randn((T_ROWS, ld), device="cuda", generator=g).to(torch.bfloat16)
    qkv = qkv0.clone()
    kv = torch.full((NSLOTS, 2, N_CTX, KVH, hd), 7.0, device="cuda", dtype=torch.bfloat16)
    tb = _table(SEGS)

    def run(buf, cache, table, nseg, hd_=hd, nslots=NSLOTS):
        return L.dec_rope_kv_seg(buf.data_ptr(), ld, T_ROWS, table.ctypes.data, nseg, H, KVH, hd_, m.cos.data_ptr(),
                                 m.sin.data_ptr(), cache[0, 0].data_ptr(), cache[0, 1].data_ptr(), kc, cache.stride(0),
                                 nslots, N_CTX, None)

    assert run(qkv, kv, tb, len(SEGS)) == 0
    torch.cuda.synchronize()
    want_q, want_kv = qkv0.clone(), torch.full_like(kv, 7.0)
    for row0, n, pos0, slot in SEGS:
        r = qkv0[row0: row0 + n].clone()
        assert L.dec_rope(r.data_ptr(), ld, n, qc + kc, hd, pos0, m.cos.data_ptr(), m.sin.data_ptr(), None) == 0
        torch.cuda.synchronize()
        want_q[row0: row0 + n, :qc] = r[:, :qc]
        want_kv[slot, 0, pos0: pos0 + n] = r[:, qc: qc + kc].reshape(n, KVH, hd)
        want_kv[slot, 1, pos0: pos0 + n] = r[:, qc + kc:].reshape(n, KVH, hd)
        if pos0 + n > 1:  # position 0 alone rotates by nothing
            assert not torch.equal(r[:, :qc], qkv0[row0: row0 + n, :qc])
    assert torch.equal(qkv, want_q)
    assert torch.equal(kv, want_kv)
    # refused tables leave both buffers alone
    for segs in ([(0, 4, 0, NSLOTS)], [(0, 30, N_CTX - 29, 0)], [(0, 10, 0, 0), (9, 4, 0, 1)],
                 [(i, 1, 0, i) for i in range(17)]):
        assert run(qkv, kv, _table(segs), len(segs), nslots=32 if len(segs) == 17 else NSLOTS) != 0, segs
    assert run(qkv, kv, tb, len(SEGS), hd_=96) != 0
    torch.cuda.synchronize()
    assert torch.equal(qkv, want_q) and torch.equal(kv, want_kv)


def test_gemm_rows_do_not_depend_on_row_count_or_place():
    """What the engine's co-admission independence rests on: a prefill pass forces the 128 x 128 GEMM kernel,
    and on that kernel a block of 128 rows gives the same bits as M = 128 alone and at rows 37 .. 164 of an
    M = 1024 operand, in every epilogue a pass uses.  Whether the 256 x 256 kernel (which the automatic choice
    would take for a large pass) gives the same bits is printed, not assumed."""
    import torch
    from libsplinter_amd.models.nomic import _lib
    L = _lib()
    g = torch.Generator(device="cuda").manual_seed(63)
    M, K, N, r0 = 1024, 512, 512, 37
    A = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16)
    W = (torch.randn((N, K), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    R = torch.randn((M, N), device="cuda", generator=g).to(torch.bfloat16)
    a1, r1 = A[r0: r0 + 128].contiguous(), R[r0: r0 + 128].contiguous()

    def gemm(mode, a, res, rows):
        cols = N // 2 if mode == 2 else N
        out = torch.zeros((rows, cols), device="cuda", dtype=torch.float32 if mode == 4 else torch.bfloat16)
        rp, ldr = (res.data_ptr(), N) if mode == 1 else (None, 0)
        assert L.nomic_gemm(mode, a.data_ptr(), K, W.data_ptr(), K, rows, N, K, out.data_ptr(), cols, rp, ldr, None,
                            None, 0, None) == 0
        torch.cuda.synchronize()
        return out

    prev = L.nomic_gemm_set_variant(128)
    try:
        for mode in (0, 1, 2, 4):
            small = gemm(mode, a1, r1, 128)
            big = gemm(mode, A, R, M)
            assert torch.equal(small, big[r0: r0 + 128]), f"128^2 kernel: mode {mode} rows moved with M / place"
            L.nomic_gemm_set_variant(256)
            big256 = gemm(mode, A, R, M)
            L.nomic_gemm_set_variant(128)
            print(f"gemm mode {mode}: 128^2 (M=128) vs 256^2 (M=1024) bits "
                  f"{'match' if torch.equal(small, big256[r0: r0 + 128]) else 'DIFFER'}")
    finally:
        L.nomic_gemm_set_variant(prev)


def _prompts():
    return [[256] + [97 + (i * (k + 3)) % 26 for i in range(n - 1)] for k, n in enumerate((5, 27, 200))]


def _prefill_all(eng, chunk):
    """prefill until nothing is pending: [(pass number, {slot: first token})] of the passes that ended a prompt"""
    firsts, passes = [], 0
    while eng.pending():
        passes += 1
        got = eng.prefill(chunk)
        if got:
            firsts.append((passes, got))
        assert passes < 100
    return passes, firsts


@pytest.mark.parametrize("quant", ["bf16", "q4"])
def test_engine_batched_prefill_matches_eager_and_is_independent(quant):
    """Prompts of 5, 27 and 200 tokens submitted together, chunk 64: 4 passes, first tokens in passes 1, 1 and 4;
    five teacher-forced steps match each prompt's own eager forward; the 200-token prompt prefilled alone (in
    another slot, with nothing sharing its passes) has the same first token, cache rows and next logits, bit
    for bit."""
    import torch
    from libsplinter_amd.models.decoder import BatchDecodeEngine, CausalLM, DecoderConfig
    cfg = DecoderConfig(layers=2, kv_heads=2)
    mdl = CausalLM.random(cfg, seed=4, device="cuda", quant=quant)
    prompts = _prompts()
    eng = BatchDecodeEngine(mdl, max_seqs=4, use_graph=False)
    slots = [eng.submit(ids, seed=11 + k) for k, ids in enumerate(prompts)]
    assert slots == [0, 1, 2] and eng.pending() == [0, 1, 2] and eng.active() == []
    assert eng.step() == {}  # pending slots are not live
    passes, firsts = _prefill_all(eng, 64)
    assert passes == 4 and eng.prefill_passes == 4
    assert [p for p, _ in firsts] == [1, 4] and sorted(firsts[0][1]) == [0, 1] and sorted(firsts[1][1]) == [2]
    assert eng.active() == [0, 1, 2] and eng.pos[:3] == [5, 27, 200] and eng.prefill(64) == {}
    first_long = firsts[1][1][2]
    cache_long = eng.kv[2, :, :, :200].clone()
    eagers = []
    for ids in prompts:
        e = CausalLM.random(cfg, seed=4, device="cuda", quant=quant)
        e.forward(ids)
        eagers.append(e)
    long_logits = []
    for i in range(5):
        toks = [72 + i + 3 * k for k in range(3)]
        for s, t in zip(slots, toks):
            eng.set_token(s, t)
        assert sorted(eng.step()) == slots
        long_logits.append(eng.logits[2].clone())
        for k, s in enumerate(slots):
            ref = eagers[k].forward([toks[k]])
            got = eng.logits[s, : cfg.vocab]
            rel = ((got - ref).norm() / ref.norm()).item()
            print(f"{quant} step {i} prompt {k}: rel {rel:.3e}")
            assert rel < 3e-2, (i, k, rel)
    # the long prompt alone
    solo = BatchDecodeEngine(mdl, max_seqs=4, use_graph=False)
    assert solo.submit(prompts[2], seed=13) == 0
    passes, firsts = _prefill_all(solo, 64)
    assert passes == 4 and [p for p, _ in firsts] == [4]
    assert firsts[0][1][0] == first_long
    assert torch.equal(solo.kv[0, :, :, :200], cache_long)
    for i in range(3):
        solo.set_token(0, 72 + i + 6)
        solo.step()
        assert torch.equal(solo.logits[0], long_logits[i]), i


def _generate(eng, slot, first, n):
    toks, lgs = [first], []
    for _ in range(n - 1):
        toks.append(eng.step()[slot])
        lgs.append(eng.logits[slot].clone())
    return toks, lgs


def test_chunked_prefill_leaves_a_live_stream_alone():
    """A is live and generating; B (200 tokens) is submitted after A's 5th step and prefilled with chunk 64, one
    pass per step.  A's 24 tokens and per-step logits are bit-identical to A alone, B's tokens equal B alone,
    and submits never recapture the step."""
    import torch
    from libsplinter_amd.models.decoder import BatchDecodeEngine, ByteTokenizer, CausalLM, DecoderConfig
    cfg = DecoderConfig()
    mask = ByteTokenizer().printable_mask(cfg.vocab)
    mdl = CausalLM.random(cfg, seed=2, device="cuda")
    A = [256] + list(b"<user>\nhello\n<assistant>\n")
    B = [256] + [int(c) for c in (b"<user>\n" + b"tell me more about this, " * 8)[:186]] + list(b"\n<assistant>\n")
    assert len(B) == 200
    mk = lambda: BatchDecodeEngine(mdl, max_seqs=4, seed=99, mask=mask)  # noqa: E731
    eng = mk()
    sa, fa = eng.admit(A, seed=7)
    solo_t, solo_l = _generate(eng, sa, fa, 24)
    eng = mk()
    sb = eng.submit(B, seed=8)
    _, firsts = _prefill_all(eng, 64)
    solo_b, _ = _generate(eng, sb, firsts[0][1][sb], 10)
    eng = mk()
    sa, fa = eng.admit(A, seed=7)
    toks, lgs, btoks = [fa], [], []
    sb, graphs = None, None
    for i in range(23):
        if i == 5:
            graphs = len(eng.graphs)
            sb = eng.submit(B, seed=8)
            assert sb != sa and eng.pending() == [sb]
        if sb is not None and eng.pending():
            got = eng.prefill(64)  # one pass between two steps
            if got:
                btoks.append(got[sb])
        out = eng.step()
        toks.append(out[sa])
        lgs.append(eng.logits[sa].clone())
        if btoks and sb in out and len(btoks) < 10:
            btoks.append(out[sb])
        assert (sb in out) == (sb is not None and not eng.pending())
    assert toks == solo_t
    assert all(torch.equal(a, b) for a, b in zip(lgs, solo_l))
    assert len(btoks) == 10 and btoks == solo_b
    assert len(set(solo_b)) > 3 and all(32 <= t < 127 or t in (10, 257) for t in solo_b)
    assert graphs == 1 and len(eng.graphs) == 1


def test_submit_errors_and_cancel():
    from libsplinter_amd.models.decoder import BatchDecodeEngine, CausalLM, DecoderConfig
    cfg = DecoderConfig(layers=1, n_ctx=64)
    mdl = CausalLM.random(cfg, seed=1, device="cuda")
    eng = BatchDecodeEngine(mdl, max_seqs=2, use_graph=False)
    with pytest.raises(ValueError):
        eng.submit([256] + [97] * 63)  # 64 tokens leave no room in a context of 64
    with pytest.raises(ValueError):
        eng.submit([])
    a = eng.submit([256] + [97] * 40)
    b = eng.submit([256, 98])
    with pytest.raises(RuntimeError):
        eng.submit([256, 99])
    with pytest.raises(RuntimeError):
        eng.admit([256, 99])  # a pending slot is taken for admit as well
    with pytest.raises(ValueError):
        eng.prefill(0)
    eng.release(a)  # cancelled while pending
    assert eng.pending() == [b]
    got = eng.prefill(16)
    assert sorted(got) == [b] and eng.active() == [b] and eng.pending() == []
    assert eng.prefill(16) == {}
    c = eng.submit([256, 100, 101])
    assert c == a and sorted(eng.prefill(16)) == [c]
    assert sorted(eng.step()) == sorted([b, c])
