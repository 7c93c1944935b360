"""Shared prompt prefix reuse (BatchDecodeEngine.set_prefix): the row fan-out kernel (dec_kv_rows_fanout in
csrc/hip/decoder_batch.hip) in both directions and its refusals, and the engine against an engine that was
never given a prefix -- first tokens, cache rows and teacher-forced logits bit for bit, the pass and row
counters, later hits, a prefix change, and a donor released before it reached the end of the prefix."""
import functools

import pytest

pytestmark = pytest.mark.gpu

CHUNK, R = 64, 128
P = [256] + [97 + (7 * i + i // 5) % 26 for i in range(129)]  # 130 tokens: 128 are reused with chunk 64
SEEDS = [21, 22, 23, 24]


def _tail(k, n):
    return [65 + (k * 5 + 3 * i) % 26 for i in range(n)]


X0, X1, X2 = P + _tail(0, 5), P + _tail(1, 70), P[:128] + _tail(2, 3)
X3 = P[:100] + [P[100] + 1] + _tail(3, 49)  # leaves the prefix at position 100: not carrying
WAVE = [X0, X1, X2, X3]
assert [len(x) for x in WAVE] == [135, 200, 131, 150] and X3[100] != P[100]


@functools.lru_cache(maxsize=None)
def _model(quant):
    from libsplinter_amd.models.decoder import CausalLM, DecoderConfig
    return CausalLM.random(DecoderConfig(layers=2, kv_heads=2), seed=4, device="cuda", quant=quant)


def _engine(quant, prefix=None, use_graph=False):
    from libsplinter_amd.models.decoder import BatchDecodeEngine
    eng = BatchDecodeEngine(_model(quant), max_seqs=6, use_graph=use_graph)
    if prefix is not None:
        assert eng.set_prefix(prefix, CHUNK) == len(prefix) // CHUNK * CHUNK
    return eng


def _run(eng, prompts, seeds):
    """submit together, prefill until nothing is pending: (slots, {slot: (pass number, first token)})"""
    slots = [eng.submit(ids, seed=sd) for ids, sd in zip(prompts, seeds)]
    firsts, passes = {}, 0
    while eng.pending():
        passes += 1
        for slot, t in eng.prefill(CHUNK).items():
            firsts[slot] = (passes, t)
        assert passes < 50
    return slots, firsts


def _same(a, b, pairs, lens, steps=3):
    """engines a and b: slot sa of a against slot sb of b for (sa, sb) in pairs -- cache rows [0, len) now, then
    the logits of `steps` teacher-forced steps, all bit for bit.  Both engines must have the same live slots."""
    import torch
    for (sa, sb), n in zip(pairs, lens):
        assert torch.equal(a.kv[sa, :, :, :n], b.kv[sb, :, :, :n]), (sa, sb)
    for i in range(steps):
        for k, (sa, sb) in enumerate(pairs):
            a.set_token(sa, 70 + i + 3 * k)
            b.set_token(sb, 70 + i + 3 * k)
        a.step()
        b.step()
        for sa, sb in pairs:
            assert torch.equal(a.logits[sa], b.logits[sb]), (i, sa, sb)


def _fanout(L, src, src_plane, src_rows, dst, dst_plane, seq_stride, slots, nslots, n_ctx, planes, rows, kvd,
            ndst=None):
    import numpy as np
    tb = np.ascontiguousarray(np.array(slots if slots else [0], dtype=np.int32))
    return L.dec_kv_rows_fanout(src.data_ptr(), src_plane, src_rows, dst.data_ptr(), dst_plane, seq_stride,
                                tb.ctypes.data, len(slots) if ndst is None else ndst, nslots, n_ctx, planes, rows, kvd,
                                None)


def test_kv_rows_fanout_copies_exactly_the_named_rows():
    """planes 4, n_ctx 256, kvd 128, 6 slots: rows [0, rows) of a [4, 200, 128] source land in slots 4, 1, 5 and
    nowhere else, the source stays as it was; the reverse direction (a slot -> the compact buffer, one
    destination) the same way; every refusal returns non-zero and leaves both buffers bit-identical."""
    import torch
    L = _model("bf16").L
    planes, n_ctx, kvd, nslots, cap = 4, 256, 128, 6, 200
    g = torch.Generator(device="cuda").manual_seed(71)
    src = torch.randn((planes, cap, kvd), device="cuda", generator=g).to(torch.bfloat16)
    src0 = src.clone()
    dests = [4, 1, 5]
    for rows in (1, 64, 200):
        dst = torch.full((nslots, planes, n_ctx, kvd), 7.0, device="cuda", dtype=torch.bfloat16)
        assert _fanout(L, src, cap * kvd, cap, dst, n_ctx * kvd, dst.stride(0), dests, nslots, n_ctx, planes, rows,
                       kvd) == 0
        torch.cuda.synchronize()
        want = torch.full_like(dst, 7.0)
        for b in dests:
            want[b, :, :rows] = src0[:, :rows]
        assert torch.equal(dst, want), rows
        assert torch.equal(src, src0)
        # the reverse: slot 1's rows into a compact buffer
        buf = torch.full((planes, cap, kvd), 7.0, device="cuda", dtype=torch.bfloat16)
        assert _fanout(L, dst[1], n_ctx * kvd, n_ctx, buf, cap * kvd, 0, [0], 1, cap, planes, rows, kvd) == 0
        torch.cuda.synchronize()
        wantb = torch.full_like(buf, 7.0)
        wantb[:, :rows] = src0[:, :rows]
        assert torch.equal(buf, wantb), rows
        assert torch.equal(dst, want)
    dst = torch.full((nslots, planes, n_ctx, kvd), 7.0, device="cuda", dtype=torch.bfloat16)
    buf = torch.full((planes, cap, kvd), 5.0, device="cuda", dtype=torch.bfloat16)
    clean_d, clean_b = dst.clone(), buf.clone()
    fwd = lambda slots, rows=8, kvd_=kvd, planes_=planes, ndst=None, ns=nslots: _fanout(  # noqa: E731
        L, src, cap * kvd, cap, dst, n_ctx * kvd, dst.stride(0), slots, ns, n_ctx, planes_, rows, kvd_, ndst)
    bad = {"no destination": fwd([], ndst=0),
           "17 destinations": fwd(list(range(17)), ns=32),
           "slot >= nslots": fwd([4, nslots]),
           "negative slot": fwd([-1]),
           "duplicate slot": fwd([4, 1, 4]),
           "rows 0": fwd(dests, rows=0),
           "rows -3": fwd(dests, rows=-3),
           "rows past the source": fwd(dests, rows=cap + 1),
           "rows past n_ctx": _fanout(L, dst[1], n_ctx * kvd, n_ctx, buf, cap * kvd, 0, [0], 1, cap, planes, cap + 1,
                                      kvd),
           "kvd % 8": fwd(dests, kvd_=124),
           "planes 0": fwd(dests, planes_=0)}
    torch.cuda.synchronize()
    for what, rc in bad.items():
        assert rc != 0, what
    assert torch.equal(dst, clean_d) and torch.equal(buf, clean_b) and torch.equal(src, src0)


def _prefix_wave(quant):
    """The four requests on an engine with the prefix and on one without: (eng, plain, slots)."""
    eng, plain = _engine(quant, P), _engine(quant)
    slots, firsts = _run(eng, WAVE, SEEDS)
    assert slots == [0, 1, 2, 3]
    assert eng.prefill_passes == 4 and [firsts[b][0] for b in slots] == [3, 4, 3, 3]
    assert eng.prefix_hits == 2 and eng.prefix_rows_reused == 256
    assert eng.prefill_rows == 135 + 72 + 3 + 150
    pslots, pfirsts = _run(plain, WAVE, SEEDS)
    assert pslots == slots and plain.prefill_passes == 4
    assert plain.prefill_rows == 135 + 200 + 131 + 150
    assert plain.prefix_hits == 0 and plain.prefix_rows_reused == 0
    assert [firsts[b][1] for b in slots] == [pfirsts[b][1] for b in slots]
    return eng, plain, slots


@pytest.mark.parametrize("quant", ["bf16", "q4"])
def test_engine_with_prefix_equals_engine_without(quant):
    """X0 = P + 5, X1 = P + 70, X2 = P[:128] + 3 and X3 (150 tokens, off the prefix at position 100) submitted
    together, chunk 64, prefix P of 130 tokens (128 reused): X0 is the donor, X1 and X2 wait two passes and start
    at row 128 from copied rows, X3 is untouched.  4 passes, first tokens in passes 3, 4, 3, 3, 360 packed rows
    instead of 616; first tokens, cache rows and three teacher-forced steps' logits equal the plain engine's."""
    eng, plain, slots = _prefix_wave(quant)
    _same(eng, plain, [(b, b) for b in slots], [len(x) for x in WAVE])


def test_later_hits_and_housekeeping():
    """After the wave: a request admitted much later is a hit in its first pass; graphs are not recaptured; the
    prefix cannot change under pending requests or run with another chunk; a new prefix needs a new donor;
    turning the prefix off stops the hits; a prompt that is the prefix and nothing more is served plainly."""
    eng, plain, _ = _prefix_wave("bf16")
    late = P + _tail(4, 9)
    for e in (eng, plain):
        e.release(0)
        assert e.admit([256] + _tail(5, 40), seed=3)[0] == 0  # the eager path, into the donor's old slot
    rows0 = eng.prefill_rows
    slot = eng.submit(late, seed=31)
    got = eng.prefill(CHUNK)  # restored and finished in its first pass: no hold
    assert sorted(got) == [slot] and eng.prefix_hits == 3 and eng.prefix_rows_reused == 384
    assert eng.prefill_rows - rows0 == 11
    pslots, pfirsts = _run(plain, [late], [31])
    assert pslots == [slot] and pfirsts[slot] == (3, got[slot])
    live = [0, 1, 2, 3, slot]
    _same(eng, plain, [(b, b) for b in live], [41, 200, 131, 150, len(late)], steps=2)
    # the prefix is pinned while a request is pending, and to its chunk
    for b in (1, 2, 3):
        eng.release(b)
    s1 = eng.submit(P + _tail(6, 2), seed=1)
    with pytest.raises(RuntimeError):
        eng.set_prefix(P, CHUNK)
    with pytest.raises(RuntimeError):
        eng.set_prefix(None, 0)
    with pytest.raises(ValueError):
        eng.prefill(32)
    assert sorted(eng.prefill(CHUNK)) == [s1] and eng.prefix_hits == 4
    with pytest.raises(ValueError):
        eng.prefill(32)  # nothing pending: still the wrong chunk for this prefix
    eng.release(s1)
    # a prompt that is exactly the reused rows has no token of its own: not carrying, two plain passes
    rows0, passes0 = eng.prefill_rows, eng.prefill_passes
    s2, f2 = _run(eng, [P[:128]], [2])
    assert f2[s2[0]][0] == 2 and eng.prefix_hits == 4
    assert eng.prefill_rows - rows0 == 128 and eng.prefill_passes - passes0 == 2
    eng.release(s2[0])
    # a new prefix (the same ids) drops the captured rows: the next carrying request is a donor again
    assert eng.set_prefix(P, CHUNK) == R
    s3, f3 = _run(eng, [late], [31])
    assert f3[s3[0]] == (3, got[slot]) and eng.prefix_hits == 4
    s4, f4 = _run(eng, [late], [31])  # and the one after it is a hit again
    assert f4[s4[0]] == (1, got[slot]) and eng.prefix_hits == 5
    eng.release(s3[0])
    eng.release(s4[0])
    # off: no hits, any chunk
    assert eng.set_prefix(None, 0) == 0
    rows0 = eng.prefill_rows
    s5, f5 = _run(eng, [late], [31])
    assert f5[s5[0]] == (3, got[slot]) and eng.prefix_hits == 5 and eng.prefix_rows_reused == 5 * R
    assert eng.prefill_rows - rows0 == len(late)
    eng.release(s5[0])
    s6 = eng.submit(late, seed=31)
    assert eng.prefill(32) == {} and eng.pending() == [s6]
    eng.release(s6)
    assert eng.set_prefix(P[:40], CHUNK) == 0  # shorter than a chunk: legal and inert
    s7, f7 = _run(eng, [late], [31])
    assert f7[s7[0]] == (3, got[slot]) and eng.prefix_hits == 5


def test_hits_do_not_recapture_the_step_graph():
    eng = _engine("bf16", P, use_graph=True)
    (a,), _ = _run(eng, [X0], SEEDS[:1])
    assert sorted(eng.step()) == [a]
    graphs = len(eng.graphs)
    assert graphs == 1
    (b,), fb = _run(eng, [X2], SEEDS[2:3])
    assert fb[b][0] == 1 and eng.prefix_hits == 1
    assert sorted(eng.step()) == [a, b] and len(eng.graphs) == graphs


def test_donor_released_before_it_reaches_the_end_of_the_prefix():
    """X0 and X1 submitted, one pass (X0 at 64, X1 held at 0), X0 released: X1 takes over as the donor from its
    own offset 0 and ends bit-identical to X1 on a plain engine; X2 after it is a hit."""
    eng, plain = _engine("bf16", P), _engine("bf16")
    a, b = eng.submit(X0, seed=SEEDS[0]), eng.submit(X1, seed=SEEDS[1])
    assert eng.prefill(CHUNK) == {} and eng.prefill_rows == 64
    eng.release(a)
    firsts, passes = {}, 1
    while eng.pending():
        passes += 1
        firsts.update(eng.prefill(CHUNK))
    assert passes == 5 and sorted(firsts) == [b] and eng.prefix_hits == 0
    assert eng.prefill_rows == 64 + 200
    (pb,), pf = _run(plain, [X1], SEEDS[1:2])
    assert pf[pb] == (4, firsts[b])
    (c,), fc = _run(eng, [X2], SEEDS[2:3])
    assert fc[c][0] == 1 and eng.prefix_hits == 1 and eng.prefix_rows_reused == R
    (pc,), pfc = _run(plain, [X2], SEEDS[2:3])
    assert pfc[pc] == (3, fc[c][1])
    _same(eng, plain, [(b, pb), (c, pc)], [len(X1), len(X2)])
