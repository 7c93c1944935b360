"""The decoder attention harness (tests/decoder_attn_ref.py) on the CPU, without a kernel.

First the gate: every case the two GPU files run is built here and `check` is fed its emulation, so the
chosen inputs keep a correct kernel's roundings inside EMU_BOUND and every one-hot answer is exactly
code(target).  Then the mutants: the fp64 reference with one mistake of the kind a kernel makes (a dropped
last key, tail chunk or split, a key past the length, a causal mask off by one either way, a neighbour's KV
head, two heads swapped, V rows shifted), rounded to bf16 as a kernel would, must be REJECTED by `check` or
the one-hot equality -- on the one-hot case and on at least one float case of the same shape and length.
Each rejection prints one MUTANT line with the check that fired."""
import pytest
import torch

import decoder_attn_ref as R

DEV = "cpu"


def _gate(cases):
    worst = 0.0
    for c in cases:
        worst = max(worst, c.check(c.emu)[1])
    assert worst <= R.EMU_BOUND
    return worst


@pytest.mark.parametrize("hd,g", R.GROUPED + R.WALKING)
def test_emulation_short_caches(hd, g):
    _gate(R.short_cases(hd, g, DEV))


@pytest.mark.parametrize("hd,g", R.GROUPED + R.WALKING)
def test_emulation_split_lengths(hd, g):
    _gate(R.split_cases(hd, g, DEV))


def test_emulation_device_length_wide_and_batched():
    for hd, g in R.GROUPED + R.WALKING:
        _gate(c for c, _ in R.devlen_cases(hd, g, DEV))
    _gate(R.wide_cases(DEV))
    for hd, H, KVH in R.BATCH_SHAPES:
        for span in R.BATCH_SPANS:
            _gate(R.batch_case(fill, hd, H, KVH, span, DEV) for fill in ("gauss", "onehot"))


@pytest.mark.parametrize("hd,H,KVH", R.PREFILL_SHAPES)
def test_emulation_prefill(hd, H, KVH):
    worst = _gate(R.prefill_case(fill, hd, H, KVH, n, pos0, DEV)
                  for n, pos0 in R.PREFILL_NP for fill in R.PREFILL_FILLS)
    print(f"prefill emulation hd={hd} H={H} worst={worst:.3e}")
    for n, pos0 in R.PREFILL_RAMP_NP:
        for ramp, step in R.PREFILL_RAMPS.items():
            c = R.prefill_ramp_case(ramp, hd, H, KVH, n, pos0, DEV)
            d = R.tile_steps(c)
            lo, hi = {"under8": (7.0, 8.0), "over8": (8.0, 9.0), "falling": (-8.0, -7.0)}[ramp]
            assert lo < d.min().item() and d.max().item() < hi, (ramp, d.min().item(), d.max().item())
            _gate([c])


def test_emulation_prefill_remap_and_segments():
    R.remap_coverage()
    for heads, nqb in R.REMAP_TABLE:
        _gate(R.prefill_case(fill, 64, heads, heads, 128 * nqb - 28, 5, DEV) for fill in ("gauss", "onehot_self"))
    for hd, H, KVH in R.PREFILL_SHAPES:
        for _, n, pos0, slot in R.SEGS:
            _gate([R.prefill_case("gauss", hd, H, KVH, n, pos0, DEV, seed=slot),
                   R.prefill_case("onehot_self", hd, H, KVH, n, pos0, DEV, offset=R.SLOT_CODE_STEP * slot)])


def test_geometry_of_the_listed_lengths():
    """What the case list claims about the split geometry, from the formula alone."""
    assert any(a >= 8193 for a, _ in R.split_ranges(8193)), "8193 keys: no split starts past the length"
    assert len(R.split_ranges(8193)) == 32 and R.split_ranges(8193)[1][0] == 320
    for L in R.SPLIT_LENS:
        chunk = R.split_ranges(L)[1][0]
        assert (chunk <= R.K_SMALL_L) == (L <= 16384), (L, chunk)      # the grouped splits end at 16384 keys
    assert all(b <= a for a, b in R.split_ranges(1, 20000)[1:])        # a device-side length of 1: 31 empty splits
    assert max(R.BATCH_SPANS) > 16384


# ------------------------------------------------------------------ mutants --
def _rejected(case, got, mutant):
    """`check` must refuse `got`; prints which check fired."""
    with pytest.raises(AssertionError) as e:
        case.check(got.bfloat16().double() if torch.isfinite(got).all() else got, f"{case.name}<{mutant}>")
    msg = str(e.value)
    by = "finite" if "not finite" in msg else "bound" if "relative error" in msg else "equality" \
        if "differs from code" in msg else None
    assert by, msg
    print(f"MUTANT case={case.name} mutant={mutant} rejected_by={by} :: {msg.split(': ', 1)[1][:110]}")
    return by


def _decode_mutants(c):
    """name -> the mutant's output [launches, 1, H, hd] for a single-slot decode case (None: not defined)."""
    K, V, L = c.slots[0]
    q, sc = c.q[:, 0], c.scale
    ref = lambda K_, V_, L_: R.reference(q, K_, V_, sc, lens=L_)[:, None]  # noqa: E731
    out = {"last key dropped": ref(K, V, L - 1) if L > 1 else None}
    tail = (L - 1) // 64 * 64
    out["last 64-key chunk dropped"] = ref(K, V, tail) if tail else None
    live = [(a, b) for a, b in R.split_ranges(L) if b > a]
    if len(live) >= 3:
        a, b = live[len(live) // 2]
        keep = torch.cat([torch.arange(a), torch.arange(b, L)])
        out["interior split dropped"] = ref(K[keep], V[keep], L - (b - a))
    # the row past the length holds NaN, as the GPU tests leave it: that sentinel is what rejects this mutant (a
    # live row there, the rising ramp's next key, moves the output by 4.5e-3 to 2.3e-1, not always past the bound)
    nan_row = torch.full_like(K[:1], float("nan"))
    out["extra key admitted"] = ref(torch.cat([K[:L], nan_row]), torch.cat([V[:L], nan_row]), L + 1)
    if c.KVH > 1:
        out["neighbour KV head"] = ref(K.roll(1, 1), V.roll(1, 1), L)
    swapped = c.ref.clone()
    swapped[:, :, [0, -1]] = c.ref[:, :, [-1, 0]]          # the first and the last head: different KV heads
    out["two heads swapped"] = swapped
    out["V rows shifted"] = ref(K, V[:L].roll(-1, 0), L) if L > 1 else None
    return {k: v for k, v in out.items() if v is not None}


# (hd, group, length): a short cache, all-key and edge-probe split lengths, the walking split kernel
DECODE_MUTANT_AT = [(128, 4, 257), (64, 1, 512), (128, 4, 1025), (128, 4, 4097), (256, 2, 8193), (64, 8, 20000),
                    (192, 2, 16385), (128, 3, 8193)]


@pytest.mark.parametrize("hd,g,L", DECODE_MUTANT_AT)
def test_decode_mutants_are_rejected(hd, g, L):
    if L <= R.K_SMALL_L:
        H, KVH = R.short_shape(hd, g)
        onehot = R.onehot_case(hd, H, KVH, L, None, DEV)
        floats = [R.float_case("gauss", hd, H, KVH, L, DEV, rows=R.K_SMALL_L)]
    else:
        onehot = R.split_onehot_case(hd, g, L, DEV)
        floats = [R.float_case(f, hd, *R.long_shape(g), L, DEV) for f in R.SPLIT_FILLS]
    for c in [onehot] + floats:
        c.check(c.emu)
    muts = {c.name: _decode_mutants(c) for c in [onehot] + floats}
    names = list(muts[onehot.name])
    if L > R.K_SMALL_L:
        assert {"last key dropped", "extra key admitted", "interior split dropped"} <= set(names)
    for m in names:
        _rejected(onehot, muts[onehot.name][m], m)
        caught = []
        for c in floats:
            got = muts[c.name][m]
            try:
                c.check(got.bfloat16().double() if torch.isfinite(got).all() else got, f"{c.name}<{m}>")
            except AssertionError as e:
                caught.append(c.name)
                print(f"MUTANT case={c.name} mutant={m} rejected :: {str(e).split(': ', 1)[1][:110]}")
        assert caught, f"no float case at hd {hd} group {g} L {L} rejects '{m}'"


@pytest.mark.parametrize("hd,H,KVH,n,pos0", [(128, 8, 2, 33, 990), (64, 8, 2, 130, 126), (64, 2, 2, 257, 511),
                                             (128, 2, 2, 17, 15)])
def test_prefill_mutants_are_rejected(hd, H, KVH, n, pos0):
    cases = {f: R.prefill_case(f, hd, H, KVH, n, pos0, DEV) for f in R.PREFILL_FILLS}
    for c in cases.values():
        c.check(c.emu)
    # the same fills one row longer: their last cache row is what a live cache holds at row pos0 + n
    longer = {f: R.prefill_case(f, hd, H, KVH, n + 1, pos0, DEV) for f in R.PREFILL_FILLS}

    def mutants(f):
        c, lg = cases[f], longer[f]
        assert torch.equal(lg.K[:-1], c.K) and torch.equal(lg.V[:-1], c.V)
        ref = lambda K_, V_, hz=0: R.reference(c.q, K_, V_, c.scale, pos0=pos0, horizon=hz)  # noqa: E731
        swapped = c.ref.clone()
        swapped[:, [0, -1]] = c.ref[:, [-1, 0]]            # the first and the last head: different KV heads
        return {"diagonal excluded": ref(c.K, c.V, -1),
                "key p+1 admitted": ref(lg.K, lg.V, 1),
                "neighbour KV head": ref(c.K.roll(1, 1), c.V.roll(1, 1)),
                "two heads swapped": swapped,
                "V rows shifted": ref(c.K, c.V.roll(-1, 0))}

    muts = {f: mutants(f) for f in cases}
    for m in muts["gauss"]:
        by = {}
        for f, c in cases.items():
            got = muts[f][m]
            try:
                c.check(got.bfloat16().double() if torch.isfinite(got).all() else got, f"{c.name}<{m}>")
            except AssertionError as e:
                by[f] = str(e)
                print(f"MUTANT case={c.name} mutant={m} rejected :: {str(e).split(': ', 1)[1][:110]}")
        assert any(f.startswith("onehot") for f in by), f"no one-hot case rejects '{m}'"
        assert any(f in by for f in ("gauss", "peaked")), f"neither gauss nor peaked rejects '{m}'"
    # the mask mutants row by row: every row but those without the key in question is wrong on its own
    c = cases["onehot_self"]
    got = R.reference(c.q, c.K, c.V, c.scale, pos0=pos0, horizon=-1).bfloat16().double()
    wrong = (got != c.want.double()).any(-1).all(-1)
    assert wrong.all(), "diagonal excluded: a row still answers code(p)"
    c = cases["onehot_next"]
    got = R.reference(c.q, c.K, c.V, c.scale, pos0=pos0, horizon=1)[:-1].bfloat16().double()
    err = R._row_err(got, c.ref[:-1])
    assert (err > R.BOUND).all(), "key p+1 admitted: a (row, head) stays inside the bound"
