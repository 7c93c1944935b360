"""The decoder attention kernels against fp64, head by head: the harness shared by
tests/test_decoder_attn_ref_cpu.py (the harness on its own mutants), tests/test_decoder_attention_gpu.py
(decode, single and batched) and tests/test_decoder_prefill_attention_gpu.py.

`reference` is fp64 softmax(q K^T * scale) V from the same bf16 inputs, one KV head at a time with the
grouped-query map written out (`heads_of`); `emulate` is the arithmetic of a correct kernel (decode: fp32
throughout, so the fp64 result rounded to bf16; prefill: fp32 scores, P rounded to bf16 for P V, l summed
from the unrounded P, bf16 output); `check` holds the relative L2 error of every single (row, head) against
BOUND after showing that the emulation stays inside EMU_BOUND on the same inputs.  Both figures are the
per-row ones of tests/test_encoder_attention_gpu.py.

Inputs are deterministic: the float fills come from seeded CPU generators (the same numbers here and on
the GPU), the one-hot fill is integer arithmetic.  A case never changes after it is built.

No GPU is touched at import; every builder takes the device."""
import functools
import math

import torch

BOUND = 1e-2        # per (row, head), kernel vs fp64
EMU_BOUND = 5e-3    # per (row, head), the emulated roundings vs fp64
LOG2E = 1.4426950408889634

# the kernels' own strides (csrc/hip/decoder_common.hpp, decoder_body_attn_g.hpp, k_prefill_attn)
K_SMALL_L = 512
MAX_SPLITS = 32
# one-hot: KV head kvh holds K[j] = code(j + 101 kvh) and V[j] = code(j + 202 kvh) (KV head 0: K = V = code(j)),
# so a neighbour KV head's rows answer a query with another code
K_CODE_STEP, V_CODE_STEP = 101, 202
SLOT_CODE_STEP = 1000


# ----------------------------------------------------------------- geometry --
def heads_of(H, KVH):
    """heads_of[kvh] = the query heads h with h // (H // KVH) == kvh."""
    assert H % KVH == 0
    grp = H // KVH
    return [[h for h in range(H) if h // grp == kvh] for kvh in range(KVH)]


def decode_splits(L):
    """Splits of a launch sized for L keys: one up to 512, then one per 256 keys, at most 32."""
    return 1 if L <= K_SMALL_L else min(MAX_SPLITS, (L + 255) // 256)


def split_ranges(L, sized_for=None):
    """[(k0, k1)] of the S splits of a cache of L keys in a launch sized for `sized_for` (the capacity or
    span; L itself for a host-side length): chunk = roundup64(ceil(L / S)); k1 <= k0 for an empty split."""
    S = decode_splits(L if sized_for is None else sized_for)
    chunk = ((L + S - 1) // S + 63) // 64 * 64
    return [(j * chunk, min(L, (j + 1) * chunk)) for j in range(S)]


def edge_probes(L, sized_for=None):
    """The keys a one-hot sweep of a long cache probes: 0, L-1, the first and last two keys of every
    split, and both sides of every 64-key boundary inside the first and the last non-empty split."""
    live = [(a, b) for a, b in split_ranges(L, sized_for) if b > a]
    keys = {0, L - 1}
    for a, b in live:
        keys.update((a, a + 1, b - 2, b - 1))
    for a, b in (live[0], live[-1]):
        for m in range((a // 64 + 1) * 64, b, 64):
            keys.update((m - 1, m))
    return sorted(k for k in keys if 0 <= k < L)


def probe_launches(keys, H):
    """The probe keys as target rows [launches, H], the last launch padded by wrapping round."""
    n = -(-len(keys) // H)
    return torch.tensor([keys[i % len(keys)] for i in range(n * H)], dtype=torch.int64).reshape(n, H)


def code(j, hd):
    """code(j): the 16 low bits of j as -1 / +1, each repeated hd / 16 times -> float [..., hd]."""
    bits = (j[..., None] >> torch.arange(16, device=j.device)) & 1
    return (bits * 2 - 1).float().repeat_interleave(hd // 16, -1)


# ---------------------------------------------------------------- reference --
def _decode(q, K, V, L, scale):
    """q [B, H, hd] over the first L rows of one cache K / V [rows, KVH, hd] -> fp64 [B, H, hd]."""
    B, H, hd = q.shape
    out = torch.empty(B, H, hd, dtype=torch.float64, device=q.device)
    for kvh, hs in enumerate(heads_of(H, K.shape[1])):
        k, v = K[:L, kvh].double(), V[:L, kvh].double()
        s = (q[:, hs].double().reshape(-1, hd) @ k.T) * scale
        out[:, hs] = (s.softmax(-1) @ v).reshape(B, len(hs), hd)
    return out


def _prefill(q, K, V, pos0, scale, emu, horizon):
    n, H, hd = q.shape
    Lk = min(pos0 + n + max(horizon, 0), K.shape[0])
    qpos = torch.arange(pos0, pos0 + n, device=q.device)[:, None] + horizon
    hidden = torch.arange(Lk, device=q.device)[None, :] > qpos                      # [n, Lk]
    out = torch.empty(n, H, hd, dtype=torch.float64, device=q.device)
    for kvh, hs in enumerate(heads_of(H, K.shape[1])):
        k, v = K[:Lk, kvh].double(), V[:Lk, kvh].double()
        s = torch.einsum("qhd,kd->hqk", q[:, hs].double(), k)                          # q . k, unscaled
        if not emu:
            p = (s * scale).masked_fill(hidden, float("-inf")).softmax(-1)
            out[:, hs] = torch.einsum("hqk,kd->qhd", p, v)
        else:
            s32 = s.float().masked_fill(hidden, float("-inf"))
            p = torch.exp2((s32 - s32.amax(-1, keepdim=True)) * (scale * LOG2E))    # fp32
            l = p.sum(-1)                                                           # [h, q], from the unrounded p
            o = torch.einsum("hqk,kd->qhd", p.bfloat16().double(), v).float()
            out[:, hs] = (o / l.T[..., None]).bfloat16().double()
    return out


def reference(q, K, V, scale, lens=None, pos0=None, horizon=0):
    """fp64 softmax(q K^T * scale) V from bf16 inputs.
    Decode (lens): q [B, H, hd] over the first `lens` rows of K / V [rows, KVH, hd] -> [B, H, hd].
    Prefill (pos0): q [n, H, hd], row r at absolute position pos0 + r, sees keys 0 .. pos0 + r -> [n, H, hd].
    horizon moves the causal edge (a row sees keys 0 .. p + horizon); only the CPU test's mutants pass it."""
    assert (lens is None) != (pos0 is None)
    if lens is not None:
        return _decode(q, K, V, int(lens), scale)
    return _prefill(q, K, V, int(pos0), scale, False, horizon)


def emulate(q, K, V, scale, lens=None, pos0=None):
    """The roundings of a correct kernel, as fp64 values (see the module docstring)."""
    assert (lens is None) != (pos0 is None)
    if lens is not None:
        return _decode(q, K, V, int(lens), scale).bfloat16().double()
    return _prefill(q, K, V, int(pos0), scale, True, 0)


# -------------------------------------------------------------------- check --
def _row_err(x, ref):
    e = (x - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)
    return torch.nan_to_num(e, nan=float("inf"), posinf=float("inf"))


def _at(mask_or_err, lens, first, dims=None):
    """(value, 'launch i slot b head h length L') of the first True / the largest entry of a [..., H] tensor."""
    flat = mask_or_err.flatten()
    i = int(flat.nonzero()[0]) if first else int(flat.argmax())
    idx = []
    rem = i
    for d in reversed(mask_or_err.shape):
        idx.append(rem % d)
        rem //= d
    idx.reverse()
    lead, head = tuple(idx[:-1]), idx[-1]
    ln = ""
    if lens is not None:
        ln = f" length {int(torch.as_tensor(lens).expand(mask_or_err.shape[:-1])[lead])}"
    dims = dims or ("launch", "slot") if len(lead) == 2 else ("row",)
    where = " ".join(f"{d} {i}" for d, i in zip(dims, lead))
    return flat[i].item(), f"{where} head {head}{ln}"


def check(got, ref, emu, name, lens=None):
    """got, ref, emu: fp64 [launches, slots, H, hd] (decode: one query row a launch) or [rows, H, hd] (prefill); lens:
    the key count behind every leading index (broadcastable), for the message.  Asserts, in this order:
    the emulation within EMU_BOUND, every output finite, the kernel within BOUND; each per (row, head).
    Prints one DECATTN line and returns (kernel error, emulation error)."""
    e_emu, at = _at(_row_err(emu, ref), lens, False)
    assert e_emu <= EMU_BOUND, f"{name}: the inputs are ill-conditioned, emulation {e_emu:.3e} > {EMU_BOUND} at {at}"
    bad = ~torch.isfinite(got).all(-1)
    if bad.any():
        _, at = _at(bad, lens, True)
        raise AssertionError(f"{name}: not finite: {int(bad.sum())} (row, head) outputs unwritten, NaN or inf, "
                             f"first at {at}")
    e_k, at = _at(_row_err(got, ref), lens, False)
    print(f"DECATTN case={name} kernel={e_k:.3e} emulation={e_emu:.3e} worst {at}")
    assert e_k <= BOUND, f"{name}: relative error {e_k:.3e} > {BOUND} at {at}; emulation {e_emu:.3e}"
    return e_k, e_emu


def check_exact(got, want, name, lens=None):
    """The one-hot equality: every output element is the +-1 of code(target), bit for bit."""
    bad = (got != want.double()).any(-1)
    if bad.any():
        _, at = _at(bad, lens, True)
        raise AssertionError(f"{name}: differs from code(target) in {int(bad.sum())} (row, head) outputs, "
                             f"first at {at}")


# ------------------------------------------------------------- decode cases --
BASE_ROWS = 23600   # 20000 keys and six slot offsets of 600 rows


@functools.lru_cache(maxsize=None)
def _base(hd, KVH, rows, seed, dev):
    """Gaussian K, V [rows, KVH, hd] (bf16) and one unit vector per KV head, shared by every case of a shape."""
    g = torch.Generator().manual_seed(seed)
    K = torch.randn(rows, KVH, hd, generator=g).bfloat16()
    V = torch.randn(rows, KVH, hd, generator=g).bfloat16()
    u = torch.randn(KVH, hd, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    return K.to(dev), V.to(dev), u.to(dev)


@functools.lru_cache(maxsize=None)
def _ramp_keys(hd, KVH, rows, seed, sign, dev):
    """K[j] = noise + sign * (j / 64) * 2 * u: against q = 2 sqrt(hd) u the score moves by 4 nats per 64 keys."""
    K, _, u = _base(hd, KVH, rows, seed, dev)
    j = torch.arange(rows, device=dev, dtype=torch.float32)[:, None, None]
    return (K.float() + sign * (j / 64) * 2 * u[None]).bfloat16()


class DecodeCase:
    """q [launches, slots, H, hd] over one cache per slot (slots[b] = (K, V, L), rows [:L] of K / V
    [>= L, KVH, hd] valid; None: an inactive slot), with the fp64 reference and the emulation of every
    launch.  want: code(target) of a one-hot case, else None."""

    def __init__(self, name, q, slots, want=None):
        self.name, self.q, self.slots, self.want = name, q, slots, want
        self.nl, self.ns, self.H, self.hd = q.shape
        self.KVH = next(s for s in slots if s is not None)[0].shape[1]
        self.scale = self.hd ** -0.5
        self.ref = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
        for b, s in enumerate(slots):
            if s is not None:
                self.ref[:, b] = reference(q[:, b], s[0], s[1], self.scale, lens=s[2])
        self.emu = self.ref.bfloat16().double()
        self.live = [b for b, s in enumerate(slots) if s is not None]
        self.lens = torch.tensor([s[2] if s is not None else 0 for s in slots])[None, :].expand(self.nl, self.ns)

    def check(self, got, name=None):
        """got: fp64 [launches, slots, H, hd]; only the live slots are compared."""
        lv = self.live
        r = check(got[:, lv], self.ref[:, lv], self.emu[:, lv], name or self.name, self.lens[:, lv])
        if self.want is not None:
            check_exact(got[:, lv], self.want[:, lv], name or self.name, self.lens[:, lv])
        return r


def _q_rows(shape, seed, dev):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def float_slot(fill, hd, H, KVH, L, dev, rows=BASE_ROWS, seed=0, row0=0):
    """(q [H, hd] float, (K, V, L)) of the fill `gauss`, `peaked`, `ramp+` or `ramp-`; the cache is rows
    row0 .. row0 + L - 1 of the shape's shared base."""
    K, V, u = _base(hd, KVH, rows, 7 + hd, dev)
    assert row0 + L <= rows
    q = _q_rows((H, hd), 1000 * seed + 13 * H + hd + L, dev)
    if fill == "peaked":
        q = q * 4
    elif fill in ("ramp+", "ramp-"):
        K = _ramp_keys(hd, KVH, rows, 7 + hd, 1.0 if fill == "ramp+" else -1.0, dev)
        kv_of = torch.tensor([h // (H // KVH) for h in range(H)], device=dev)
        q = 2 * math.sqrt(hd) * u[kv_of] + 0.1 * q
    else:
        assert fill == "gauss", fill
    return q, (K[row0:row0 + L], V[row0:row0 + L], L)


def float_case(fill, hd, H, KVH, L, dev, rows=BASE_ROWS):
    q, slot = float_slot(fill, hd, H, KVH, L, dev, rows)
    return DecodeCase(f"{fill}_hd{hd}_H{H}_KVH{KVH}_L{L}", q.bfloat16()[None, None], [slot])


def onehot_slot(hd, H, KVH, L, targets, dev, vshift=0, offset=0):
    """targets int64 [launches, H] -> (q [launches, H, hd], (K, V, L), want [launches, H, hd]):
    K[j, kvh] = code(j + offset + 101 kvh), V[j, kvh] = code(j + offset + vshift + 202 kvh), query head h =
    32 code(its target's K row); the answer is its target's V row."""
    j = torch.arange(L, device=dev)[:, None] + offset
    kvh = torch.arange(KVH, device=dev)[None, :]
    K = code(j + K_CODE_STEP * kvh, hd).bfloat16()
    V = code(j + vshift + V_CODE_STEP * kvh, hd).bfloat16()
    kv_of = torch.tensor([h // (H // KVH) for h in range(H)], device=dev)[None, :]
    t = targets.to(dev) + offset
    return 32 * code(t + K_CODE_STEP * kv_of, hd), (K, V, L), code(t + vshift + V_CODE_STEP * kv_of, hd)


def onehot_case(hd, H, KVH, L, keys, dev, vshift=0):
    """One-hot case probing `keys` (every key of the cache when None), H heads per launch."""
    keys = list(range(L)) if keys is None else keys
    q, slot, want = onehot_slot(hd, H, KVH, L, probe_launches(keys, H), dev, vshift)
    c = DecodeCase(f"onehot{'_vshift' if vshift else ''}_hd{hd}_H{H}_KVH{KVH}_L{L}", q.bfloat16()[:, None], [slot],
                   want[:, None])
    c.keys = keys
    return c


# the cache lengths of the decode files
SHORT_LENS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]
SPLIT_LENS = [513, 576, 577, 769, 1025, 4097, 8192, 8193, 16384, 16385, 20000]
ALL_KEYS_UP_TO = 2048
SPLIT_FILLS = ["gauss", "peaked", "ramp+", "ramp-"]
# (hd, query-group size): the twelve grouped kernels, then the key-walking ones (head dim 192, a group of 3)
GROUPED = [(hd, g) for hd in (64, 128, 256) for g in (1, 2, 4, 8)]
WALKING = [(192, 2), (192, 4), (128, 3)]
DEV_LEN = [(1, 512), (300, 512), (512, 512), (1, 20000), (700, 20000), (8193, 20000)]   # (length, capacity)
WIDE = dict(hd=64, H=136, KVH=17, lens=[600, 1024, 1025])                               # the H > 128 arm
# batched: (hd, H, KVH) for groups 1, 4 and 3; span -> the seven slots' lengths (None: the inactive slot)
BATCH_SHAPES = [(64, 2, 2), (128, 8, 2), (192, 6, 2)]
BATCH_SPANS = {512: [1, 64, None, 65, 257, 511, 512],
               2048: [1, 513, None, 577, 1025, 700, 2048],
               16640: [1, 513, None, 4097, 8193, 16385, 16640]}


def short_shape(hd, g):
    """(H, KVH) of the short-cache sweeps: 128 heads (126 for a group of 3), so one launch probes 128 keys."""
    H = 126 if g == 3 else 128
    return H, H // g


def long_shape(g, kvh=2):
    """(H, KVH) of the long caches: 2 KV heads for the float fills, 4 for the one-hot probes."""
    return kvh * g, kvh


def short_cases(hd, g, dev):
    """Every case of the short-cache sweep of one shape: gauss and every key probed at every length, and the
    shifted-V probe at one length."""
    H, KVH = short_shape(hd, g)
    for L in SHORT_LENS:
        yield float_case("gauss", hd, H, KVH, L, dev, rows=K_SMALL_L)
        yield onehot_case(hd, H, KVH, L, None, dev)
    yield onehot_case(hd, H, KVH, 257, None, dev, vshift=1)


def split_onehot_case(hd, g, L, dev, vshift=0):
    """Every key up to 2048 keys (128 heads a launch), the edge keys of the splits beyond (4 KV heads)."""
    if L <= ALL_KEYS_UP_TO:
        return onehot_case(hd, *short_shape(hd, g), L, None, dev, vshift)
    return onehot_case(hd, *long_shape(g, 4), L, edge_probes(L), dev, vshift)


def split_cases(hd, g, dev, lens=None):
    for L in lens or SPLIT_LENS:
        for fill in SPLIT_FILLS:
            yield float_case(fill, hd, *long_shape(g), L, dev)
        yield split_onehot_case(hd, g, L, dev)
    if lens is None:
        yield split_onehot_case(hd, g, 8193, dev, vshift=1)


def devlen_cases(hd, g, dev):
    """(case, capacity): the one-hot edge probes of a cache whose length the kernels read on the device."""
    for L, cap in DEV_LEN:
        keys = list(range(L)) if L <= 64 else edge_probes(L, cap)
        if cap <= K_SMALL_L:
            keys = sorted(set(keys) | {k for m in range(64, L, 64) for k in (m - 1, m)})
        c = onehot_case(hd, *long_shape(g, 4), L, keys, dev)
        c.name += f"_cap{cap}"
        yield c, cap


def wide_cases(dev):
    for L in WIDE["lens"]:
        yield float_case("gauss", WIDE["hd"], WIDE["H"], WIDE["KVH"], L, dev, rows=1100)
        yield onehot_case(WIDE["hd"], WIDE["H"], WIDE["KVH"], L, None, dev)


def batch_case(fill, hd, H, KVH, span, dev):
    """Seven slots (one inactive) of BATCH_SPANS[span]; slot b's gaussian cache starts 600 b rows into the
    shared base, its one-hot cache carries the code offset 1000 b, its probes are its own edge keys."""
    lens = BATCH_SPANS[span]
    qs, slots, wants = [], [], []
    if fill == "gauss":
        for b, L in enumerate(lens):
            if L is None:
                qs.append(torch.zeros(1, H, hd, device=dev))
                slots.append(None)
                continue
            q, s = float_slot("gauss", hd, H, KVH, L, dev, seed=b + 1, row0=600 * b)
            qs.append(q[None])
            slots.append(s)
        return DecodeCase(f"batch_gauss_hd{hd}_H{H}_KVH{KVH}_span{span}", torch.stack(qs, 1).bfloat16(), slots)
    assert fill == "onehot"
    probes = {b: (list(range(L)) if L <= 64 else edge_probes(L, span)) for b, L in enumerate(lens) if L is not None}
    nl = max(-(-len(k) // H) for k in probes.values())
    for b, L in enumerate(lens):
        if L is None:
            qs.append(torch.zeros(nl, H, hd, device=dev))
            wants.append(torch.zeros(nl, H, hd, device=dev))
            slots.append(None)
            continue
        keys = probes[b]
        t = torch.tensor([keys[i % len(keys)] for i in range(nl * H)], dtype=torch.int64).reshape(nl, H)
        q, s, w = onehot_slot(hd, H, KVH, L, t, dev, offset=SLOT_CODE_STEP * b)
        qs.append(q)
        wants.append(w)
        slots.append(s)
    c = DecodeCase(f"batch_onehot_hd{hd}_H{H}_KVH{KVH}_span{span}", torch.stack(qs, 1).bfloat16(), slots,
                   torch.stack(wants, 1))
    c.probes = probes
    return c


# ------------------------------------------------------------ prefill cases --
PREFILL_ROWS = 1100
PREFILL_NP = [(1, 0), (1, 31), (1, 32), (1, 63), (1, 64), (16, 0), (17, 15), (33, 31), (127, 1), (128, 0), (129, 0),
              (130, 126), (257, 511), (33, 990)]
PREFILL_SHAPES = [(hd, 2 * g, 2) for hd in (64, 128) for g in (1, 4)]      # (hd, H, KVH): groups 1 and 4
PREFILL_FILLS = ["gauss", "peaked", "onehot_self", "onehot_next", "onehot_first", "onehot_tile"]
# rise of every row's maximum score per key tile in the kernel's log2 units; the rescale is deferred up to 8
PREFILL_RAMPS = {"under8": 7.5, "over8": 8.5, "falling": -7.5}
PREFILL_RAMP_NP = [(130, 126), (33, 990)]
# the XCD remap: heads x q-blocks workgroups; n = 128 nqb - 28
REMAP_NQB = [3, 6, 7]
REMAP_HEADS = [1, 2, 3, 5, 12]
REMAP_TABLE = [(h, n) for n in REMAP_NQB for h in REMAP_HEADS]
# (row0, n, pos0, slot): unequal n with 1 and 129, slots out of order, slot 1 skipped, gaps between the segments
SEGS = [(2, 1, 63, 3), (5, 129, 200, 0), (140, 33, 990, 2)]
SEG_T, SEG_SLOTS, SEG_CTX = 180, 4, 1024


def key_tile(hd):
    """Keys per tile of k_prefill_attn."""
    return 32 if hd == 128 else 64


def remap_coverage():
    """The table reaches every workgroup count modulo 8, a grid below 8, and an uneven one above 8."""
    assert {h * n % 8 for h, n in REMAP_TABLE} == set(range(8))
    assert any(h * n < 8 for h, n in REMAP_TABLE)
    assert any(h * n > 8 and h * n % 8 for h, n in REMAP_TABLE)


class PrefillCase:
    """q [n, H, hd] at positions pos0 .. pos0 + n - 1 over K / V [pos0 + n, KVH, hd]."""

    def __init__(self, name, q, K, V, pos0, want=None):
        self.name, self.q, self.K, self.V, self.pos0, self.want = name, q, K, V, pos0, want
        self.n, self.H, self.hd = q.shape
        self.KVH = K.shape[1]
        self.scale = self.hd ** -0.5
        assert K.shape[0] == pos0 + self.n
        self.ref = reference(q, K, V, self.scale, pos0=pos0)
        self.emu = emulate(q, K, V, self.scale, pos0=pos0)
        self.lens = torch.arange(pos0 + 1, pos0 + self.n + 1)

    def check(self, got, name=None):
        r = check(got, self.ref, self.emu, name or self.name, self.lens)
        if self.want is not None:
            check_exact(got, self.want, name or self.name, self.lens)
        return r


def prefill_case(fill, hd, H, KVH, n, pos0, dev, offset=0, seed=0):
    """One prompt chunk.  gauss, peaked; onehot_self (target = the row's own position: the diagonal key must
    be seen, exact), onehot_next (target p + 1: it must not be seen; no exact answer, a leak lands on
    code(p + 1)), onehot_first (key 0), onehot_tile (the first key of the row's last key tile); offset: the
    slot's code offset."""
    Lk = pos0 + n
    name = f"{fill}_hd{hd}_H{H}_KVH{KVH}_n{n}_pos{pos0}"
    if fill in ("gauss", "peaked"):
        K, V, _ = _base(hd, KVH, PREFILL_ROWS, 3 + hd + seed, dev)
        q = _q_rows((n, H, hd), 17 * n + pos0 + hd + H + seed, dev) * (4 if fill == "peaked" else 1)
        return PrefillCase(name, q.bfloat16(), K[:Lk], V[:Lk], pos0)
    p = torch.arange(pos0, Lk, dtype=torch.int64)
    KT = key_tile(hd)
    t = {"onehot_self": p, "onehot_next": p + 1, "onehot_first": p * 0, "onehot_tile": p // KT * KT}[fill]
    q, (K, V, _), want = onehot_slot(hd, H, KVH, Lk, t[:, None].expand(n, H), dev, offset=offset)
    return PrefillCase(name, q.bfloat16(), K, V, pos0, None if fill == "onehot_next" else want)


def prefill_ramp_case(ramp, hd, H, KVH, n, pos0, dev):
    """Every row's maximum score moves by PREFILL_RAMPS[ramp] log2 units from one key tile to the next."""
    step, KT, Lk = PREFILL_RAMPS[ramp], key_tile(hd), pos0 + n
    g = torch.Generator().manual_seed(29 + hd)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    u = rnd(KVH, hd)
    u = u / u.norm(dim=-1, keepdim=True)
    cq = 4.0
    dg = abs(step) / (cq * hd ** -0.5 * LOG2E)            # score = cq * g * scale nats
    tile = torch.arange(Lk, device=dev) // KT
    gk = dg * (tile if step > 0 else (Lk - 1) // KT - tile).float()
    kv_of = torch.tensor([h // (H // KVH) for h in range(H)], device=dev)
    q = 0.03 * rnd(n, H, hd) + cq * u[kv_of][None]
    K = 0.125 * rnd(Lk, KVH, hd) + gk[:, None, None] * u[None]
    V = rnd(Lk, KVH, hd)
    return PrefillCase(f"ramp_{ramp}_hd{hd}_H{H}_n{n}_pos{pos0}", q.bfloat16(), K.bfloat16(), V.bfloat16(), pos0)


def tile_steps(c):
    """Per-row steps of the maximum score between neighbouring full key tiles, log2 units, [H, n, tiles - 1]."""
    KT = key_tile(c.hd)
    full = c.K.shape[0] // KT * KT
    steps = []
    for kvh, hs in enumerate(heads_of(c.H, c.KVH)):
        s = torch.einsum("qhd,kd->hqk", c.q[:, hs].double(), c.K[:full, kvh].double()) * (c.scale * LOG2E)
        steps.append(s.reshape(len(hs), c.n, -1, KT).amax(-1).diff(dim=-1))
    return torch.cat(steps)
