"""Inputs and CPU-side expectations of tests/test_gpu_wire_limits.py: the newer wires -- the requantised byte gather
(include/ina_i8_gather.h), error feedback and stochastic rounding on the byte wire (ina_i8_ef.h, ina_i8_sr.h) and
the nibble wire (ina_i4.h) -- at every compile-time slice count and loop remainder, every ragged tail of the nibble
sums, every block width, on tests/_rot_limits.py's planted bucket, at sign keys that need the counter's high word
and in views of one receive buffer.  Everything here is numpy and the yardsticks tests/_i4_ref.py, _i8_ref.py,
_i8_ef_ref.py and _i8_sr_ref.py; the builders are cached and their results are never written to
(tests/test_wire_limits_inputs.py asserts, without a GPU, that they reach what they are meant to reach)."""
import functools

import numpy as np

from tests import _i4_ref as r4
from tests import _i8_ef_ref as r8ef
from tests import _i8_ref as r8
from tests import _i8_sr_ref as r8sr
from tests import _rot_limits as R

F32 = np.float32
SEED, NBLK = R.SEED, R.NBLK
RND = dict(step=5, sub=65, e0=16 * 1_000_003)       # the stochastic requantiser's rounding stream
SR_SEED, SR_KEY = SEED ^ 5, dict(sub=3, e0=4 * 777)  # the stochastic quantiser's; the rotation's is R.key()
SUMS = ("i8.sum", "i8.rq", "i8.rq_sr", "i4.sum", "i4.rq")
REQUANT = ("i8.rq", "i8.rq_sr", "i4.rq")
G_STATIC, G_LOOP = (4, 16), (5, 15, 31, 63)         # instances of their own; remainders 1, 8+2+2+2+1, a batch of 15
ALL_V = (8, 16, 32, 64, 128, 256)
# a block's largest |sum| -> its shift, for both byte rules (rne(A / 2^sh) <= 127 and A <= 127 << sh agree on these)
BYTE_TARGETS = {100: 0, 200: 1, 400: 2, 800: 3, 1600: 4, 3200: 5, 6400: 6, 8192: 7}
NIBBLE_TARGETS = {20: 0, 100: 0, 200: 1, 400: 2, 512: 3}     # 3 slices reach 24


def nibble(kind):
    return kind.startswith("i4")


def lim(kind):
    """(lowest, highest) value of a slice."""
    return (-8, 7) if nibble(kind) else (-128, 127)


def lane_values(kind):
    """The values one lane of the kind's kernel owns: a block of V is V / lane_values adjacent lanes."""
    return 32 if nibble(kind) else 16


def ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays if len(arrays) > 1 else arrays[0]


def spread(S, G, kind, rng):
    """[G, ...] slices that add up to S exactly: S / G each, the remainder over the first slices, and where that
    leaves room a random d added to slice 2j and taken from slice 2j + 1, so that the slices differ."""
    lo, hi = lim(kind)
    S = np.asarray(S, np.int64)
    p = S // G + (np.arange(G).reshape((G,) + (1,) * S.ndim) < S % G)
    d = rng.integers(-(hi // 6), hi // 6 + 1, (G // 2,) + S.shape)
    d = np.where(np.abs(p[0]) <= hi // 2, d, 0)            # the slices of one value differ by at most 1
    p[0:2 * (G // 2):2] += d
    p[1:2 * (G // 2):2] -= d
    assert np.array_equal(p.sum(0), S) and p.min() >= lo and p.max() <= hi
    return p


def slices_of(kind, vals):
    """The [G, n] values as the device takes them: int8 rows, or packed nibbles."""
    return ro(np.stack([r4.pack(v) for v in vals]) if nibble(kind) else np.asarray(vals).astype(np.int8))


def expect(kind, parts, V):
    """The outputs of one sum over `parts` (slices_of), from the yardsticks: (int16 sums,) or (bytes, shifts)."""
    parts = list(parts)
    out = {"i8.sum": lambda: (r8.sum_slices(parts),), "i8.rq": lambda: r8.requant(parts, V),
           "i8.rq_sr": lambda: r8sr.requant(parts, V, SEED, **RND), "i4.sum": lambda: (r4.sum_slices(parts),),
           "i4.rq": lambda: r4.requant(parts, V)}[kind]()
    for a in out:
        a.flags.writeable = False
    return tuple(out)


# ---- 1. every compile-time G and the loop's remainders ---------------------------------------------------------
G_V, G_N = 16, 5 * 16                                 # bytes: 5 whole chunks; nibbles: 2 and a ragged lane of 2 dwords


@functools.lru_cache(maxsize=None)
def g_case(kind, G, fill):
    """(slices, expected): "extreme": columns of the lowest and of the highest value in every slice (G = 63: -504 and
    +441 for nibbles, -8064 and +8001 for bytes); "random": the full range."""
    lo, hi = lim(kind)
    rng = np.random.default_rng(G * 1000 + len(kind))
    vals = (np.where(np.arange(G_N) % 2, hi, lo) + 0 * np.arange(G)[:, None] if fill == "extreme"
            else rng.integers(lo, hi + 1, (G, G_N)))
    parts = slices_of(kind, vals)
    return parts, expect(kind, parts, G_V)


# ---- 2. every ragged tail of the nibble sums -------------------------------------------------------------------
RAG_G = (3, 16, 33)
RAG_SUM_N = (16, 48, 80)                              # rag = 2: alone, after one whole chunk, after two
RAG_RQ = [(8, nblk) for nblk in range(1, 8)] + [(16, nblk) for nblk in (1, 2, 3)]


def rag_of(n):
    return n % 32 // 8


@functools.lru_cache(maxsize=None)
def rag_sum_case(G, n):
    rng = np.random.default_rng(G * 100 + n)
    vals = rng.integers(-8, 8, (G, n))
    vals[:, n - 1], vals[:, n - 8] = -8, 7            # the tail's last dword: its first and last value
    parts = slices_of("i4.sum", vals)
    return parts, expect("i4.sum", parts, 0)


@functools.lru_cache(maxsize=None)
def rag_rq_case(G, V, nblk):
    """Sums within +-2 G (shift 0 up to G = 33), a +7 G column in the block before the last and -8 G in the last:
    the largest sum, and at G = 16 and 33 a shift no other block has."""
    rng = np.random.default_rng(G * 1000 + V * 10 + nblk)
    vals = rng.integers(-2, 3, (G, nblk, V))
    if nblk > 1:
        vals[:, nblk - 2, 3] = 7
    vals[:, nblk - 1, V - 2] = -8
    parts = slices_of("i4.rq", vals.reshape(G, nblk * V))
    return parts, expect("i4.rq", parts, V)


# ---- 3. every V for the three requantisers ---------------------------------------------------------------------
V_G = (3, 64)


def max_pos(b, V):
    """Where block b holds its largest |sum|: its first value, its last, or one in the middle lane of its group."""
    return (0, V - 1, V // 2 + 3)[b % 3]


def targets(kind, G):
    lo = lim(kind)[0]
    return [t for t in (NIBBLE_TARGETS if nibble(kind) else BYTE_TARGETS) if t <= -lo * G]


@functools.lru_cache(maxsize=None)
def v_case(kind, V, G):
    """(slices, (bytes, shifts), the planted sums [NBLK]): block b's sums lie within half of its target T, but for
    +-T at max_pos(b, V) -- so the block's shift is right only if that one lane's maximum reaches every lane of the
    group.  The targets cycle with period 8 (bytes) or 5 (nibbles), the positions with period 3."""
    lo = lim(kind)[0]
    rng = np.random.default_rng(V * 100 + G + len(kind))
    ts = targets(kind, G)
    T = np.array([ts[b % len(ts)] for b in range(NBLK)])
    S = rng.integers(-(T[:, None] // 2), T[:, None] // 2 + 1, (NBLK, V))
    planted = np.where((T == -lo * G) | (np.arange(NBLK) % 2 == 1), -T, T)       # lo * G is reached from below only
    planted = np.where(planted > lim(kind)[1] * G, -planted, planted)
    S[np.arange(NBLK), [max_pos(b, V) for b in range(NBLK)]] = planted
    parts = slices_of(kind, spread(S.reshape(-1), G, kind, rng))
    return parts, expect(kind, parts, V), ro(planted)


# ---- 4. the quantisers on the planted bucket -------------------------------------------------------------------
def _given(kb):
    return ro(R.given_scales(kb, plants=False))


@functools.lru_cache(maxsize=None)
def q4_case(V, W, src, e0, rot):
    """(scales over the W buckets, the GIVEN scales, {w: (nibbles, flags)} for R.i8_workers(W))."""
    xs, rotate = R.bucket(V, W, src, e0)[1], SEED if rot else None
    kb = ro(r4.block_scales(list(xs), V, rotate, **R.key(e0)))
    given = _given(kb)
    return kb, given, {w: ro(*r4.quantize(xs[w], given, V, rotate, **R.key(e0))) for w in R.i8_workers(W)}


@functools.lru_cache(maxsize=None)
def sr_case(V, W, src, rot):
    """The same for i8.block_scales_sr / i8.quantize_sr: rounding stream (SR_SEED, STEP, SR_KEY), rotation R.key()."""
    xs, rotate, k = R.bucket(V, W, src)[1], SEED if rot else None, R.key()
    kb = ro(r8sr.block_scales(list(xs), V, rotate, **k))
    given = _given(kb)
    return kb, given, {w: ro(*r8sr.quantize(xs[w], given, V, SR_SEED, rotate, step=k["step"], rot_sub=k["sub"], **SR_KEY))
                       for w in R.i8_workers(W)}


@functools.lru_cache(maxsize=None)
def residuals(V, W):
    """One finite residual a worker, magnitudes 1e-3: below the ordinary blocks' values, far above TINY's."""
    return ro((np.random.default_rng(V + W).standard_normal((W, NBLK * V)) * 1e-3).astype(F32))


@functools.lru_cache(maxsize=None)
def ef_case(V, W, src, rot):
    """(scales over the W pairs, the GIVEN scales, {w: (bytes, flags, residual after)}) for i8.block_scales_ef /
    i8.quantize_ef."""
    xs, res, rotate = R.bucket(V, W, src)[1], residuals(V, W), SEED if rot else None
    kb = ro(r8ef.block_scales(list(xs), list(res), V, rotate, **R.key()))
    given = _given(kb)
    return kb, given, {w: ro(*r8ef.quantize(xs[w], res[w], given, V, rotate, **R.key())[:3]) for w in R.i8_workers(W)}


# ---- 5 and 6. the decode of the requantised gather under a key ------------------------------------------------
@functools.lru_cache(maxsize=None)
def gather_case(V, e0=0):
    """(bytes, shifts 0..7 and one above 7, scales, the rotated decode of the whole under e0)."""
    rng = np.random.default_rng(V + 17)
    q8 = rng.integers(-127, 128, NBLK * V).astype(np.int8)
    sh = (np.arange(NBLK) % 8).astype(np.uint8)
    sh[9] = 200                                           # read as 7
    kb = rng.choice([-126, -3, 0, 14, 127], NBLK).astype(np.int8)
    s16 = q8.astype(np.int16) << np.repeat(np.minimum(sh, 7), V).astype(np.int16)
    return ro(q8, sh, kb, r8.dequantize(s16, kb, V, SEED, **R.key(e0)))


# ---- 7. views of one receive buffer ------------------------------------------------------------------------------
SHARD = 128 * 3                                           # values a slice: 192 bytes of nibbles, 384 of bytes
VIEW_V = 128


@functools.lru_cache(maxsize=None)
def view_case(kind, G):
    """(the receive buffer [G, SHARD values], n, expected over the first n values of each slice): the exact nibble
    sum stops 8 values short of the shard (a ragged lane of 3 dwords), the requantisers take the 3 whole blocks."""
    lo, hi = lim(kind)
    rng = np.random.default_rng(G + len(kind))
    vals = rng.integers(lo, hi + 1, (G, SHARD))
    vals[:, 0], vals[:, 1] = lo, hi
    n = SHARD - 8 if kind == "i4.sum" else SHARD
    vals[:, n - 1] = lo
    recv = slices_of(kind, vals)
    return recv, n, expect(kind, slices_of(kind, vals[:, :n]), VIEW_V)
