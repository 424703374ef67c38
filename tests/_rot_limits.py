"""Inputs and CPU-side expectations of tests/test_gpu_rot_limits.py: the rotation (include/ina_rot.h) and the
byte wire (include/ina_i8.h) at every V, at W up to 64, on edge values, at sign keys that need the counter's
high word, and in placed outputs.  Everything here is numpy and the yardsticks tests/_rot_ref.py,
tests/_i8_ref.py and tests/_blk_ref.py; the builders are cached and their results are never written to
(tests/test_rot_limits_inputs.py asserts, without a GPU, that they reach what they are meant to reach).  The
device helpers at the end need a GPU."""
import functools

import numpy as np
import torch

from tests import _blk_ref as bref
from tests import _i8_ref as iref
from tests import _rot_ref as rref
from tests._limits import BIG, EDGE, FILL, TINY, W_LIMIT, X16, bits, same, sent, widen

F32 = np.float32
SEED, STEP, SUB = 0xC0FFEE123456789, 5, 0xFFFFFFFE      # tests/test_gpu_rot.py's key
NBLK = 41               # V = 16: two whole waves and nine blocks; V = 128: ends on half a wave
V_NEW, V_OLD = (16, 64, 128), (8, 32, 256)
SRCS = ("f32", "bf16", "f16")
W_RUNTIME = W_LIMIT + (6,)        # every one a run-time-loop W: even, odd, and the limit
# (V, W, source type) of every planted bucket the device tests run
CASES = ([(V, 4, src) for V in V_NEW for src in SRCS] + [(8, 4, "f32"), (32, 4, "bf16"), (256, 4, "f16")]
         + [c for W in W_RUNTIME for c in ((32, W, "f32"), (256, W, "bf16"))])

# the sign keys: the counter of value 0 is e0 >> 7
E0_ODD = 2**34 + 128 * 7          # an odd counter: a wave's two Philox calls are at c and c + 1, not c | 1
E0_CARRY = 2**39 - 128            # c = 2^32 - 1: the carry into the high word falls between the two calls
E0_CARRY256 = 2**39 - 256         # the same at V = 256: the second call of the first wave is the last low one
E0_HIGH = 2**45 + 256 * 5         # e0 >> 7 itself needs the high word


def e0s(V):
    return (E0_ODD, E0_CARRY, E0_HIGH) if V < 256 else (E0_CARRY256, E0_HIGH)


# one plant a block, ordinary blocks (and the GIVEN edits, blocks 1 and 3) between them
PLANT = dict(edge=5, tiny=8, big=11, zero=14, nan=17, inf2=20, nan_inf=23, negzero=26,
             i_inside=29, i_sat=31, i_leave=33, i_last2=35, wrap=37)
EDITED = (1, 3)                   # GIVEN: block 1 reads -128 (as -126), block 3 is 8 too large (clamps)
ORDINARY = tuple(s for s in range(NBLK) if s not in PLANT.values() and s not in EDITED)
K_INT, K_WRAP = 0, 40             # the GIVEN scales of the integer-side plants and of the int32 wrap plant

EDGE_FINITE = EDGE[np.isfinite(EDGE)]
BIG_F16 = np.array([65504, -65504, 65472, -65472, 65488, -65488, 65519, -65519, 65456, -65456], F32)
TINY_F16 = np.ldexp(F32(1), [-24, -23, -15, -14, -13]).astype(F32)
TINY_F16 = np.concatenate([TINY_F16, -TINY_F16, np.array([3 * 2.0**-24, -3 * 2.0**-24], F32)])


def key(e0=0):
    return dict(step=STEP, sub=SUB, e0=e0)


def blk(name_or_s, V):
    s = PLANT.get(name_or_s, name_or_s)
    return slice(s * V, (s + 1) * V)


@functools.lru_cache(maxsize=None)
def sigma(V, e0=0):
    return rref.signs(NBLK * V, SEED, **key(e0))


def big_values(V, src, sg):
    """BIG at the head of one block or repeated to fill it, rolled: the first such arrangement at which the
    butterfly under the block's signs sg leaves both an inf and an inf - inf among the rotated values (which
    adds overflow is a matter of the signs); fp16 values cannot overflow an fp32 add."""
    if src == "f16":
        return np.resize(BIG_F16, V)
    for roll in range(BIG.size):
        for count in (min(V, BIG.size), V):              # at the block's head alone, or repeated to fill it
            vals = np.zeros(V, F32)
            vals[:count] = np.resize(np.roll(BIG, roll), count)
            vals = vals if src == "f32" else widen(vals, X16[src])[1]
            r = rref.forward(vals, V, sg)
            if np.isfinite(vals).all() and np.isinf(r).any() and np.isnan(r).any():
                return vals
    raise AssertionError("no arrangement of BIG overflows to both inf and NaN")


@functools.lru_cache(maxsize=None)
def bucket(V, W, src="f32", e0=0):
    """(what the device gets: fp32 [W, n] array or 16-bit tensor, its exact fp32 widening [W, n]): 41 blocks of
    tests/_blk_ref.py's bucket (magnitudes 1e-4 .. 1e2), and one plant a block (PLANT):
      edge      the finite EDGE values (the first V of them) in worker 0, the other workers ordinary
      tiny      TINY in worker W - 1 alone (fp16: the fp16 subnormals and their neighbours), all others zero
      big       BIG in worker 0 alone, arranged by big_values (fp16: +-65504, +-65472 and what rounds to them),
                all others zero
      zero, nan, negzero   the block is 0.0 / NaN / -0.0 in every worker
      inf2      +inf from worker 1 and +inf from worker 2 at different positions
      nan_inf   a NaN from worker 0 and -inf from worker W - 1
    and the integer-side plants: x[j] = sigma[j] * c rotates exactly to r[0] = c * 2^floor(m/2) and zeros, so
    under the GIVEN scale K_INT = 0 worker w adds exactly the integer planted for it to value 0 of the block:
      i_inside  every worker -32768: no summand saturates, the sum does
      i_sat     every worker +32768: every summand saturates
      i_leave   28672, 28672, -28672, -28672, 0, ..: the running sum leaves int16 after two workers and is
                back at 0 after four (the sum is saturated once, at the end)
      i_last2   20480 in workers W - 2 and W - 1 alone: the sum saturates only once worker W - 1 is added
      wrap      every worker 1.0, GIVEN scale K_WRAP = 40: every int32 summand saturates at 2^31 - 1 and the
                W-way sum wraps
    (the integers are exact in bf16 and fp16 too).  16-bit sources: every value is rounded to the type first.

    int16 flags of the planted blocks.  AUTO: nan, inf2, nan_inf always; big for f32 / bf16 (the butterfly
    overflows: finite inputs, rotated values +-inf and NaN, scale -126; the fp16 values cannot overflow an
    fp32 add); edge from V = 16 on (the 3e38 pair, at values 10 and 11, overflows in stage 0; fp16 rounds it to
    +-inf; the first 8 EDGE values hold neither).  No other planted block flags under AUTO.  GIVEN adds
    i_inside, i_sat, i_last2 and wrap; i_leave, tiny, zero and negzero never flag."""
    m, n = V.bit_length() - 1, NBLK * V
    x = bref.bucket(np.random.default_rng(7000 + 100 * V + W), W, n, V, lo=-4.0, hi=2.0)

    def alone(name, w, vals):
        x[:, blk(name, V)] = 0
        x[w, PLANT[name] * V:PLANT[name] * V + min(V, vals.size)] = vals[:V]

    x[0, PLANT["edge"] * V:PLANT["edge"] * V + min(V, EDGE_FINITE.size)] = EDGE_FINITE[:V]
    alone("tiny", W - 1, TINY_F16 if src == "f16" else TINY)
    alone("big", 0, big_values(V, src, sigma(V, e0)[blk("big", V)]))
    x[:, blk("zero", V)], x[:, blk("nan", V)], x[:, blk("negzero", V)] = 0.0, np.nan, -0.0
    x[1, PLANT["inf2"] * V + 1], x[2, PLANT["inf2"] * V + 6] = np.inf, np.inf
    x[0, PLANT["nan_inf"] * V + 2], x[W - 1, PLANT["nan_inf"] * V + 5] = np.nan, -np.inf
    unit = sigma(V, e0).astype(F32) * F32(2.0 ** -(m // 2))
    per_worker = {"i_inside": np.full(W, -32768.0), "i_sat": np.full(W, 32768.0), "i_leave": np.zeros(W),
                  "i_last2": np.zeros(W), "wrap": np.ones(W)}
    per_worker["i_leave"][:4] = 28672, 28672, -28672, -28672
    per_worker["i_last2"][W - 2:] = 20480
    for name, c in per_worker.items():
        x[:, blk(name, V)] = c.astype(F32)[:, None] * unit[blk(name, V)][None, :]
    if src == "f32":
        got, xs = x, x
    else:
        got, xs = widen(x, X16[src])
        for name in per_worker:
            assert np.array_equal(xs[:, blk(name, V)], x[:, blk(name, V)]), (name, src)
    xs.flags.writeable = False
    return got, xs


def flagged_plants(V, src, mode):
    """The planted blocks whose int16 flag must be set (bucket()'s docstring); every other planted one is clear."""
    names = {"nan", "inf2", "nan_inf"}
    if src != "f16":
        names.add("big")
    if V >= 16:
        names.add("edge")
    if mode == "given":
        names |= {"i_inside", "i_sat", "i_last2", "wrap"}
    return sorted(PLANT[name] for name in names)


def given_scales(auto, plants=True):
    """AUTO with block 1 set to -128 and block 3 raised by 8 (the existing tests' edits), and the integer-side
    plants at their stated scales."""
    g = auto.copy()
    g[1], g[3] = -128, min(int(g[3]) + 8, 127)
    if plants:
        for name in ("i_inside", "i_sat", "i_leave", "i_last2"):
            g[PLANT[name]] = K_INT
        g[PLANT["wrap"]] = K_WRAP
    return g


@functools.lru_cache(maxsize=None)
def rotated(V, W, src="f32", e0=0):
    """r of the contract for every worker, [W, n]."""
    sg = sigma(V, e0)
    r = np.stack([rref.forward(x, V, sg) for x in bucket(V, W, src, e0)[1]])
    r.flags.writeable = False
    return r


@functools.lru_cache(maxsize=None)
def fused(V, W, src, e0, nbits, mode):
    """(q, flags or None, kblk the call returns, the decode of q) of one fused reduce; mode "auto" / "given"."""
    rs = list(rotated(V, W, src, e0))
    if mode == "auto":
        kb = bref.kblk_ref(rs, V, W, nbits)
    else:
        kb = given_scales(fused(V, W, src, e0, nbits, "auto")[2])
    if nbits == 32:
        q, flags = bref.quantize_reduce_i32(rs, kb, V), None
    else:
        q, flags = bref.quantize_reduce_i16(rs, kb, V)
    y = rref.dequantize(q, kb, V, SEED, **key(e0))
    for a in (q, flags, kb, y):
        if a is not None:
            a.flags.writeable = False
    return q, flags, kb, y


def i8_workers(W):
    return sorted({0, 1, 2, W - 1})       # EDGE / BIG / NaN; an inf each; TINY and -inf


@functools.lru_cache(maxsize=None)
def i8_case(V, W, src, e0, rot):
    """(scales over the W buckets, the GIVEN scales, {w: (bytes, flags)} for i8_workers(W))."""
    xs, rotate = bucket(V, W, src, e0)[1], SEED if rot else None
    kb = iref.block_scales(list(xs), V, rotate, **key(e0))
    given = given_scales(kb, plants=False)
    out = {w: iref.quantize(xs[w], given, V, rotate, **key(e0)) for w in i8_workers(W)}
    kb.flags.writeable = given.flags.writeable = False
    return kb, given, out


def slice_lo(V):
    """An odd multiple of 128 that is a multiple of V; the slice is 9 blocks."""
    lo = 128 if V <= 128 else 256 * 3
    return lo, lo + 9 * V


@functools.lru_cache(maxsize=None)
def ps_case(V, W, ws):
    """(local, paras [W, n], kblk, expected) for rot.ps_combine_ina: the planted bucket as the parameters, the
    replay of the deltas -> decode -> local + xhat * float32(ws) in two fp32 operations."""
    paras = bucket(V, W)[1]
    local = bref.bucket(np.random.default_rng(9000 + V), 1, NBLK * V, V, lo=-4.0, hi=2.0)[0]     # ordinary, finite
    with np.errstate(all="ignore"):
        deltas = [(p - local).astype(F32) for p in paras]
        q, _, kb = rref.quantize_reduce(deltas, V, SEED, **key())
        xhat = rref.dequantize(q, kb, V, SEED, **key())
        want = (local + (xhat * F32(ws)).astype(F32)).astype(F32)
    return local, paras, kb, want


# ---- device helpers ---------------------------------------------------------------------------
def out16(n, dtype):
    """A sent() output 16 bytes past a 256-byte boundary."""
    v = sent(n, dtype, 16 // torch.empty(0, dtype=dtype).element_size())
    assert v.data_ptr() % 256 == 16
    return v


def canon(a):
    """fp32 as bits, every NaN as one pattern: the contract leaves a NaN's sign and payload open."""
    a = np.ascontiguousarray(a, F32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), bits(a))


def same_out(got, want, what):
    """_limits.same (bit for bit, FILL after the result) and FILL in the bytes before the view; fp32 results
    compare with any NaN matching any NaN."""
    torch.cuda.synchronize()
    off = got.storage_offset()
    front = got._base[:off].view(torch.uint8).cpu().numpy() if off else np.empty(0, np.uint8)
    assert np.array_equal(front, np.full(front.size, FILL, np.uint8)), f"{what}: wrote before the start"
    if got.dtype == torch.float32:
        g = bits(got.detach().cpu().numpy()).copy()
        g[:want.size] = canon(g[:want.size].view(F32))
        same(g, canon(want), what)
    else:
        same(got, want, what)


def untouched(*outs):
    torch.cuda.synchronize()
    for o in outs:
        b = (o._base if o._base is not None else o).view(torch.uint8).cpu().numpy()
        assert np.array_equal(b, np.full(b.size, FILL, np.uint8)), "a refused call wrote to its output"
