"""Inputs and CPU-side expectations of tests/test_gpu_limits.py: the ABI's stated limits
(include/ina.h: 1 <= W <= 64, k in [-126, 127]; csrc/ina_shard.hip: at most 64 ranks on the int16
wire).  Everything here is numpy, the CPU oracle and tests/_blk_ref.py; the builders are cached
and their results are never written to.  The device helpers at the end need a GPU."""
import functools

import numpy as np
import torch

from oracle import oracle as orc

DEV = "cuda:0"
FILL, PAD = 0xA5, 3                     # every caller-supplied output: 0xA5 bytes, PAD elements longer
W_LIMIT = (17, 33, 63, 64)              # runtime-W bodies; past W = 8 the grid cap changes as well
V1 = 32
N1 = 4 * V1 * 5 + 13                    # whole chunks, a ragged tail, a partial last slot
N_STRIDE, SMALL_CAP = 70_001, 4         # with 4 workgroups every default-cap kernel strides
K_LIMITS = (-126, -125, 31, 126, 127)
K_REFUSED = (-127, 128)
I32_MIN, I32_MAX = -2**31, 2**31 - 1
X16 = {"bf16": torch.bfloat16, "f16": torch.float16}

# tests/test_gpu_parity.py's EDGE / mixed_floats
EDGE = np.array([0.0, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5, 1e-45, -1e-45, 1e-38, np.inf, -np.inf,
                 np.nan, 3e38, -3e38, 32767.5, -32768.5, 2147483520.0, 2147483648.0,
                 -2147483648.0, -2147483904.0, 0.49999997, -0.49999997], np.float32)
TINY = np.ldexp(np.float32(1), [-149, -148, -127, -126, -125]).astype(np.float32)
TINY = np.concatenate([TINY, -TINY, np.array([1e-40, -1e-40], np.float32)])
# what still quantises to something at k = -126: ties and the top of the fp32 range
BIG = (np.array([1, -1, 1.5, -1.5, 2.5, -2.5, 0.5, -0.5, 3, 3.99], np.float64) * 2.0**126).astype(np.float32)


def mixed_floats(rng, n):
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)).astype(np.float32)
    x[:min(n, len(EDGE))] = EDGE[:min(n, len(EDGE))]
    return x


def mixed(flags):
    """The oracle's flags are neither all set nor all clear."""
    assert 0 < int(flags.sum()) < flags.size, (int(flags.sum()), flags.size)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize]).reshape(-1)


def widen(x, dtype):
    """fp32 [.., n] -> (16-bit host tensor, its exact fp32 widening: what the oracle takes)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return t, t.float().numpy()


def round16(f32, dtype):
    """tests/test_gpu_x16.py's reference rounding: the fp32 result rounded once, as bits."""
    return torch.from_numpy(np.ascontiguousarray(f32)).to(dtype).view(torch.int16).numpy()


# ---- part 1: W at and near the limit ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def i32_bufs(W, n):
    """[W, n] int32, full range; W x INT32_MIN in the vector loop, W x INT32_MAX mid-way, half of
    each in the last (tail) value: the result is the wrapping sum."""
    rng = np.random.default_rng(100 * W + n % 97)
    x = rng.integers(-2**31, 2**31, (W, n), dtype=np.int64).astype(np.int32)
    x[:, 5], x[:, n // 2] = I32_MIN, I32_MAX
    x[:W // 2, n - 1], x[W // 2:, n - 1] = I32_MIN, I32_MAX
    return x


def _at(slot, V, n):
    return slot * V + (7 * slot + 3) % min(V, n - slot * V)


WILD0, WILD_STEP = 12, 50


@functools.lru_cache(maxsize=None)
def i16_plan(W, n, V):
    """[W, n] int16 whose sums stay in range (|noise| <= 32000 / W) except where planted, one plant a
    slot: 2 every worker +32767; 4 every worker -32768; 6 the running sum leaves int16 after two
    workers and is back at 0 after four (never flagged); 8 and the last slot: 20000 in workers W - 2
    and W - 1 and 0 elsewhere, so the sum saturates only once worker W - 1 is added (one int16 value
    cannot saturate a sum alone: the lone saturating value and the lone NaN in worker W - 1 exist on
    the float paths only, f16path_bufs); 12, 62, ..: full-range noise.  Returns (values, slots that
    must not flag, slots that must)."""
    rng = np.random.default_rng(200 * W + n % 97 + V)
    A = 32000 // W
    q = rng.integers(-A, A + 1, (W, n)).astype(np.int16)
    nslot = -(-n // V)
    q[:, _at(2, V, n)] = 32767
    q[:, _at(4, V, n)] = -32768
    e = _at(6, V, n)
    q[:, e], q[0:2, e], q[2:4, e] = 0, 30000, -30000
    e = _at(8, V, n)
    q[:, e], q[W - 2:, e] = 0, 20000
    q[:, n - 1], q[W - 2:, n - 1] = 0, -20000
    for s in range(WILD0, nslot - 1, WILD_STEP):
        q[:, s * V:(s + 1) * V] = rng.integers(-32768, 32768, (W, V)).astype(np.int16)
    return q, (0, 1, 3, 5, 6, 7), (2, 4, 8, nslot - 1)


K16 = 10


@functools.lru_cache(maxsize=None)
def f16path_bufs(W, n, V):
    """fp32 [W, n] for the fused int16 reduce at k = 10: i16_plan / 2^10 (exact), and in slots of
    their own a NaN and a clamping value in worker W - 1 alone, EDGE in worker 0 and in worker W - 1."""
    q, clear, flagged = i16_plan(W, n, V)
    x = q.astype(np.float32) / np.float32(2**K16)
    for slot, val in ((10, np.nan), (14, 1e9)):
        e = _at(slot, V, n)
        x[:, e], x[W - 1, e] = 0, val
    x[0, 16 * V:16 * V + EDGE.size] = EDGE
    x[W - 1, 18 * V:18 * V + EDGE.size] = EDGE
    return x, clear, flagged + (10, 14, 16, 18)


K32 = 16


@functools.lru_cache(maxsize=None)
def f32path_bufs(W, n):
    """fp32 [W, n] for the fused int32 reduce at k = 16: mixed_floats, EDGE in worker 0 (head),
    worker 16 (middle) and worker W - 1 (tail), every worker saturating high / low / half each."""
    rng = np.random.default_rng(300 * W + n % 97)
    x = np.stack([mixed_floats(rng, n) for _ in range(W)])
    x[1:, :EDGE.size] = x[1:, EDGE.size:2 * EDGE.size]
    x[16, 300:300 + EDGE.size] = EDGE
    x[W - 1, n - EDGE.size:] = EDGE
    x[:, 100], x[:, 101] = 3e38, -3e38
    x[:W // 2, 102], x[W // 2:, 102] = 3e38, -3e38
    return x


@functools.lru_cache(maxsize=None)
def ps_bufs(W, n):
    """(local, paras [W, n]) for the fp32 combine and the INA combine at k = 16: finite values (no
    inf - inf, whose NaN sign is the processor's), large deltas in worker W - 1 and worker 16."""
    rng = np.random.default_rng(400 * W + n % 97)
    local = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
    paras = (local + rng.standard_normal((W, n)).astype(np.float32) * np.float32(1e-2)).astype(np.float32)
    paras[W - 1, 7::50] += np.float32(1e3)
    paras[16, 11::50] -= np.float32(1e6)          # saturates q32 at k = 16
    paras[W - 1, n - 1] = np.float32(3e38)
    return local, paras


@functools.lru_cache(maxsize=None)
def quiet_bufs(W, n):
    """(xs [W, n], base) of magnitude 1e-3: absmax_multi must find what a test plants."""
    rng = np.random.default_rng(500 * W + n % 97)
    return ((rng.standard_normal((W, n)) * 1e-3).astype(np.float32),
            (rng.standard_normal(n) * 1e-3).astype(np.float32))


@functools.lru_cache(maxsize=None)
def blk_bufs(W, n, V):
    """tests/_blk_ref.py's bucket (neighbouring blocks differ in k) with a NaN in worker W - 1 and an
    inf in worker 16, in blocks of their own: the int16 flags are mixed under AUTO scales too."""
    from tests import _blk_ref as ref
    x = ref.bucket(np.random.default_rng(600 * W + n % 97), W, n, V)
    x[W - 1, _at(3, V, n)] = np.nan
    x[16, _at(5, V, n)] = np.inf
    x[W - 1, n - 1] = np.nan
    return x


# ---- part 2: k at the limits ------------------------------------------------------------------
S_SPECIAL = [0, 1, -1, 3, -3, 32767, -32767, -32768, I32_MAX, I32_MIN, 2**23, -2**23, 2**24 + 1, -(2**24 + 1)]
S16_SPECIAL = [0, 1, -1, 3, -3, 32767, -32767, -32768]
L_SPECIAL = np.array([0.0, -0.0, 2.0**-149, -2.0**-149, 2.0**-127, -2.0**-127, 2.0**-126, -2.0**-126,
                      1.0, -1.0, 3e38, -3e38], np.float32)
N_DEQ = 1037


@functools.lru_cache(maxsize=None)
def deq_sources():
    """(int32 [1037], int16 [1037]): the special values at the head and, reversed, at the tail."""
    rng = np.random.default_rng(71)
    s32 = rng.integers(-2**31, 2**31, N_DEQ, dtype=np.int64)
    s32[100:400] >>= rng.integers(0, 31, 300)
    s16 = rng.integers(-2**15, 2**15, N_DEQ, dtype=np.int64)
    for s, sp in ((s32, S_SPECIAL), (s16, S16_SPECIAL)):
        s[:len(sp)], s[-len(sp):] = sp, sp[::-1]
    return s32.astype(np.int32), s16.astype(np.int16)


def sum_ints(rng, n):
    """int32 [n] sums: every S_SPECIAL against every L_SPECIAL first (ps_local's layout), then full
    range, |s| < 8 (finite even at k = -126) and |s| < 2^20 by turns."""
    s = rng.integers(-2**31, 2**31, n, dtype=np.int64)
    s[1::3] = rng.integers(-7, 8, s[1::3].size)
    s[2::3] = rng.integers(-2**20, 2**20, s[2::3].size)
    head = np.repeat(S_SPECIAL, L_SPECIAL.size)
    s[:head.size] = head
    # +-3 at every tenth value (ps_local searches there): 3 * fp32(1/3) is inexact and, unlike any larger
    # sum, still finite at k = -126, so every k has values where one rounding and two can differ
    s[head.size:n:10] = rng.choice([3, -3], s[head.size:n:10].size)
    return s.astype(np.int32)


def two_roundings(local, d, ws):
    """local + fp32(fp32(d) * fp32(weight_step)): the PS update as the existing tests state it."""
    with np.errstate(over="ignore", under="ignore"):
        return (local + (d * np.float32(ws)).astype(np.float32)).astype(np.float32)


def _one_rounding_differs(local, d, ws):
    with np.errstate(over="ignore", under="ignore"):
        one = (local.astype(np.float64) + d.astype(np.float64) * np.float64(np.float32(ws))).astype(np.float32)
    return one.view(np.uint32) != two_roundings(local, d, ws).view(np.uint32)


def fma_differs(local, d, ws):
    """Where ONE rounding of local + d * fp32(ws) (in float64: the product is exact there) gives other
    bits than the two roundings: a contracted multiply-add fails the comparison at these."""
    return np.flatnonzero(_one_rounding_differs(local, d, ws))


def _sane(x):
    return np.clip(np.nan_to_num(x, nan=1.0, posinf=3e38, neginf=-3e38), -3e38, 3e38).astype(np.float32)


def ps_local(rng, d, ws, tries=64):
    """local for the update d: L_SPECIAL against every special sum, then values of the update's own
    magnitude (the sum then rounds: the only place one and two roundings can differ); every fifth of
    those is the first of `tries` such values at which they do differ, where there is one."""
    n = d.size
    mult = [-1.75, -1.0, -0.6, 0.3, 1.0, 1.9, 700.0]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = d.astype(np.float64) * np.float64(np.float32(ws))
        local = _sane(t * rng.choice(mult, n) * (1 + rng.random(n)))
        idx = np.arange(len(S_SPECIAL) * L_SPECIAL.size, n, 5)
        cand = _sane(t[idx] * rng.choice(mult, (tries, idx.size)) * (1 + rng.random((tries, idx.size))))
    hit = np.stack([_one_rounding_differs(c, d[idx], ws) for c in cand])
    local[idx] = np.where(hit.any(axis=0), cand[hit.argmax(axis=0), np.arange(idx.size)], local[idx])
    head = np.tile(L_SPECIAL, len(S_SPECIAL))
    local[:head.size] = head[:n]
    return local


@functools.lru_cache(maxsize=None)
def ps_case(k, ws, n):
    """(local, sums, expected update, indices where an FMA would differ) for one k and weight_step.
    With weight_step = 1.0 the product d * 1.0 is exact, so one rounding and two agree everywhere:
    only weight_step = 1/3 can (and must) have such indices."""
    rng = np.random.default_rng(abs(k) * 7 + n)
    s = sum_ints(rng, n)
    d = orc.dequantize_i32(s, k)
    local = ps_local(rng, d, ws)
    want = two_roundings(local, d, ws)
    assert not np.isnan(want).any()
    fma = fma_differs(local, d, ws)
    assert (fma.size > 0) == (ws != 1.0), (k, ws, fma.size)
    return local, s, want, fma


@functools.lru_cache(maxsize=None)
def combine_ina_case(k, ws, W=3, n=N_DEQ):
    """(local, paras, expected, FMA indices) for ps.combine_ina at one k: deltas of about 2^20 / 2^k on
    a local of about 2^10 / 2^k, some saturating; the oracle's update restated as the two roundings."""
    rng = np.random.default_rng(abs(k) * 11 + W)
    lmag, dmag = (1000, 2**20) if k > -100 else (0.5, 4)      # near k = -126 only |sum| < 4 stays finite
    with np.errstate(over="ignore", under="ignore"):
        unit = np.ldexp(np.float64(1), -k)
        local = np.clip(rng.standard_normal(n) * lmag * unit, -3e38, 3e38).astype(np.float32)
        local[:L_SPECIAL.size] = L_SPECIAL
        delta = rng.integers(-dmag, dmag, (W, n)).astype(np.float64)
        delta[:, 50::40] *= 2.0**12                                   # past int32 at this k
        paras = np.clip(local.astype(np.float64) + delta * unit, -3e38, 3e38).astype(np.float32)
        deltas = [(p - local).astype(np.float32) for p in paras]
    d = orc.dequantize_i32(orc.quantize_reduce_i32(deltas, k), k)
    want = orc.ps_combine_ina_f32(local, list(paras), k, ws)
    assert np.array_equal(bits(want), bits(two_roundings(local, d, ws))) and not np.isnan(want).any()
    fma = fma_differs(local, d, ws)
    assert (fma.size > 0) == (ws != 1.0), (k, ws, fma.size)
    return local, paras, want, fma


@functools.lru_cache(maxsize=None)
def quant_inputs(W, n, V):
    """fp32 [W, n] for the quantise side at k = -126 / 127: mixed_floats with the subnormals and the
    top of the range in every worker; slot 1 holds zeros and subnormals too small to count even at
    k = 127, so the int16 flags stay mixed at both scales."""
    rng = np.random.default_rng(800 + W + n)
    x = np.stack([mixed_floats(rng, n) for _ in range(W)])
    for w in range(W):
        x[w, 2 * V:2 * V + TINY.size] = np.roll(TINY, w)
        x[w, 3 * V:3 * V + BIG.size] = np.roll(BIG, w)
        x[w, n - BIG.size:] = BIG
    x[:, V:2 * V] = 0
    x[:, V + 3], x[:, V + 4] = 2.0**-149, -(2.0**-140)
    return x


# ---- part 3: the int16 wire at its rank limit --------------------------------------------------
WIRE_K = 11
WIRE_V = (4, 8, 32, 256, 100, 512, 1, 6)      # ballot writer at lps 1, 2, 8, 64; scalar + memset
WIRE_KINDS = ("all_hi", "all_lo", "all_clamp", "all_nan", "zeros", "one_short_of_clamp", "sum_leaves",
              "one_clamps_low")
WIRE_ROT = (0, 3, 7)                           # the three sizes of one V start at kinds 0, 3, 7


def wire_sizes(V):
    return (3 * V + 1, 5 * V, 64 * 4 * 3 + 7)


@functools.lru_cache(maxsize=None)
def wire_case(R, V, which):
    """R ranks' buckets [R, n] at k = 11.  Slot 0 is noise that never saturates; slot s >= 1 holds one
    planted value of WIRE_KINDS[(s - 1 + WIRE_ROT[which]) % 8] among such noise, so the three sizes of
    a V cover every kind:
      all_hi / all_lo       every rank +32767 / -32768 (the 22-bit field's bottom, -2^21, at R = 64)
      all_clamp / all_nan   every rank clamps high / is NaN: the count is R, the word's top at 64
      one_short_of_clamp    R - 1 ranks clamp high, the last sits at -32768
      sum_leaves            30000 each: no rank saturates, the sum leaves int16 (from R = 2)
      one_clamps_low        the last rank clamps low, the others add up to 3 (R - 1): in range, flagged
    Returns (buckets, {kind: [element, ..]})."""
    n = wire_sizes(V)[which]
    rng = np.random.default_rng(R * 1000 + V * 3 + which)
    A = 32000 // R
    x = rng.integers(-A, A + 1, (R, n)).astype(np.float32) / np.float32(2**WIRE_K)
    where = {}
    for s in range(1, -(-n // V)):
        kind = WIRE_KINDS[(s - 1 + WIRE_ROT[which]) % len(WIRE_KINDS)]
        e = _at(s, V, n)
        col = {"all_hi": 32767 / 2048, "all_lo": -16.0, "all_clamp": 1e9, "all_nan": np.nan, "zeros": 0.0,
               "one_short_of_clamp": 1e9, "sum_leaves": 30000 / 2048, "one_clamps_low": 3 / 2048}[kind]
        if kind == "zeros":
            x[:, s * V:(s + 1) * V] = 0
        x[:, e] = col
        if kind == "one_short_of_clamp":
            x[R - 1, e] = -16.0
        if kind == "one_clamps_low":
            x[R - 1, e] = -1e9
        where.setdefault(kind, []).append(e)
    return x, where


# ---- device helpers ---------------------------------------------------------------------------
def ops():
    from ina_amd import ops as o
    return o


def dev(a, off=0):
    """A device copy of a 1-D array / tensor; off = 1: a view one element past a 16-byte boundary."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = buf[off:]
    v.copy_(t)
    assert v.data_ptr() % 16 == off * t.element_size()
    return v


def dev_rows(x, off=0):
    """The rows of a [W, n] array / tensor as W device views, each 16-byte aligned (off = 0) or one
    element past a 16-byte boundary (off = 1): one upload."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    W, n = t.shape
    pitch = (n + off + 15) // 16 * 16
    buf = torch.zeros((W, pitch), dtype=t.dtype, device=DEV)
    buf[:, off:off + n].copy_(t)
    rows = [buf[w, off:off + n] for w in range(W)]
    assert all(r.data_ptr() % 16 == off * t.element_size() and r.is_contiguous() for r in rows)
    return rows


def sent(n, dtype, off=0):
    """An output of n elements plus PAD, every byte FILL; off as in dev()."""
    buf = torch.empty(n + PAD + off, dtype=dtype, device=DEV)
    buf.view(torch.uint8).fill_(FILL)
    return buf[off:]


def same(got, want, what):
    """Bit for bit; a device result longer than `want` must still hold FILL past it."""
    if isinstance(got, torch.Tensor):
        torch.cuda.synchronize()
        got = got.detach().contiguous().view(torch.uint8).cpu().numpy()
    g, w = bits(got), bits(want)
    if g.dtype != w.dtype:
        g = g.view(w.dtype)
    assert g.size >= w.size, what
    bad = np.flatnonzero(g[:w.size] != w)
    assert np.array_equal(g[:w.size], w), \
        f"{what}: {bad.size} of {w.size} differ, first at {bad[0]}: got {int(g[bad[0]]):#x}, want {int(w[bad[0]]):#x}"
    rest = np.ascontiguousarray(g[w.size:]).view(np.uint8)
    assert np.array_equal(rest, np.full(rest.size, FILL, np.uint8)), f"{what}: wrote past the end"
