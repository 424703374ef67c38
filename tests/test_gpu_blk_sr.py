"""Stochastic rounding with per-block scales on the device (include/ina_blk_sr.h, ina_amd.blk_sr).

Replay: every integer, wire word, flag and computed scale is bit for bit tests/_blk_sr_ref.py, whatever the
dtype, the block size (vector and value-by-value path), the alignment, the size (ragged chunks, a short
last block, several passes of a capped grid), the worker count (every specialisation, the run-time loop
and the re-read AUTO instance) or the scale mode.  Then the header's four consequences against the
device's own siblings, the bias of the 8-way sum, and what the pair buys on the int16 wire."""
import numpy as np
import pytest
import torch

from tests import _blk_ref as bref
from tests import _blk_sr_ref as bsr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
WS = (1, 2, 3, 4, 8, 16)              # 1, 2, 4, 8, 16 specialised; 3 the run-time loop; int16 at 16: re-read
SIZES = (1, 37, 1029, 6181)           # ragged chunks, a short last block, more than one pass of a capped grid
LAYOUTS = {"V32": (32, False), "V256": (256, False), "V12": (12, False), "V32-misaligned": (32, True)}
SEED = 0xC0FFEE123456789
STEP, SUB, E0 = 5, 0xFFFFFFFE, (1 << 34) + 8          # sub + w wraps; e0 needs 64 bits
GUARD = 16
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _mods():
    from ina_amd import blk, blk_sr, ops, sr, wire
    return blk_sr, blk, sr, ops, wire


_BUCKETS = {}


def buckets(dtype, n, V):
    """16 seeded buckets of n values as (CPU tensors of dtype, their exact float32 widenings), block
    magnitudes log-uniform over six decades; NaN and +-inf where n holds them."""
    key = (dtype, n, V)
    if key not in _BUCKETS:
        rng = np.random.default_rng(n * 1000 + V)
        x = bref.bucket(rng, 16, n, V, lo=-4.0, hi=2.0)
        if n >= 37:
            x[0, 3], x[1, 5], x[0, n - 1] = np.nan, np.inf, -np.inf
        ts = [torch.from_numpy(r).to(dtype) for r in x]
        _BUCKETS[key] = (ts, [t.float().numpy() for t in ts])
    return _BUCKETS[key]


_GIVEN = {}


def given_scales(dtype, n, V):
    """Scales to read: the 16-summand int16 scales of the 16 buckets, then a -128 (read as -126) and a
    block whose scale is 8 too large for int16 (it saturates)."""
    key = (dtype, n, V)
    if key not in _GIVEN:
        kb = bsr.kblk_ref(buckets(dtype, n, V)[1], V, 16, 16)
        if kb.size > 2:
            kb[1] = -128
        if kb.size > 3:
            kb[3] = min(int(kb[3]) + 8, 127)
        _GIVEN[key] = kb
    return _GIVEN[key]


def dev(t, mis=False):
    """t on the device; mis: 4 bytes into its allocation (off the vector path's alignment)."""
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    off = 4 // t.element_size() if mis else 0
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t)
    v = buf[off:]
    assert not mis or v.data_ptr() % (4 * t.element_size())
    return v


def host(t):
    return t.cpu().numpy()


class Guarded:
    """An output of n elements, 4 bytes off where mis, between GUARD sentinels on each side."""

    def __init__(self, n, dtype, mis=False, fill=0x5A):
        off = 4 // torch.empty(0, dtype=dtype).element_size() if mis else 0
        self.buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=dtype, device=DEV)
        self.fill, self.lo, self.hi = fill, GUARD + off, GUARD + off + n
        self.t = self.buf[self.lo:self.hi]

    def check(self, what):
        h = host(self.buf)
        assert (h[: self.lo] == self.fill).all() and (h[self.hi:] == self.fill).all(), what
        return h[self.lo:self.hi]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def run_reduce(bs, bufs, V, n, mis, kblk=None, degree=None, **kw):
    """Both fused calls into guarded outputs: (sums32, scales32), (sums16, flags, scales16)."""
    nblk = -(-n // V)
    g, kg = Guarded(n, torch.int32, mis), Guarded(nblk, torch.int8)
    if kblk is not None:
        kg.t.copy_(kblk)
    bs.quantize_reduce(bufs, V, SEED, kblk=None if kblk is None else kg.t, degree=degree, out=g.t,
                       kblk_out=kg.t, **kw)
    r32 = (g.check("i32"), kg.check("scales32"))
    g, f, kg = Guarded(n, torch.int16, mis), Guarded(nblk, torch.uint8), Guarded(nblk, torch.int8)
    if kblk is not None:
        kg.t.copy_(kblk)
    bs.quantize_reduce_i16(bufs, V, SEED, kblk=None if kblk is None else kg.t, degree=degree, out=g.t,
                           overflow=f.t, kblk_out=kg.t, **kw)
    return r32, (g.check("i16"), f.check("flags"), kg.check("scales16"))


def check_reduce(bs, dtype, n, V, W, mis, auto, degree=None, what=""):
    ts, xs = buckets(dtype, n, V)
    ts, xs = ts[:W], xs[:W]
    kw = dict(step=STEP, sub=SUB, e0=E0)
    what = f"{what} {dtype} V={V} n={n} W={W} mis={mis} auto={auto}"
    if auto:
        deg = degree or W
        k32, k16 = bsr.kblk_ref(xs, V, deg, 32), bsr.kblk_ref(xs, V, deg, 16)
        kd = None
    else:
        k32 = k16 = given_scales(dtype, n, V)
        kd = torch.from_numpy(k32).to(DEV)
    (s32, g32), (s16, f16, g16) = run_reduce(bs, [dev(t, mis) for t in ts], V, n, mis, kblk=kd, degree=degree, **kw)
    same(g32, k32, what + " scales32")
    same(g16, k16, what + " scales16")
    same(s32, bsr.quantize_reduce(xs, k32, V, SEED, **kw), what + " i32")
    w16, wf = bsr.quantize_reduce_i16(xs, k16, V, SEED, **kw)
    same(s16, w16, what + " i16")
    same(f16, wf, what + " flags")
    return wf


# ---- replay ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_replay_given_scales(dtype, layout):
    bs, _, _, ops, _ = _mods()
    V, mis = LAYOUTS[layout]
    flagged = clean = 0
    try:
        for n in SIZES:
            if n == SIZES[-1]:
                ops.set_tuning(max_blocks=2)              # every grid-stride loop takes several passes
            for W in WS:
                wf = check_reduce(bs, dtype, n, V, W, mis, auto=False)
                flagged, clean = flagged + int(wf.sum()), clean + int((wf == 0).sum())
    finally:
        ops.set_tuning(max_blocks=16384)
    assert flagged and clean                              # NaN, inf and the too-large scale flagged; most blocks not


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_replay_auto_scales(dtype, layout):
    bs, _, _, ops, _ = _mods()
    V, mis = LAYOUTS[layout]
    try:
        for n in SIZES:
            if n == SIZES[-1]:
                ops.set_tuning(max_blocks=2)
            # (the replay's exact-rational scales cost a millisecond a block: the two middle sizes at every
            # W, the smallest and the largest at the run-time loop and at the re-read instance)
            for W in (WS if n in SIZES[1:3] else (3, 16)):
                check_reduce(bs, dtype, n, V, W, mis, auto=True)
        check_reduce(bs, dtype, SIZES[2], V, 4, mis, auto=True, degree=64, what="degree > W")
    finally:
        ops.set_tuning(max_blocks=16384)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_bucket_replay_and_scales(dtype, layout):
    bs, _, _, ops, _ = _mods()
    V, mis = LAYOUTS[layout]
    kw = dict(step=STEP, sub=SUB, e0=E0)
    try:
        for n in SIZES:
            if n == SIZES[-1]:
                ops.set_tuning(max_blocks=2)
            ts, xs = buckets(dtype, n, V)
            kb = given_scales(dtype, n, V)
            kd = torch.from_numpy(kb).to(DEV)
            x = dev(ts[2], mis)
            for fn, ref in ((bs.quantize, bsr.quantize), (bs.quantize_i16_wire, bsr.quantize_i16_wire)):
                g = Guarded(n, torch.int32, mis)
                fn(x, kd, V, SEED, out=g.t, **kw)
                same(g.check(fn.__name__), ref(xs[2], kb, V, SEED, **kw), f"{fn.__name__} {dtype} {layout} n={n}")
            if n <= SIZES[2]:
                for bits, W, degree in ((16, 3, 64), (32, 2, None)):
                    g = Guarded(-(-n // V), torch.int8)
                    bs.block_scales([dev(t, mis) for t in ts[:W]], V, bits=bits, degree=degree, out=g.t)
                    same(g.check("scales"), bsr.kblk_ref(xs[:W], V, degree or W, bits), f"block_scales {dtype} {layout} n={n}")
    finally:
        ops.set_tuning(max_blocks=16384)


def test_wire_words_carry_the_saturation_bit():
    bs, _, _, _, _ = _mods()
    n, V = 1029, 32
    ts, xs = buckets(torch.float32, n, V)
    kb = given_scales(torch.float32, n, V)
    w = host(bs.quantize_i16_wire(dev(ts[0]), torch.from_numpy(kb).to(DEV), V, SEED))
    sat = (w + (1 << 21)) >> 22                  # the count above the sign-extended q16
    assert set(np.unique(sat)) == {0, 1} and sat[3 * V:4 * V].any() and sat[3] == 1       # the large scale; the NaN
    assert (np.abs((w - (sat << 22))) <= 32768).all()


# ---- consequence 1: per block, the global-k sibling on that block alone ------------------------------
@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_per_block_is_the_global_k_sibling(dtype, mis):
    bs, _, sr, _, _ = _mods()
    n, V, e0 = 1029, 32, 1 << 33
    ts, _ = buckets(dtype, n, V)
    kb = given_scales(dtype, n, V)
    kd = torch.from_numpy(kb).to(DEV)
    for W in (1, 3, 8):
        bufs = [dev(t, mis) for t in ts[:W]]
        kw = dict(step=STEP, sub=SUB)
        q = bs.quantize(bufs[0], kd, V, SEED, e0=e0, **kw)
        wr = bs.quantize_i16_wire(bufs[0], kd, V, SEED, e0=e0, **kw)
        s32, _ = bs.quantize_reduce(bufs, V, SEED, kblk=kd, e0=e0, **kw)
        s16, fl, _ = bs.quantize_reduce_i16(bufs, V, SEED, kblk=kd, e0=e0, **kw)
        for s, sl in enumerate(bref.blocks(n, V)):
            k, e = bref.keff(kb[s]), e0 + s * V
            part = [b[sl] for b in bufs]
            assert torch.equal(q[sl], sr.quantize(part[0], k, SEED, e0=e, **kw)), (W, s)
            assert torch.equal(wr[sl], sr.quantize_i16_wire(part[0], k, SEED, e0=e, **kw)), (W, s)
            assert torch.equal(s32[sl], sr.quantize_reduce(part, k, SEED, e0=e, **kw)), (W, s)
            o, f = sr.quantize_reduce_i16(part, k, V, SEED, e0=e, **kw)
            assert torch.equal(s16[sl], o) and f.numel() == 1 and int(f[0]) == int(fl[s]), (W, s)


# ---- consequence 2: composition -----------------------------------------------------------------------
@pytest.mark.parametrize("V", [32, 12])
@pytest.mark.parametrize("dtype", DTYPES)
def test_composition(dtype, V):
    bs, _, _, ops, _ = _mods()
    n = 1029
    ts, _ = buckets(dtype, n, V)
    kb = torch.from_numpy(given_scales(dtype, n, V)).to(DEV)
    for W in (2, 3, 8, 16):
        bufs = [dev(t) for t in ts[:W]]
        kw = dict(step=STEP, e0=E0)
        s32, _ = bs.quantize_reduce(bufs, V, SEED, kblk=kb, sub=SUB, **kw)
        parts = [bs.quantize(b, kb, V, SEED, sub=(SUB + w) & 0xFFFFFFFF, **kw) for w, b in enumerate(bufs)]
        assert torch.equal(s32, ops.sum_reduce(parts)), W
        s16, fl, _ = bs.quantize_reduce_i16(bufs, V, SEED, kblk=kb, sub=SUB, **kw)
        acc, flags = np.zeros(n, np.int64), np.zeros(-(-n // V), np.uint8)
        for w, b in enumerate(bufs):
            o, f, _ = bs.quantize_reduce_i16([b], V, SEED, kblk=kb, sub=(SUB + w) & 0xFFFFFFFF, **kw)
            acc += host(o).astype(np.int64)
            flags |= host(f)
        out = np.clip(acc, -32768, 32767)
        flags |= np.maximum.reduceat((out != acc).astype(np.uint8), np.arange(0, n, V))
        same(host(s16), out.astype(np.int16), f"composition i16 W={W}")
        same(host(fl), flags, f"composition flags W={W}")


# ---- consequence 3: integers and slices ------------------------------------------------------------------
@pytest.mark.parametrize("V", [32, 12])
@pytest.mark.parametrize("dtype", DTYPES)
def test_integers_give_the_nearest_siblings_results(dtype, V):
    bs, blk, _, _, wire = _mods()
    rng = np.random.default_rng(V)
    W, n = 4, 1029
    nblk = -(-n // V)
    kb = rng.integers(-6, 7, nblk).astype(np.int8)
    ints = rng.integers(-120, 121, (W, n)).astype(F32)        # 8 bits: exact in bf16 and fp16 at every scale here
    ints[0, 7], ints[1, n - 2] = 2.0 ** 16, -(2.0 ** 17)        # saturate int16, still integers
    kb[7 // V], kb[(n - 2) // V] = 7, 7                         # (512 and -1024 as values: within fp16's range)
    x = ints * np.ldexp(F32(1), -np.repeat(kb.astype(np.int32), V)[:n]).astype(F32)
    bufs = [dev(torch.from_numpy(r).to(dtype)) for r in x]
    assert all(np.array_equal(host(b.float()), r) for b, r in zip(bufs, x))        # the dtype holds them exactly
    kd = torch.from_numpy(kb).to(DEV)
    want_q, want_w = blk.quantize(bufs[0], kd, V), wire.quantize_blk(bufs[0], kd, V)
    want32, _ = blk.quantize_reduce(bufs, V, kblk=kd)
    want16, wantf, _ = blk.quantize_reduce_i16(bufs, V, kblk=kd)
    assert int(wantf.sum()) >= 2
    for seed in (0, 1, SEED, (1 << 64) - 1):
        kw = dict(step=seed & 0xFFFF, sub=3, e0=64)
        assert torch.equal(bs.quantize(bufs[0], kd, V, seed, **kw), want_q)
        assert torch.equal(bs.quantize_i16_wire(bufs[0], kd, V, seed, **kw), want_w)
        assert torch.equal(bs.quantize_reduce(bufs, V, seed, kblk=kd, **kw)[0], want32)
        o, f, _ = bs.quantize_reduce_i16(bufs, V, seed, kblk=kd, **kw)
        assert torch.equal(o, want16) and torch.equal(f, wantf)


@pytest.mark.parametrize("V", [32, 12])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_slice_with_e0_lo_is_that_slice_of_the_bucket(dtype, V):
    bs, _, _, _, _ = _mods()
    n, W = 1029, 3
    lo, hi = 2 * V, 1029 - 40                                    # lo a multiple of V and of 4
    assert lo % 4 == 0
    ts, _ = buckets(dtype, n, V)
    kd = torch.from_numpy(given_scales(dtype, n, V)).to(DEV)
    bufs = [dev(t) for t in ts[:W]]
    kw = dict(step=STEP, sub=SUB)
    whole32, _ = bs.quantize_reduce(bufs, V, SEED, kblk=kd, e0=E0, **kw)
    whole16, wholef, _ = bs.quantize_reduce_i16(bufs, V, SEED, kblk=kd, e0=E0, **kw)
    whole_w = bs.quantize_i16_wire(bufs[1], kd, V, SEED, e0=E0, **kw)
    part = [b[lo:hi] for b in bufs]
    ks = kd[lo // V:]
    assert torch.equal(bs.quantize_reduce(part, V, SEED, kblk=ks, e0=E0 + lo, **kw)[0], whole32[lo:hi])
    o, f, _ = bs.quantize_reduce_i16(part, V, SEED, kblk=ks, e0=E0 + lo, **kw)
    assert torch.equal(o, whole16[lo:hi])
    nb = -(-(hi - lo) // V)
    assert torch.equal(f[: nb - 1], wholef[lo // V: lo // V + nb - 1])          # (the slice's last block is cut short)
    assert torch.equal(bs.quantize_i16_wire(part[1], ks, V, SEED, e0=E0 + lo, **kw), whole_w[lo:hi])


# ---- consequence 4: the two layouts of a sharded step give the same bits --------------------------------------
@pytest.mark.parametrize("wire_name", ["i32", "i16"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layouts_agree(dtype, wire_name):
    bs, _, _, ops, _ = _mods()
    n, V, world, step = 1029, 32, 4, 9
    lo, hi = 8 * V, n                                            # a rank's range, the bucket's short end in it
    ts, _ = buckets(dtype, n, V)
    ranks = [dev(t) for t in ts[:world]]
    bits = 32 if wire_name == "i32" else 16
    # layout A: every rank's scales for `world` summands, their MIN, the rank's quantise on stream r, the SUM
    ks = torch.stack([bs.block_scales([x], V, bits=bits, degree=world) for x in ranks])
    kmin = ks.min(dim=0).values.contiguous()
    fn = bs.quantize if wire_name == "i32" else bs.quantize_i16_wire
    total = ops.sum_reduce([fn(x, kmin, V, SEED, step=step, sub=r) for r, x in enumerate(ranks)])
    # layout B: the AUTO reduce over all ranks' slices of [lo, hi)
    slices = [x[lo:hi] for x in ranks]
    kw = dict(degree=world, step=step, sub=0, e0=lo)
    if wire_name == "i32":
        out, kb = bs.quantize_reduce(slices, V, SEED, **kw)
        assert torch.equal(out, total[lo:hi])
    else:
        out, fl, kb = bs.quantize_reduce_i16(slices, V, SEED, **kw)
        o16, _, fa = ops.i16_wire_finish_blk(total, kmin, V, want_y=False)
        assert torch.equal(out, o16[lo:hi]) and torch.equal(fl, fa[lo // V:])
        assert int(fa.sum()) >= 1                                 # NaN / inf raised flags in both layouts
    assert torch.equal(kb, kmin[lo // V:])


# ---- bias -----------------------------------------------------------------------------------------------------
BIAS_SEED = 5
BIAS_N, BIAS_V, BIAS_W = 65_536, 32, 8


def bias_case():
    """x with t = 0.3f exactly under every block's own scale: (x [n] float32, kblk [n / V] int8)."""
    rng = np.random.default_rng(20261)
    kb = rng.integers(-20, 21, BIAS_N // BIAS_V).astype(np.int8)
    x = (F32(0.3) * np.ldexp(F32(1), -np.repeat(kb.astype(np.int32), BIAS_V))).astype(F32)
    return x, kb


def test_bias_of_the_eight_way_sum():
    """W = 8 summands of t = 0.3f each: the mean over 65,536 elements of (sum - 8 * 0.3f) must lie within 3
    standard errors of 0, one standard error being sqrt(8 * 0.21 / n) = 0.00506.  The seed was picked on
    the CPU from the replay, before any device run: BIAS_SEED = 5 gives a replay mean of +0.000482
    (+0.10 standard errors; seeds 1 to 7 all lie within 0.9).  Round to nearest sends every summand to 0: a mean of -2.4, 474 standard
    errors away."""
    bs, blk, _, _, _ = _mods()
    x, kb = bias_case()
    kd = torch.from_numpy(kb).to(DEV)
    bufs = [dev(x) for _ in range(BIAS_W)]
    exact = BIAS_W * float(F32(0.3))
    se = np.sqrt(BIAS_W * 0.21 / BIAS_N)
    got, _ = bs.quantize_reduce(bufs, BIAS_V, BIAS_SEED, kblk=kd)
    mean = float(host(got).astype(np.float64).mean()) - exact
    print(f"stochastic: mean error {mean:+.6f} = {mean / se:+.2f} standard errors")
    same(host(got), bsr.quantize_reduce([x] * BIAS_W, kb, BIAS_V, BIAS_SEED), "bias replay")
    assert abs(mean) < 3 * se
    near, _ = blk.quantize_reduce(bufs, BIAS_V, kblk=kd)
    mean_near = float(host(near).astype(np.float64).mean()) - exact
    print(f"nearest: mean error {mean_near:+.6f} = {mean_near / se:+.2f} standard errors")
    assert abs(mean_near) > 100 * se


# ---- what it buys ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [32, 256])
def test_int16_sixteen_way_sum_keeps_every_block_within_a_quantum_per_summand(V):
    """The log-uniform 96-block bucket at W = 16 on the int16 AUTO reduce: no flag, and every decoded value
    strictly within W * 2^-kblk[s] of the float64 sum -- each summand moves by less than one quantum and the
    decode is exact."""
    bs, blk, _, _, _ = _mods()
    rng = np.random.default_rng(20260)
    W, nblk = 16, 96
    n = nblk * V
    x = bref.bucket(rng, W, n, V)
    out, flags, kb = bs.quantize_reduce_i16([dev(r) for r in x], V, SEED, step=1)
    same(host(kb), bsr.kblk_ref(x, V, W, 16), "scales")
    assert not host(flags).any()
    y = host(blk.dequantize(out, kb, V)).astype(np.float64)
    exact = x.astype(np.float64).sum(0)
    quantum = np.ldexp(1.0, -np.repeat(host(kb).astype(np.int64), V))
    assert (np.abs(y - exact) < W * quantum).all()
    assert (host(out).reshape(nblk, V) != 0).any(axis=1).all()        # no block sums to zero
