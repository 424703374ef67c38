"""Stochastic rounding in the fused quantise + reduce calls on the device (include/ina_reduce_sr.h,
sr.quantize_reduce / sr.quantize_reduce_i16, dist.StochasticRangeAggregator).

Replay: every sum and flag is bit for bit tests/_sr_reduce_ref.py -- the numpy replay of ina_sr.h per
worker on stream sub + w, the oracle's wrapping sum or one int16 clamp -- whatever the dtype, the worker
count (every specialisation and the run-time loop), the size, the alignment, the slot size or the grid.
Saturation: a summand alone, the sum alone, neither.  Streams wrap at 2^32.  Integers: the nearest
sibling's result for every seed.  Slices: e0 = lo.  Composition: the device's own sr.quantize* and
reduces.  Bias: the mean error of the 8-way sum is within 4 standard errors of 0 where nearest is 2.4
off.  The aggregator on one rank follows the replay over steps."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _sr_reduce_ref as rref
from tests import _sr_ref as sref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WS = (1, 2, 3, 4, 8, 16, 17)          # int32: 2, 4, 8, 16 specialised; int16: 1, 4, 8, 16; 3 and 17 the loop
SIZES = (1, 5, 511, 512, 513, 4099)   # a chunk's tail, a wave's region of 512 short, whole and one over, several blocks
VS = (8, 32, 256, 12)                 # 12: no ballot layout, the value-by-value path
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
K, CLIP16 = 9, 17                     # 0.3 * 2^17 is past int16: most summands clip, some do not
SEED = 0x1234
GUARD = 16
F32 = np.float32
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -3e-42, -1e-30, 0.0, 7.0, -7.5], F32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _mods():
    from ina_amd import ops, sr
    return sr, ops


def workers(seed, W, n, dtype, specials=True):
    """W seeded buckets as (CPU tensors of dtype, their exact float32 widenings); with specials, NaN,
    +-inf, -0.0, subnormals and integers sit in the first two workers, as many as n holds."""
    ts, xs = [], []
    for w in range(W):
        rng = np.random.default_rng(1000 * seed + w)
        x = (rng.standard_normal(n) * 0.3).astype(F32)
        if specials and w < 2:
            sp = rng.permutation(SPECIALS)[: min(n, SPECIALS.size)]
            x[rng.choice(n, size=sp.size, replace=False)] = sp
        t = torch.from_numpy(x).to(dtype)
        ts.append(t)
        xs.append(t.float().numpy())
    return ts, xs


def dev(t, off=0):
    """t on the device; off = 1: one element into its allocation (the unaligned path)."""
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t)
    return buf[off:]


class Guarded:
    """An output of n elements `off` elements into a buffer of sentinels, GUARD of them on each side."""

    def __init__(self, n, dtype, off=0, fill=0x5A):
        self.buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=dtype, device=DEV)
        self.fill, self.lo, self.hi = fill, GUARD + off, GUARD + off + n
        self.t = self.buf[self.lo:self.hi]

    def check(self, what):
        h = self.buf.cpu().numpy()
        assert (h[: self.lo] == self.fill).all() and (h[self.hi:] == self.fill).all(), what
        return h[self.lo:self.hi]


I16_CASES = [(K, V) for V in VS] + [(CLIP16, 8), (CLIP16, 12)]
_WANT = {}                             # the replay of a bucket set, computed once for both alignments


def want_all(bseed, dtype, W, n, xs, **kw):
    """The replay of workers(bseed, W, n, dtype)'s buckets xs under kw, cached under all of these."""
    key = (bseed, dtype, W, n, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = ([rref.quantize_reduce(xs, K, SEED, **kw)] +
                      [rref.quantize_reduce_i16(xs, k, V, SEED, **kw) for k, V in I16_CASES])
    return _WANT[key]


def run_all(sr, bufs, n, off, **kw):
    g = Guarded(n, torch.int32, off)
    sr.quantize_reduce(bufs, K, SEED, out=g.t, **kw)
    res = [g.check("i32")]
    for k, V in I16_CASES:
        g, f = Guarded(n, torch.int16, off), Guarded(-(-n // V), torch.uint8, 0)
        sr.quantize_reduce_i16(bufs, k, V, SEED, out=g.t, overflow=f.t, **kw)
        res.append((g.check(("i16", k, V)), f.check(("flags", k, V))))
    return res


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, tuple):
            assert g[0].dtype == w[0].dtype and np.array_equal(g[0], w[0]), (what, i, "sums")
            assert np.array_equal(g[1], w[1]), (what, i, "flags")
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, i)


# ---- replay ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_replay(dtype, off):
    sr, _ = _mods()
    clipped = flagged = clean = 0
    for W in WS:
        for n in SIZES:
            ts, xs = workers(n + W, W, n, dtype)
            kw = dict(step=3, sub=n)
            got = run_all(sr, [dev(t, off) for t in ts], n, off, **kw)
            want = want_all(n + W, dtype, W, n, xs, **kw)
            assert_same(got, want, (W, n))
            clipped += int((np.abs(want[5][0].astype(np.int64)) >= 32767).sum())
            flagged += int(want[2][1].sum())
            clean += int((want[2][1] == 0).sum())
    assert clipped and flagged and clean       # the clipping k clipped; NaN / inf raised flags; most slots raised none


def test_replay_at_the_worker_limit():
    sr, _ = _mods()
    n, W = 513, 64
    ts, xs = workers(64, W, n, torch.float32)
    kw = dict(step=1, sub=7)
    assert_same(run_all(sr, [dev(t) for t in ts], n, 0, **kw), want_all(64, torch.float32, W, n, xs, **kw), W)


def test_replay_is_of_every_worker_stream_and_is_not_nearest():
    """The yardstick moves with seed, step and sub, gives two workers with equal buckets different
    roundings, and is not round-to-nearest: a kernel that dropped one of these would not pass above."""
    n = 4099
    _, xs = workers(1, 2, n, torch.float32, specials=False)
    a = rref.quantize_reduce(xs, K, SEED, step=3, sub=5)
    for seed, kw in ((SEED + 1, dict(step=3, sub=5)), (SEED, dict(step=4, sub=5)), (SEED, dict(step=3, sub=6))):
        assert (rref.quantize_reduce(xs, K, seed, **kw) != a).mean() > 0.2
    assert (orc.sum_reduce_i32([orc.quantize_i32(x, K) for x in xs]) != a).mean() > 0.2
    same = rref.quantize_reduce([xs[0], xs[0]], K, SEED)
    assert (same != 2 * sref.quantize(xs[0], K, SEED)).mean() > 0.2


def test_grid_stride_under_a_capped_grid():
    sr, ops = _mods()
    n = 4099
    for dtype in DTYPES:
        for W in (2, 3, 8):
            ts, xs = workers(77, W, n, dtype)
            want = want_all(77, dtype, W, n, xs, step=1, sub=2)
            bufs = [dev(t) for t in ts]
            try:
                ops.set_tuning(max_blocks=2)
                got = run_all(sr, bufs, n, 0, step=1, sub=2)
            finally:
                ops.set_tuning(max_blocks=16384)
            assert_same(got, want, (dtype, W))


# ---- saturation, specials, stream wrap -------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_saturation_of_a_summand_of_the_sum_and_of_neither(dtype):
    """Slot 0: one summand past int16, the others pull the sum back inside.  Slot 1: eight summands near
    5000, none saturated, the sum past int16.  Slot 2: nothing."""
    sr, _ = _mods()
    W, V, n, k = 8, 32, 96, 0
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((W, n)) * 3).astype(F32)
    x[:, 5] = F32(-5000.25)
    x[0, 5] = F32(40000.5)
    x[:, 32:64] = F32(5000.25) + x[:, 32:64]
    ts = [torch.from_numpy(r).to(dtype) for r in x]
    xs = [t.float().numpy() for t in ts]
    want, wflags = rref.quantize_reduce_i16(xs, k, V, SEED, step=2)
    assert list(wflags) == [1, 1, 0] and -32768 < want[5] < 32767 and (want[32:64] == 32767).all()
    for off in (0, 1):
        got, flags = sr.quantize_reduce_i16([dev(t, off) for t in ts], k, V, SEED, step=2)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(flags.cpu().numpy(), wflags), off


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_inf_and_subnormals(dtype):
    sr, _ = _mods()
    W, V, n = 3, 8, 64
    x = np.zeros((W, n), F32)
    x[0, :10] = SPECIALS                       # one special a column, the other workers finite
    x[1, 16:26] = SPECIALS
    x[2, 16] = F32(np.nan)                     # NaN + NaN
    x[2, 17] = F32(-np.inf)                    # +inf + -inf: both saturate, the sum is -1
    x[1:, 40:48] = F32(0.3) * F32(2.0 ** -K)
    ts = [torch.from_numpy(r).to(dtype) for r in x]
    xs = [t.float().numpy() for t in ts]
    bufs = [dev(t) for t in ts]
    want = rref.quantize_reduce(xs, K, SEED)
    assert np.array_equal(sr.quantize_reduce(bufs, K, SEED).cpu().numpy(), want)
    assert want[0] == 0 and want[1] == np.iinfo(np.int32).max and want[2] == np.iinfo(np.int32).min
    w16, wf = rref.quantize_reduce_i16(xs, K, V, SEED)
    got, flags = sr.quantize_reduce_i16(bufs, K, V, SEED)
    assert np.array_equal(got.cpu().numpy(), w16) and np.array_equal(flags.cpu().numpy(), wf)
    assert w16[17] == -1 and list(wf[:6]) == [1, 0, 1, 0, 0, 0]


def test_the_worker_stream_wraps_at_2_to_the_32():
    sr, _ = _mods()
    n, top = 4099, (1 << 32) - 1
    ts, xs = workers(9, 2, n, torch.float32, specials=False)
    bufs = [dev(t) for t in ts]
    got = sr.quantize_reduce(bufs, K, SEED, sub=top).cpu().numpy()
    assert np.array_equal(got, rref.quantize_reduce(xs, K, SEED, sub=top))
    parts = sr.quantize(bufs[0], K, SEED, sub=top).cpu().numpy() + sr.quantize(bufs[1], K, SEED, sub=0).cpu().numpy()
    assert np.array_equal(got, parts)          # worker 1 rounds on stream 0


# ---- integers, slices, composition -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_t_equals_the_nearest_sibling_for_every_seed(dtype):
    sr, ops = _mods()
    n, V, W = 4099, 32, 4
    rng = np.random.default_rng(11)
    bufs = []
    for w in range(W):
        m = rng.integers(-256, 257, n).astype(F32)                       # exact in bf16 and fp16 as well
        m[rng.choice(n, 40, replace=False)] = F32(40960.0) * rng.choice([-1, 1], 40).astype(F32)   # past int16
        t = torch.from_numpy(m * F32(2.0 ** -K)).to(dtype)
        assert np.array_equal(t.float().numpy() * F32(2.0 ** K), m)
        bufs.append(dev(t))
    near = ops.quantize_reduce(bufs, K).cpu().numpy()
    near_h, near_f = (a.cpu().numpy() for a in ops.quantize_reduce_i16(bufs, K, V))
    assert near_f.any() and not near_f.all()
    for seed in (0, SEED, (1 << 64) - 1):
        assert np.array_equal(sr.quantize_reduce(bufs, K, seed, step=seed & 7).cpu().numpy(), near)
        h, f = sr.quantize_reduce_i16(bufs, K, V, seed, sub=3)
        assert np.array_equal(h.cpu().numpy(), near_h) and np.array_equal(f.cpu().numpy(), near_f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_slice_with_its_offset_is_the_slice_of_the_whole(dtype):
    sr, _ = _mods()
    n, lo, hi, V, W = 4099, 1024, 3000, 8, 3
    ts, xs = workers(5, W, n, dtype)
    bufs = [dev(t) for t in ts]
    kw = dict(step=2, sub=1)
    whole = sr.quantize_reduce(bufs, K, SEED, **kw).cpu().numpy()
    whole_h, whole_f = (a.cpu().numpy() for a in sr.quantize_reduce_i16(bufs, K, V, SEED, **kw))
    assert np.array_equal(whole, rref.quantize_reduce(xs, K, SEED, **kw))
    part = [b[lo:hi] for b in bufs]
    got = sr.quantize_reduce(part, K, SEED, e0=lo, **kw).cpu().numpy()
    got_h, got_f = (a.cpu().numpy() for a in sr.quantize_reduce_i16(part, K, V, SEED, e0=lo, **kw))
    assert np.array_equal(got, whole[lo:hi])
    assert np.array_equal(got_h, whole_h[lo:hi]) and np.array_equal(got_f, whole_f[lo // V:hi // V])
    assert not np.array_equal(sr.quantize_reduce(part, K, SEED, **kw).cpu().numpy(), got)       # e0 matters


@pytest.mark.parametrize("dtype", DTYPES)
def test_composition_of_the_device_quantisers_and_reduces(dtype):
    sr, ops = _mods()
    n, V = 4099, 32
    for W, k in ((2, K), (5, K), (8, CLIP16)):
        ts, _ = workers(21, W, n, dtype)
        bufs = [dev(t) for t in ts]
        kw = dict(step=6, e0=2048)
        qs = [sr.quantize(b, k, SEED, sub=40 + w, **kw) for w, b in enumerate(bufs)]
        assert torch.equal(sr.quantize_reduce(bufs, k, SEED, sub=40, **kw), ops.sum_reduce(qs))
        hs = [sr.quantize_i16(b, k, V, SEED, sub=40 + w, **kw) for w, b in enumerate(bufs)]
        s16, f = ops.sum_reduce_i16([h for h, _ in hs], V)
        for _, fw in hs:
            f = f | fw
        got, flags = sr.quantize_reduce_i16(bufs, k, V, SEED, sub=40, **kw)
        assert torch.equal(got, s16) and torch.equal(flags, f), (W, k)


def test_an_offset_that_splits_a_philox_call_is_refused_before_any_device_work():
    import ctypes
    from ina_amd import _lib
    sr, _ = _mods()
    x = torch.zeros(64, device=DEV)
    q = torch.full((64,), 77, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="e0 must be a multiple of 4"):
        sr.quantize_reduce([x, x], K, SEED, e0=2, out=q)
    prm = _lib.SrParams(SEED, 2, 0, 0)
    arr = _lib.ptr_array([x.data_ptr(), x.data_ptr()])
    rc = _lib.load().ina_quantize_reduce_sr_f32_i32(arr, 2, q.data_ptr(), 64, K, ctypes.byref(prm), None)
    assert rc == _lib.INA_EINVAL and b"e0 must be a multiple of 4" in _lib.load().ina_last_error_string()
    torch.cuda.synchronize()
    assert (q.cpu().numpy() == 77).all()


# ---- bias ------------------------------------------------------------------------------------------
BIAS_SEED = 3          # chosen on the CPU from the numpy replay alone: its mean error is inside the bound


def test_the_sum_is_unbiased_where_nearest_is_not():
    """W = 8 workers, every t = 0.3: the mean of sum - sum_w t_w is within 4 standard errors of 0 (a summand's
    variance is 0.3 * 0.7, so the standard error of the mean over n values is sqrt(8 * 0.21 / n)); to nearest
    every summand is 0 and the mean is -2.4."""
    sr, ops = _mods()
    W, n = 8, 65536
    xh = np.full(n, F32(0.3) * F32(2.0 ** -K), F32)
    meant = W * float(F32(0.3))
    se = np.sqrt(W * 0.21 / n)
    ref = rref.quantize_reduce([xh] * W, K, BIAS_SEED)
    assert abs(ref.mean() - meant) <= 4 * se                             # the yardstick itself
    bufs = [torch.from_numpy(xh).to(DEV) for _ in range(W)]
    got = sr.quantize_reduce(bufs, K, BIAS_SEED).cpu().numpy()
    err = got.astype(np.float64).mean() - meant
    print("mean error of the sum", err, "standard errors", err / se)
    assert np.array_equal(got, ref)
    assert abs(err) <= 4 * se
    near = ops.quantize_reduce(bufs, K).cpu().numpy().astype(np.float64).mean() - meant
    print("to nearest", near, "standard errors", near / se)
    assert abs(near) > 4 * se
    h, f = sr.quantize_reduce_i16(bufs, K, 256, BIAS_SEED)
    assert np.array_equal(h.cpu().numpy(), ref.astype(np.int16)) and not f.any().item()


# ---- the aggregator at world 1 ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("wire", ["i32", "i16"])
def test_aggregator_on_one_rank(wire, dtype):
    from ina_amd.dist import RangeAggregator, StochasticRangeAggregator
    n, V, k, T, W = 5003, 32, 6, 3, 3
    agg = StochasticRangeAggregator(n, k=k, device=torch.device(DEV), wire=wire, V=V, seed=SEED, out_dtype=dtype)
    assert isinstance(agg, RangeAggregator) and agg.range == (0, n) and agg.seed == SEED
    m = agg.hi - agg.lo
    sets = [workers(300 + t, W, m, dtype) for t in range(T)]

    def check(full, t, step):
        xs = sets[t][1]
        if wire == "i32":
            y = orc.dequantize_i32(rref.quantize_reduce(xs, k, SEED, step=step), k)
        else:
            s16, flags = rref.quantize_reduce_i16(xs, k, V, SEED, step=step)
            y = orc.dequantize_i16(s16, k)
            assert np.array_equal(agg.overflow.cpu().numpy(), flags) and flags.any()
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert full.dtype == dtype and full.numel() == n
        assert torch.equal(full.cpu().view(bits), torch.from_numpy(y).to(dtype).view(bits)), (t, step)

    for t in range(T):
        assert agg.step == t
        check(agg([dev(x) for x in sets[t][0]]), t, t)
    assert agg.step == T
    agg.aggregate_int([dev(x) for x in sets[0][0]])                      # a step like any other
    assert agg.step == T + 1
    agg.phase_reduce_decode([dev(x) for x in sets[0][0]])
    assert agg.step == T + 2
    agg.step = 1                                                         # a resumed job repeats step 1
    check(agg([dev(x) for x in sets[1][0]]), 1, 1)
    assert agg.step == 2
