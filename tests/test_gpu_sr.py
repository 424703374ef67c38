"""Stochastic rounding on the device (include/ina_sr.h, ina_amd.sr, dist.ShardedAggregator).

Replay: every q, flag and wire word is bit for bit tests/_sr_ref.py -- Philox4x32-10 and the contract's
float32 steps in numpy, the CPU oracle's clamps -- on the CPU-widened bucket, whatever the dtype, the
size, the alignment, the grid or the slot size.  Integers: where t is an integer the result is the
round-to-nearest sibling's for every seed.  Slices: x[lo:hi] with e0 = lo is that slice of the whole
bucket.  Streams: seed, step and sub each change about half of the roundings at t = 0.5.  Bias: the mean
of q is t within 5 sigma where nearest sends nothing, in one step and summed over 64."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _sr_ref as sref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 5, 255, 256, 257, 4099)
VS = (8, 32, 256, 12)                 # 12: no ballot layout, the value-by-value path
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
K = 9
CLIP32, CLIP16 = 33, 17               # 0.3 * 2^33 is past int32, 0.3 * 2^17 past int16: most values clip, some do not
SEED = 0x1234
GUARD = 16                            # elements on each side of an output
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _mods():
    from ina_amd import ops, sr, wire
    return sr, ops, wire


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -3e-42, -1e-30, 0.0, 7.0, -7.5], F32)


def bucket(seed, n, dtype):
    """(x as a CPU tensor of dtype, its exact float32 widening, a float32 base): seeded values with
    NaN, +-inf, -0.0, subnormals, a tiny negative (p rounds to 1) and integers among them, as many as
    n holds; the seed moves them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.3).astype(F32)
    sp = rng.permutation(SPECIALS)[: min(n, SPECIALS.size)]
    x[rng.choice(n, size=sp.size, replace=False)] = sp
    t = torch.from_numpy(x).to(dtype)
    base = (rng.standard_normal(n) * 0.3).astype(F32)
    return t, t.float().numpy(), base


def dev(t, off=0):
    """t on the device; off = 1: as a view one element into its allocation (the unaligned path)."""
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t)
    return buf[off:]


class Guarded:
    """An output of n elements `off` elements into a buffer filled with a sentinel, GUARD elements of
    it on each side: check() asserts nothing around the output was written."""

    def __init__(self, n, dtype, off=0, fill=0x5A):
        self.buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=dtype, device=DEV)
        self.fill, self.lo, self.hi = fill, GUARD + off, GUARD + off + n
        self.t = self.buf[self.lo:self.hi]

    def check(self, what):
        h = self.buf.cpu().numpy()
        assert (h[: self.lo] == self.fill).all() and (h[self.hi:] == self.fill).all(), what
        return h[self.lo:self.hi]


def run_all(sr, x, base, n, k32, k16, off, **kw):
    """The three calls on one bucket, outputs guarded: [q32, (q16, flags) per V, words]."""
    res = []
    g = Guarded(n, torch.int32, off)
    sr.quantize(x, k32, SEED, base=base, out=g.t, **kw)
    res.append(g.check("q32"))
    for V in VS:
        g, f = Guarded(n, torch.int16, off), Guarded(-(-n // V), torch.uint8, 0)
        sr.quantize_i16(x, k16, V, SEED, base=base, out=g.t, overflow=f.t, **kw)
        res.append((g.check(("q16", V)), f.check(("flags", V))))
    g = Guarded(n, torch.int32, off)
    sr.quantize_i16_wire(x, k16, SEED, out=g.t, **kw)
    res.append(g.check("wire"))
    return res


def want_all(xw, base, k32, k16, **kw):
    res = [sref.quantize(xw, k32, SEED, base=base, **kw)]
    res += [sref.quantize_i16(xw, k16, V, SEED, base=base, **kw) for V in VS]
    res.append(sref.quantize_i16_wire(xw, k16, SEED, **kw))
    return res


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, tuple):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), (what, i)
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, i)


# ---- replay ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_replay(dtype, off):
    sr, _, _ = _mods()
    clipped = flagged = 0
    for n in SIZES:
        t, xw, base = bucket(n, n, dtype)
        x = dev(t, off)
        for with_base in (False, True):
            b = base if with_base else None
            bd = dev(base, off) if with_base else None
            for k32, k16 in ((K, K), (CLIP32, CLIP16)):
                kw = dict(step=3, sub=n)
                got = run_all(sr, x, bd, n, k32, k16, off, **kw)
                want = want_all(xw, b, k32, k16, **kw)
                assert_same(got, want, (n, with_base, k32))
                clipped += int((want[0] == np.iinfo(np.int32).max).sum())
                flagged += int(want[2][1].sum())
    assert clipped and flagged                          # the clipping k clipped, NaN / inf raised flags


def test_replay_depends_on_every_field_and_is_not_nearest():
    """The replay is of this seed, step and sub (a kernel that ignored one would still pass above only
    if the reference did too), and differs from round-to-nearest."""
    n = 4099
    _, xw, _ = bucket(1, n, torch.float32)
    a = sref.quantize(xw, K, SEED, step=3, sub=5)
    for kw in (dict(seed=SEED + 1, step=3, sub=5), dict(seed=SEED, step=4, sub=5), dict(seed=SEED, step=3, sub=6),
               dict(seed=SEED + (1 << 32), step=3, sub=5)):
        assert (sref.quantize(xw, K, kw.pop("seed"), **kw) != a).mean() > 0.2
    assert (orc.quantize_i32(xw, K) != a).mean() > 0.2


def test_grid_stride_under_a_capped_grid():
    sr, ops, _ = _mods()
    n = 4099
    for dtype in DTYPES:
        t, xw, base = bucket(77, n, dtype)
        want = want_all(xw, base, K, K, step=1, sub=2)
        try:
            ops.set_tuning(max_blocks=2)
            got = run_all(sr, dev(t), dev(base), n, K, K, 0, step=1, sub=2)
        finally:
            ops.set_tuning(max_blocks=16384)
        assert_same(got, want, dtype)


# ---- slices ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_slice_with_its_offset_is_the_slice_of_the_whole(dtype):
    sr, _, _ = _mods()
    n, lo, hi, V = 4099, 1024, 3000, 8
    t, xw, base = bucket(5, n, dtype)
    x, b = dev(t), dev(base)
    kw = dict(step=2, sub=1)
    whole_q = sr.quantize(x, K, SEED, base=b, **kw).cpu().numpy()
    whole_h, whole_f = (a.cpu().numpy() for a in sr.quantize_i16(x, K, V, SEED, base=b, **kw))
    whole_w = sr.quantize_i16_wire(x, K, SEED, **kw).cpu().numpy()
    assert np.array_equal(whole_q, sref.quantize(xw, K, SEED, base=base, **kw))
    part_q = sr.quantize(x[lo:hi], K, SEED, base=b[lo:hi], e0=lo, **kw).cpu().numpy()
    part_h, part_f = (a.cpu().numpy() for a in sr.quantize_i16(x[lo:hi], K, V, SEED, base=b[lo:hi], e0=lo, **kw))
    part_w = sr.quantize_i16_wire(x[lo:hi], K, SEED, e0=lo, **kw).cpu().numpy()
    assert np.array_equal(part_q, whole_q[lo:hi]) and np.array_equal(part_w, whole_w[lo:hi])
    assert np.array_equal(part_h, whole_h[lo:hi]) and np.array_equal(part_f, whole_f[lo // V:hi // V])
    assert not np.array_equal(sr.quantize(x[lo:hi], K, SEED, base=b[lo:hi], **kw).cpu().numpy(), part_q)   # e0 matters


def test_an_offset_that_splits_a_philox_call_is_refused():
    sr, _, _ = _mods()
    from ina_amd import _lib
    x = torch.zeros(64, device=DEV)
    q = torch.full((64,), 77, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="e0 must be a multiple of 4"):
        sr.quantize(x, K, SEED, e0=2, out=q)
    prm = _lib.SrParams(SEED, 2, 0, 0)
    rc = _lib.load().ina_quantize_sr_f32_i32(x.data_ptr(), None, q.data_ptr(), 64, K, ctypes.byref(prm), None)
    assert rc == _lib.INA_EINVAL and b"e0 must be a multiple of 4" in _lib.load().ina_last_error_string()
    torch.cuda.synchronize()
    assert (q.cpu().numpy() == 77).all()                # refused before any device work


# ---- integers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_t_equals_the_nearest_sibling_for_every_seed(dtype):
    """m * 2^-k with integer m (within the dtype's exact integers, and past the int16 range): p = 0, so
    no word is ever looked at."""
    sr, ops, wire = _mods()
    n, V = 4099, 32
    rng = np.random.default_rng(11)
    m = rng.integers(-256, 257, n).astype(F32)                          # exact in bf16 and fp16 as well
    m[rng.choice(n, 40, replace=False)] = F32(40960.0) * rng.choice([-1, 1], 40).astype(F32)   # 5 * 2^13: past int16
    t = torch.from_numpy(m * F32(2.0 ** -K)).to(dtype)
    xw = t.float().numpy()
    assert np.array_equal(xw * F32(2.0 ** K), m)
    x = dev(t)
    near_q = ops.quantize(x, K).cpu().numpy()
    near_h, near_f = (a.cpu().numpy() for a in ops.quantize_i16(x, K, V))
    near_w = wire.quantize(x, K).cpu().numpy()
    assert np.array_equal(near_q, orc.quantize_i32(xw, K)) and near_f.any()
    for seed in (0, SEED, (1 << 64) - 1):
        assert np.array_equal(sr.quantize(x, K, seed, step=seed & 7).cpu().numpy(), near_q)
        h, f = sr.quantize_i16(x, K, V, seed, sub=3)
        assert np.array_equal(h.cpu().numpy(), near_h) and np.array_equal(f.cpu().numpy(), near_f)
        assert np.array_equal(sr.quantize_i16_wire(x, K, seed).cpu().numpy(), near_w)


# ---- streams, bias ---------------------------------------------------------------------------------
def test_seed_step_and_sub_each_move_about_half_of_the_roundings():
    sr, _, _ = _mods()
    n = 4096
    x = torch.full((n,), 0.5, device=DEV)
    a = sr.quantize(x, 0, SEED).cpu().numpy()
    assert set(np.unique(a)) == {0, 1}
    for kw in (dict(seed=SEED + 1), dict(seed=SEED, step=1), dict(seed=SEED, sub=1)):
        b = sr.quantize(x, 0, kw.pop("seed"), **kw).cpu().numpy()
        frac = float((a != b).mean())
        print("changed", kw, frac)
        assert 0.40 <= frac <= 0.60, (kw, frac)


def test_the_mean_is_unbiased_where_nearest_sends_nothing():
    sr, ops, _ = _mods()
    n = 65536
    xh = np.full(n, F32(0.3) * F32(2.0 ** -K), F32)
    x = torch.from_numpy(xh).to(DEV)
    q = sr.quantize(x, K, SEED).cpu().numpy()
    sigma = np.sqrt(0.21 / n)
    print("mean", q.mean(), "sigmas", (q.mean() - 0.3) / sigma)
    assert abs(q.mean() - 0.3) <= 5 * sigma
    assert np.array_equal(q, sref.quantize(xh, K, SEED))
    assert not ops.quantize(x, K).cpu().numpy().any()


def test_the_sum_over_steps_tracks_what_was_meant():
    sr, _, _ = _mods()
    n, T = 4096, 64
    x = torch.from_numpy(np.full(n, F32(0.3) * F32(2.0 ** -K), F32)).to(DEV)
    acc = torch.zeros(n, dtype=torch.int64, device=DEV)
    for t in range(T):
        acc += sr.quantize(x, K, SEED, step=t)
    mean = float(acc.double().mean().item())
    sigma = np.sqrt(T * 0.21 / n)
    print("mean of sums", mean, "sigmas", (mean - 19.2) / sigma)
    assert abs(mean - 0.3 * T) <= 5 * sigma


# ---- the aggregator at world 1 ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("wire", ["i32", "i16"])
def test_aggregator_on_one_rank(wire, dtype):
    from ina_amd.dist import ShardedAggregator
    n, V, k, T = 5003, 32, 6, 3
    agg = ShardedAggregator(n, k=k, device=torch.device(DEV), wire=wire, V=V, rounding="stochastic", seed=SEED,
                            out_dtype=dtype)
    buckets = [bucket(300 + t, n, dtype) for t in range(T)]

    def want(t, step):
        xw = buckets[t][1]
        if wire == "i32":
            return orc.dequantize_i32(sref.quantize(xw, k, SEED, step=step), k), None
        o16, y, flags = orc.i16_wire_finish(sref.quantize_i16_wire(xw, k, SEED, step=step), k, V)
        return y, flags

    def check(full, t, step):
        y, flags = want(t, step)
        assert full.dtype == dtype
        w = torch.from_numpy(y).to(dtype)                                # the fp32 aggregate rounded once
        assert torch.equal(full.cpu().view(torch.int16 if dtype != torch.float32 else torch.int32),
                           w.view(torch.int16 if dtype != torch.float32 else torch.int32)), (t, step)
        if flags is not None:
            assert np.array_equal(agg.overflow.cpu().numpy(), flags) and flags.any()

    for t in range(T):
        assert agg.step == t
        check(agg(dev(buckets[t][0])), t, t)
    assert agg.step == T
    agg.aggregate_int(dev(buckets[0][0]))                                # a step like any other
    assert agg.step == T + 1
    agg.step = 1                                                         # a resumed job repeats step 1
    check(agg(dev(buckets[1][0])), 1, 1)
    assert agg.step == 2
    # the default rounds to nearest, as before, and owns no moving counter
    near = ShardedAggregator(n, k=k, device=torch.device(DEV), wire=wire, V=V)
    full = near(dev(buckets[0][0]))
    xw = buckets[0][1]
    y = (orc.dequantize_i32(orc.quantize_i32(xw, k), k) if wire == "i32"
         else orc.i16_wire_finish(orc.quantize_i16_wire(xw, k), k, V)[1])
    assert np.array_equal(full.cpu().numpy().view(np.uint32), y.view(np.uint32)) and near.step == 0
