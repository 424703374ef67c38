"""Error feedback on the 8-bit wire on the device (include/ina_i8_ef.h, ina_amd.i8, dist.ByteWireAggregator) against
tests/_i8_ef_ref.py, bit for bit: scales, bytes, flags and the residual carried back through the rotation."""
import numpy as np
import pytest
import torch

from tests import _i8_ef_ref as eref
from tests._i8_rank import bucket as rank_bucket
from tests.test_gpu_i8 import buckets
from tests.test_gpu_rot import DEV, DTYPES, E0, F32, SEED, STEP, SUB, _need_gpu, dev, grid_cap, host  # noqa: F401

pytestmark = pytest.mark.gpu
ref, PAD = eref.ref, 0x5A5A5A5A
ROT = pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
DT = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)  # noqa: E731


def check_replay(ts, xs, V, rotate, e0=0, caps=(None,), big=(3,)):
    """From the residuals a first replay step leaves: the scales over the 3 pairs (over 2: the MIN of the single
    pairs'), and pair 0's bytes, flags and residual under scales of which one is read as -126 and those of `big` are
    8 too large (block 3 clamps and carries the clipped part), equal the replay (returned); no -128, nothing past n.
    With a zero residual, scales, bytes and flags are the plain calls'."""
    from ina_amd import i8
    key, zero, n = dict(step=STEP, sub=SUB, e0=e0), np.zeros(xs[0].size, F32), xs[0].size
    kb0 = eref.block_scales(xs, [zero] * 3, V, rotate, **key)
    res = [eref.quantize(x, zero, kb0, V, rotate, **{**key, "step": STEP - 1})[2] for x in xs]
    want_kb = eref.block_scales(xs, res, V, rotate, **key)
    given = want_kb.copy()
    given[1], given[list(big)] = -128, np.minimum(given[list(big)].astype(int) + 8, 127)
    want = eref.quantize(xs[0], res[0], given, V, rotate, **key)
    assert want[1][3] == 1 and np.abs(want[2][3 * V:4 * V]).max() > 2.0 ** -int(given[3])
    bufs, rbufs = [dev(t) for t in ts], [dev(r) for r in res]
    singles = [i8.block_scales_ef([b], [r], V, rotate, **key) for b, r in zip(bufs[:2], rbufs)]
    assert torch.equal(i8.block_scales_ef(bufs[:2], rbufs[:2], V, rotate, **key), torch.minimum(*singles))
    z = torch.zeros(n, device=DEV)                       # a zero residual: the plain calls, compared on the device
    assert torch.equal(i8.block_scales_ef(bufs, [z] * 3, V, rotate, **key), i8.block_scales(bufs, V, rotate, **key))
    for got, plain in zip(i8.quantize_ef(bufs[0], z, dev(given), V, rotate, **key), i8.quantize(bufs[0], dev(given), V, rotate, **key)):
        assert torch.equal(got, plain) and z.any()
    for cap in caps:
        guarded = torch.cat([dev(res[0]), dev(np.full(64, PAD, np.uint32).view(F32))])
        with grid_cap(cap):
            kb = i8.block_scales_ef(bufs, rbufs, V, rotate, **key)
            q, f = i8.quantize_ef(bufs[0], guarded[:n], dev(given), V, rotate, **key)
        assert np.array_equal(host(kb), want_kb) and np.array_equal(host(f), want[1]), cap
        assert np.array_equal(host(q), want[0]) and host(q).min() >= -127, cap
        assert np.array_equal(bits(host(guarded)[:n]), bits(want[2])) and (bits(host(guarded)[n:]) == PAD).all(), cap
    return want


@pytest.mark.parametrize("nblk", (37, 1061))           # a partial wave at V = 8; several passes of a capped grid
@DT
@ROT
@pytest.mark.parametrize("V", (8, 16, 32, 64, 128, 256))
def test_replay_bit_for_bit(V, rotate, dtype, nblk):
    e0 = E0 if (dtype, nblk) == (torch.float32, 37) else 0
    check_replay(*buckets(dtype, nblk * V, V), V, rotate, e0, caps=(None, 1) if nblk == 1061 else (None,))


@ROT
def test_nan_inf_and_overflow_heal(rotate):
    """A NaN in block 0, an inf in block 2, 3e38 in block 4 under a scale 8 too large (the inverse butterfly overflows
    on its d): zero residuals where the contract says so, every other block as without them."""
    V, n = 32, 37 * 32
    clean = buckets(torch.float32, n, V)[1]
    xs = [x.copy() for x in clean]
    xs[0][3], xs[0][2 * V + 5], xs[0][4 * V + 9] = np.nan, np.inf, 3e38
    q, _, r1, u = check_replay([torch.from_numpy(x) for x in xs], xs, V, rotate, big=(3, 4))
    q0, _, r0, _ = check_replay([torch.from_numpy(x) for x in clean], clean, V, rotate, big=(3, 4))
    blk = np.arange(n) // V
    if rotate is None:
        assert not r1[[3, 2 * V + 5]].any() and r1[:V].any() and r1[2 * V:3 * V].any() and r1[4 * V + 9] > 1e38
    else:
        assert not r1[blk == 0].any() and not r1[blk == 2].any()
        assert not np.isfinite(u[blk == 4]).all() and not r1[(blk == 4) & ~np.isfinite(u)].any()
    keep = ~np.isin(blk, (0, 2, 4))
    assert np.array_equal(q[keep], q0[keep]) and np.array_equal(bits(r1[keep]), bits(r0[keep]))


@ROT
@pytest.mark.parametrize("V", (8, 256))
def test_the_sum_is_kept(V, rotate):
    """T = 16 steps of one bucket: the mean decode is off by resid_T / T, at worst sqrt(3) one-step rms errors over T,
    about 0.11 (the replay alone: 0.045-0.078); asked: a quarter.  The sum: 2m + 4 roundings of 2^-24 a step."""
    from ina_amd import blk, i8, rot
    T, key = 16, dict(step=STEP, sub=SUB)
    x64 = ref.rref.bref.bucket(np.random.default_rng(V), 1, 37 * V, V, lo=-4.0, hi=2.0)[0].astype(np.float64)
    x, res, xhats = dev(x64.astype(F32)), torch.zeros(37 * V, device=DEV), []
    for _ in range(T):
        kb = i8.block_scales_ef([x], [res], V, rotate, **key)
        s16 = i8.sum_slices([i8.quantize_ef(x, res, kb, V, rotate, **key)[0]])
        xhats.append(host(rot.dequantize(s16, kb, V, rotate, **key) if rotate else blk.dequantize(s16, kb, V)).astype(np.float64))
    mean_err, one_err = np.linalg.norm(np.mean(xhats, axis=0) - x64), np.linalg.norm(xhats[0] - x64)
    assert mean_err <= 0.25 * one_err
    assert np.linalg.norm(np.sum(xhats, axis=0) + host(res) - T * x64) <= 1e-5 * T * np.linalg.norm(x64)


@pytest.mark.parametrize("rotate", (False, True), ids=("plain", "rot"))
def test_aggregator_on_one_rank(rotate):
    """Three calls against the chained replay; gather="i8": the same residuals; reset_residual(): no error feedback."""
    from ina_amd.dist import ByteWireAggregator
    n, V, seed = 4_000 if rotate else 4_001, 32, SEED if rotate else None    # the plain wire takes a ragged block
    make = lambda **kw: ByteWireAggregator(n, V=V, device=torch.device(DEV), rotate=rotate, seed=SEED, **kw)  # noqa: E731
    agg, agg8, plain = make(error_feedback=True), make(error_feedback=True, gather="i8"), make()
    agg.step = agg8.step = STEP
    res = np.zeros(-(-n // V) * V, F32)
    for t in range(3):
        x = rank_bucket(t, n)
        xp = np.concatenate([x, np.zeros(-n % V, F32)])
        kb = eref.block_scales([xp], [res], V, seed, step=STEP + t)
        q, f, res, _ = eref.quantize(xp, res, kb, V, seed, step=STEP + t)
        full, _ = host(agg(dev(x))), agg8(dev(x))
        assert np.array_equal(full, ref.dequantize(ref.sum_slices([q]), kb, V, seed, step=STEP + t)[:n]), t
        assert np.array_equal(host(agg.kblk), kb) and np.array_equal(host(agg.local_overflow), f), t
        assert np.array_equal(bits(host(agg.residual)), bits(res[:n])) and torch.equal(agg8.residual, agg.residual), t
    assert agg.step == STEP + 3 and res.any()
    agg.reset_residual()
    agg.step = plain.step = STEP
    assert torch.equal(agg(dev(x)), plain(dev(x))) and torch.equal(agg.kblk, plain.kblk) and torch.equal(agg.q8, plain.q8)
