"""The randomised Hadamard rotation on the device (include/ina_rot.h, ina_amd.rot) against tests/_rot_ref.py:
the float32 replay bit for bit, the exact integer round trip against float64, what the rotation buys on the
int16 wire, and the PS combine against the composition of the calls it fuses."""
import contextlib

import numpy as np
import pytest
import torch

from tests import _rot_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
SEED, STEP, SUB = 0xC0FFEE123456789, 5, 0xFFFFFFFE
E0 = (1 << 34) + 768                                   # needs 64 bits; a multiple of 128 and of every V
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(DEV)


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """Bit for bit, a NaN matching any NaN (the contract leaves a NaN's sign and payload open)."""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@contextlib.contextmanager
def grid_cap(cap):
    """The default grid, or every launch capped at `cap` workgroups (several grid-stride passes)."""
    from ina_amd import ops
    if cap is not None:
        ops.set_tuning(max_blocks=cap)
    try:
        yield
    finally:
        ops.set_tuning(max_blocks=16384)


_BUCKETS = {}


def buckets(dtype, n, V):
    """9 seeded buckets as (tensors of dtype, their exact float32 widenings); block magnitudes log-uniform
    over six decades, so neighbouring blocks carry different scales."""
    if (dtype, n, V) not in _BUCKETS:
        x = ref.bref.bucket(np.random.default_rng(n * 1000 + V), 9, n, V, lo=-4.0, hi=2.0)
        ts = [torch.from_numpy(r).to(dtype) for r in x]
        _BUCKETS[dtype, n, V] = (ts, [t.float().numpy() for t in ts])
    return _BUCKETS[dtype, n, V]


def check_replay(ts, xs, V, e0, caps=(None,)):
    """q, flags and kblk of both fused calls under AUTO and GIVEN, and y of both decodes, equal the replay."""
    from ina_amd import rot
    key = dict(step=STEP, sub=SUB, e0=e0)
    bufs = [dev(t) for t in ts]
    for bits in (32, 16):
        auto = ref.quantize_reduce(xs, V, SEED, bits=bits, **key)
        given = auto[2].copy()
        given[1], given[3] = -128, min(int(given[3]) + 8, 127)       # read as -126; saturates int16
        wants = {None: auto, "given": ref.quantize_reduce(xs, V, SEED, kblk=given, bits=bits, **key)}
        for cap in caps:
            for mode, (q, flags, kblk) in wants.items():
                kb = None if mode is None else dev(given)
                with grid_cap(cap):
                    if bits == 32:
                        got_q, got_kb = rot.quantize_reduce(bufs, V, SEED, kblk=kb, **key)
                    else:
                        got_q, got_f, got_kb = rot.quantize_reduce_i16(bufs, V, SEED, kblk=kb, **key)
                        assert np.array_equal(host(got_f), flags), (bits, mode, cap)
                    y = rot.dequantize(got_q, got_kb, V, SEED, **key)
                assert np.array_equal(host(got_kb), kblk), (bits, mode, cap)
                assert np.array_equal(host(got_q), q), (bits, mode, cap)
                want_y = ref.dequantize(q, kblk, V, SEED, **key)
                assert same_bits(host(y), want_y), (bits, mode, cap)


@pytest.mark.parametrize("nblk", (37, 1061))           # a partial wave at V = 8; several passes of a capped grid
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("W", (1, 4, 9))               # held instances and the run-time loop
@pytest.mark.parametrize("V", (8, 32, 256))            # one cross-lane stage, three, all six
def test_replay_bit_for_bit(V, W, dtype, nblk):
    ts, xs = buckets(dtype, nblk * V, V)
    e0 = E0 if (V, W, nblk) == (32, 4, 37) else 0
    check_replay(ts[:W], xs[:W], V, e0, caps=(None, 1) if nblk == 1061 else (None,))


@pytest.mark.parametrize("W", (2, 8, 16))              # the other held instances; int16 at 16: the re-read one
def test_replay_every_instance(W):
    V, n = 256, 37 * 256
    xs = buckets(torch.float32, n, V)[1]
    xs = (xs + [x[::-1].copy() for x in xs])[:W]
    check_replay([torch.from_numpy(x) for x in xs], xs, V, 0)


def test_nan_and_inf_stay_in_their_blocks():
    """A NaN in block 0 and an inf in block 2: the replay's bits, flags for exactly those blocks, and every
    other block as without them."""
    from ina_amd import rot
    V, W, n = 32, 4, 37 * 32
    clean = [x.copy() for x in buckets(torch.float32, n, V)[1][:W]]
    xs = [x.copy() for x in clean]
    xs[0][3], xs[1][2 * V + 5] = np.nan, np.inf
    check_replay([torch.from_numpy(x) for x in xs], xs, V, 0)
    got = rot.quantize_reduce_i16([dev(x) for x in xs], V, SEED)
    base = rot.quantize_reduce_i16([dev(x) for x in clean], V, SEED)
    assert host(base[1]).sum() == 0 and np.flatnonzero(host(got[1])).tolist() == [0, 2]
    keep = np.ones(n, bool)
    keep[:V], keep[2 * V:3 * V] = False, False
    assert np.array_equal(host(got[0])[keep], host(base[0])[keep])
    assert np.array_equal(np.delete(host(got[2]), [0, 2]), np.delete(host(base[2]), [0, 2]))


@pytest.mark.parametrize("V", (8, 16, 32, 64, 128, 256))
def test_integers_round_trip_exactly(V):
    """Integer inputs, |x| <= 1000, W = 8, given k = ceil(m/2): every add is exact, so the int32 sum is
    H D sum(x) and the decode returns sum(x) bit for bit -- for every legal butterfly."""
    from ina_amd import rot
    W, n, k = 8, 37 * V, (V.bit_length()) // 2
    xs = np.random.default_rng(V).integers(-1000, 1001, (W, n)).astype(F32)
    kb = dev(np.full(n // V, k, np.int8))
    q, _ = rot.quantize_reduce([dev(x) for x in xs], V, SEED, kblk=kb, step=STEP)
    total = xs.astype(np.float64).sum(0)
    want = ref.forward(total, V, ref.signs(n, SEED, STEP), np.float64) * 2.0 ** k
    assert np.array_equal(host(q).astype(np.float64), want)
    assert np.array_equal(host(rot.dequantize(q, kb, V, SEED, step=STEP)), total.astype(F32))


def test_what_it_buys_on_the_int16_wire():
    """W = 16, int16, V = 256, AUTO; each block one 1.0 and 255 values of +-2e-4, just under half the
    unrotated quantum.  Per block, against the float64 sum: the rotated decode's L2 error is at most
        2^ceil(m/2) * W * 2^-(kblk+1)  +  the fp32 butterfly term
    (half a quantum per summand in the rotated domain, through ||H|| = sqrt(V) and the inverse's
    2^-floor(m/2); the butterfly term: sum_w ||fwd32(x_w) - fwd64(x_w)|| * 2^(m/2 - floor(m/2)) +
    ||inv32(y) - inv64(y)||, the float32 and float64 versions of tests/_rot_ref.py on the same inputs), no
    flag is raised, and the unrotated block-scaled reduce exceeds that bound on every block."""
    from ina_amd import blk, rot
    V, W, nblk, m = 256, 16, 64, 8
    rng = np.random.default_rng(2024)
    xs = (rng.choice([-2e-4, 2e-4], (W, nblk, V))).astype(F32)
    pos = rng.integers(0, V, (W, nblk))
    np.put_along_axis(xs, pos[..., None], F32(1.0), axis=2)
    xs = xs.reshape(W, nblk * V)
    bufs = [dev(x) for x in xs]
    total = xs.astype(np.float64).sum(0)
    l2 = lambda v: np.sqrt((v.astype(np.float64).reshape(nblk, V) ** 2).sum(1))

    q, flags, kb = rot.quantize_reduce_i16(bufs, V, SEED)
    xhat = host(rot.dequantize(q, kb, V, SEED))
    sg = ref.signs(nblk * V, SEED)
    y = ref.bref.dequantize(host(q), host(kb), V)
    fly = sum(l2(ref.forward(x, V, sg) - ref.forward(x, V, sg, np.float64)) for x in xs) * 2.0 ** (m / 2 - m // 2)
    fly = fly + l2(ref.inverse(y, V, sg) - ref.inverse(y, V, sg, np.float64))
    bound = 2.0 ** ((m + 1) // 2) * W * 2.0 ** -(host(kb).astype(np.float64) + 1) + fly
    err = l2(xhat - total)
    print("rotated err", err.max(), "bound", bound.min(), "butterfly term", fly.max())
    assert host(flags).sum() == 0 and (err <= bound).all()

    q0, flags0, kb0 = blk.quantize_reduce_i16(bufs, V)
    err0 = l2(host(blk.dequantize(q0, kb0, V)) - total)
    print("unrotated err", err0.min(), "bound", bound.max())
    assert (err0 > bound).all()


@pytest.mark.parametrize("alias", (False, True), ids=("out", "in-place"))
@pytest.mark.parametrize("W", (2, 8))
@pytest.mark.parametrize("V", (32, 256))
def test_ps_combine_is_the_composition(V, W, alias):
    """ps.combine_ina(rotate=seed) = deltas -> rot.quantize_reduce AUTO -> rot.dequantize -> the unfused
    update, bit for bit; out may be local."""
    from ina_amd import ps, rot
    n, ws = 37 * V, 0.37 / (W + 1)
    ps_w = buckets(torch.float32, n, V)[1][:W]
    local = (ps_w[0] * F32(0.5) + F32(0.01)).astype(F32)
    q, kb = rot.quantize_reduce([dev((p - local).astype(F32)) for p in ps_w], V, SEED)
    xhat = host(rot.dequantize(q, kb, V, SEED))
    want = (local + (xhat * F32(ws)).astype(F32)).astype(F32)
    l = dev(local)
    got = ps.combine_ina(l, [dev(p) for p in ps_w], "block", ws, out=l if alias else None, block=V, rotate=SEED)
    assert (got.data_ptr() == l.data_ptr()) == alias
    assert same_bits(host(got), want)
