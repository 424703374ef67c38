"""The 8-bit wire on the device (include/ina_i8.h, ina_amd.i8, dist.ByteWireAggregator) against
tests/_i8_ref.py, bit for bit: scales, bytes and flags; the slice sum at its field-carry and bias cases; the
round trip within its bound and exact on integers; what the rotation buys; the aggregator on 1, 2 and 3 ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _i8_ref as ref
from tests._i8_rank import bucket as rank_bucket
from tests.conftest import REPO
from tests.test_gpu_dist import _free_port
from tests.test_gpu_rot import DEV, DTYPES, E0, F32, SEED, STEP, SUB, _need_gpu, dev, grid_cap, host  # noqa: F401

pytestmark = pytest.mark.gpu
_BUCKETS = {}


def buckets(dtype, n, V):
    """3 seeded buckets as (tensors of dtype, their exact float32 widenings), scales differing block to block."""
    if (dtype, n, V) not in _BUCKETS:
        x = ref.rref.bref.bucket(np.random.default_rng(n * 1000 + V), 3, n, V, lo=-4.0, hi=2.0)
        ts = [torch.from_numpy(r).to(dtype) for r in x]
        _BUCKETS[dtype, n, V] = (ts, [t.float().numpy() for t in ts])
    return _BUCKETS[dtype, n, V]


def check_replay(ts, xs, V, rotate, e0=0, caps=(None,)):
    """The scales of all the buckets, and bucket 0's bytes and flags under scales of which one is read as
    -126 and one is 8 too large (its block clamps), equal the replay; -128 is never written."""
    from ina_amd import i8
    key = dict(step=STEP, sub=SUB, e0=e0)
    want_kb = ref.block_scales(xs, V, rotate, **key)
    given = want_kb.copy()
    given[1], given[3] = -128, min(int(given[3]) + 8, 127)
    want_q, want_f = ref.quantize(xs[0], given, V, rotate, **key)
    bufs = [dev(t) for t in ts]
    for cap in caps:
        with grid_cap(cap):
            kb = i8.block_scales(bufs, V, rotate, **key)
            q, f = i8.quantize(bufs[0], dev(given), V, rotate, **key)
        assert np.array_equal(host(kb), want_kb) and np.array_equal(host(f), want_f), cap
        assert np.array_equal(host(q), want_q) and host(q).min() >= -127, cap
    return want_q, want_f


@pytest.mark.parametrize("nblk", (37, 1061))           # a partial wave at V = 8; several passes of a capped grid
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
@pytest.mark.parametrize("V", (8, 32, 256))
def test_scales_and_bytes_bit_for_bit(V, rotate, dtype, nblk):
    ts, xs = buckets(dtype, nblk * V, V)
    e0 = E0 if (V, dtype, nblk) == (32, torch.float32, 37) else 0
    check_replay(ts, xs, V, rotate, e0, caps=(None, 1) if nblk == 1061 else (None,))


@pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
def test_nan_inf_and_clamp_stay_in_their_blocks(rotate):
    """A NaN in block 0, an inf in block 2 and the too-large scale of block 3: the replay's bits, flags for
    exactly those blocks, and every other block's bytes as without them."""
    V, n = 32, 37 * 32
    clean = buckets(torch.float32, n, V)[1]
    xs = [x.copy() for x in clean]
    xs[0][3], xs[0][2 * V + 5] = np.nan, np.inf
    q, f = check_replay([torch.from_numpy(x) for x in xs], xs, V, rotate)
    q0, f0 = check_replay([torch.from_numpy(x) for x in clean], clean, V, rotate)
    assert np.flatnonzero(f).tolist() == [0, 2, 3] and np.flatnonzero(f0).tolist() == [3]
    keep = np.arange(n) // V % 2 == 1
    assert np.array_equal(q[keep], q0[keep]) and np.array_equal(q[4 * V:], q0[4 * V:])


FILLS = {"random": lambda rng, G, n: rng.integers(-128, 128, (G, n)), "min": lambda rng, G, n: np.full((G, n), -128),
         "max": lambda rng, G, n: np.full((G, n), 127),
         "alt": lambda rng, G, n: np.where((np.arange(n) + np.arange(G)[:, None] // 2) % 2, 127, -127)}


@pytest.mark.parametrize("n", (1, 15, 16, 17, 4099, 70_001))      # tails alone, whole chunks, both; a capped grid
@pytest.mark.parametrize("G", (1, 2, 3, 4, 8, 16, 17, 64))       # compile-time and run-time slice counts
def test_slice_sum_is_exact(G, n):
    """Whole slices of -128 (the bias at its limit), of 127 (the fields at their largest) and of alternating
    +-127 (neighbouring fields of opposite sign), and random bytes; nothing is written past n."""
    from ina_amd import i8
    rng = np.random.default_rng(G * 100_000 + n)
    for name, fill in FILLS.items():
        parts = fill(rng, G, n).astype(np.int8)
        out = torch.full((n + 40,), 0x5A5A, dtype=torch.int16, device=DEV)
        with grid_cap(1 if n == 70_001 else None):
            i8.sum_slices([dev(p) for p in parts], out=out)
        got = host(out)
        assert np.array_equal(got[:n], ref.sum_slices(parts)) and (got[n:] == 0x5A5A).all(), name


def l2(v, V):
    return np.sqrt((v.astype(np.float64).reshape(-1, V) ** 2).sum(1))


def step(xs, V, rotate, kblk=None, **key):
    """One step in process -- scales over all the buckets (the ranks' MIN) unless given, each bucket's bytes,
    their sum, the decode -- each equal to the replay.  Returns (xhat, kblk, int16 sums, any flag)."""
    from ina_amd import blk, i8, rot
    bufs = [dev(x) for x in xs]
    want_kb = ref.block_scales(xs, V, rotate, **key) if kblk is None else kblk
    kb = i8.block_scales(bufs, V, rotate, **key) if kblk is None else dev(kblk)
    qs, flags = zip(*(i8.quantize(b, kb, V, rotate, **key) for b in bufs))
    s16 = i8.sum_slices(qs)
    xhat = host(rot.dequantize(s16, kb, V, rotate, **key) if rotate is not None else blk.dequantize(s16, kb, V))
    want_s = ref.sum_slices([ref.quantize(x, want_kb, V, rotate, **key)[0] for x in xs])
    assert np.array_equal(host(kb), want_kb) and np.array_equal(host(s16), want_s)
    assert np.array_equal(xhat, ref.dequantize(want_s, want_kb, V, rotate, **key))
    return xhat, want_kb, want_s, any(host(f).any() for f in flags)


def bound(xs, V, rotate, kb, s16):
    """Per block: half a quantum per summand through the rotation (||H|| = sqrt(V), the inverse's
    2^-floor(m/2)), plus the fp32 butterfly term from the float32 and float64 versions of tests/_rot_ref.py."""
    m, half = V.bit_length() - 1, len(xs) * 2.0 ** -(np.maximum(kb.astype(np.float64), -126) + 1)
    if rotate is None:
        return np.sqrt(V) * half
    fly = sum(l2(ref.rotated(x, V, rotate) - ref.rotated(x, V, rotate, dtype=np.float64), V) for x in xs)
    inv = l2(ref.dequantize(s16, kb, V, rotate) - ref.dequantize(s16, kb, V, rotate, dtype=np.float64), V)
    return 2.0 ** ((m + 1) // 2) * half + fly * 2.0 ** (m / 2 - m // 2) + inv


@pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
@pytest.mark.parametrize("V", (8, 256))
def test_round_trip(V, rotate):
    """G = 8 buckets under agreed scales: the decode of the summed bytes is within the bound of the float64
    sum on every block, and integer inputs at kblk = ceil(m/2) (0 unrotated) come back bit for bit."""
    G, n = 8, 37 * V
    xs = ref.rref.bref.bucket(np.random.default_rng(V), G, n, V, lo=-4.0, hi=2.0)
    xhat, kb, s16, _ = step(list(xs), V, rotate)
    assert (l2(xhat - xs.astype(np.float64).sum(0), V) <= bound(xs, V, rotate, kb, s16)).all()
    ints = np.random.default_rng(V + 1).choice([-1, 0, 0, 1], (G, n)).astype(F32)
    k = 0 if rotate is None else V.bit_length() // 2
    xhat, _, _, flagged = step(list(ints), V, rotate, kblk=np.full(n // V, k, np.int8))
    assert not flagged and np.array_equal(xhat, ints.sum(0))


def test_what_the_rotation_buys_on_the_byte_wire():
    """G = 8, V = 256, 64 blocks, each one 1.0 and 255 values of +-3e-3 with signs independent per rank (a fifth
    of the unrotated quantum 2^-6).  Per block against the float64 sum, the rotated decode's L2 error is at most
    2^ceil(m/2) * G * 2^-(kblk+1) + the fp32 butterfly term, no flag is raised, and the unrotated byte wire
    exceeds that bound on every block.  (The numpy replay alone: kblk 10 against 6, bound 0.0625, rotated error
    at most 0.0145, unrotated 0.121 to 0.147.)"""
    G, V, nblk = 8, 256, 64
    rng = np.random.default_rng(2024)
    xs = rng.choice([-3e-3, 3e-3], (G, nblk, V)).astype(F32)
    np.put_along_axis(xs, rng.integers(0, V, (G, nblk))[..., None], F32(1.0), axis=2)
    xs = xs.reshape(G, nblk * V)
    total = xs.astype(np.float64).sum(0)
    xhat, kb, s16, flagged = step(list(xs), V, SEED)
    lim, err = bound(xs, V, SEED, kb, s16), l2(xhat - total, V)
    print("rotated err", err.max(), "bound", lim.min(), lim.max(), "kblk", kb.min(), kb.max())
    assert not flagged and (err <= lim).all()
    err0 = l2(step(list(xs), V, None)[0] - total, V)
    print("unrotated err", err0.min(), err0.max())
    assert (err0 > lim).all()


@pytest.mark.parametrize("rotate", (False, True), ids=("plain", "rot"))
def test_aggregator_on_one_rank(rotate):
    from ina_amd.dist import ByteWireAggregator
    n, V = 70_001 // 32 * 32 if rotate else 70_001, 32          # the plain wire takes a ragged last block
    x = rank_bucket(0, n)
    agg = ByteWireAggregator(n, V=V, device=torch.device(DEV), rotate=rotate, seed=SEED)
    agg.step = STEP
    full = host(agg(dev(x)))
    want, kb, s16, _ = step([np.concatenate([x, np.zeros(-n % V, F32)])], V, SEED if rotate else None, step=STEP)
    assert np.array_equal(full, want[:n]) and np.array_equal(host(agg.kblk), kb)
    assert np.array_equal(host(agg.s16_full)[:n], s16[:n]) and not host(agg.s16_full)[s16.size:].any()
    assert agg.step == STEP + 1 and (agg.wire_bytes, agg.gather_bytes, agg.scale_bytes) == (0, 0, 0)


@pytest.mark.parametrize("world", (2, 3))
def test_aggregator_ranks_hold_the_in_process_result(tmp_path, world):
    """2 and 3 ranks on one GPU over gloo: every rank's full, kblk and int16 sums after two steps are, bit for
    bit, the in-process sequence's on the same buckets; the byte counts are the arithmetic's."""
    n, V = 70_016, 64
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.join(REPO, "tests", "_i8_rank.py"),
           str(n), str(V), str(SEED), str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    want, kb, s16, _ = step([rank_bucket(w, n) for w in range(world)], V, SEED, step=1)     # the second step
    for rank in range(world):
        d = np.load(os.path.join(tmp_path, f"rank{rank}.npz"))
        assert np.array_equal(d["full"], want) and np.array_equal(d["kblk"], kb), rank
        assert np.array_equal(d["s16"][:n], s16), rank
        shard = int(d["shard"])
        assert shard % 128 == 0 and d["bytes"].tolist() == [(world - 1) * shard, (world - 1) * shard * 2, n // V]
