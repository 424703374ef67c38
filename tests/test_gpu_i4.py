"""The 4-bit wire on the device (include/ina_i4.h, ina_amd.i4, dist.NibbleWireAggregator) against tests/_i4_ref.py,
bit for bit: scales, nibbles and flags; both slice sums; the decode glue and the round trip; the aggregator."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _i4_ref as ref
from tests import test_gpu_i8 as t8
from tests._i8_rank import bucket as rank_bucket
from tests.conftest import REPO
from tests.test_gpu_dist import _free_port
from tests.test_gpu_rot import DEV, DTYPES, E0, F32, SEED, STEP, SUB, _need_gpu, dev, grid_cap, host, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
GS = (1, 2, 3, 4, 8, 16, 17, 18, 33, 64)                  # the compile-time counts and either side of a batch of 16


def check_replay(ts, xs, V, rotate, e0=0, caps=(None,)):
    """Scales, and bucket 0's nibbles and flags under scales of which one is -128 and one 8 too large, equal the replay."""
    from ina_amd import i4
    key = dict(step=STEP, sub=SUB, e0=e0)
    want_kb = ref.block_scales(xs, V, rotate, **key)
    given = want_kb.copy()
    given[1], given[3] = -128, min(int(given[3]) + 8, 127)
    want_q, want_f = ref.quantize(xs[0], given, V, rotate, **key)
    bufs = [dev(t) for t in ts]
    for cap in caps:
        with grid_cap(cap):
            kb = i4.block_scales(bufs, V, rotate, **key)
            q, f = i4.quantize(bufs[0], dev(given), V, rotate, **key)
        assert np.array_equal(host(kb), want_kb) and np.array_equal(host(f), want_f) and want_f[3] == 1, cap
        assert np.array_equal(host(q), want_q) and ref.unpack(host(q)).min() >= -7, cap      # -8 is never written
    return want_q, want_f


@pytest.mark.parametrize("nblk", (37, 1061))           # a partial wave at V = 8; several passes of a capped grid
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
@pytest.mark.parametrize("V", (8, 32, 256))
def test_scales_nibbles_and_flags_bit_for_bit(V, rotate, dtype, nblk):
    ts, xs = t8.buckets(dtype, nblk * V, V)
    special = (V, dtype, nblk) == (32, torch.float32, 37)
    q0, f0 = check_replay(ts, xs, V, rotate, E0 if special else 0, caps=(None, 1) if nblk == 1061 else (None,))
    if special:                                        # a NaN and an inf stay in their own blocks
        bad = [x.copy() for x in xs]
        bad[0][3], bad[0][2 * V + 5] = np.nan, np.inf
        q, f = check_replay([torch.from_numpy(x) for x in bad], bad, V, rotate, E0)
        keep = np.repeat(np.arange(nblk) % 2 == 1, V // 2) | (np.arange(nblk * V // 2) >= 2 * V)
        assert np.flatnonzero(f).tolist() == [0, 2, 3] and np.flatnonzero(f0).tolist() == [3] and np.array_equal(q[keep], q0[keep])


FILLS = {"min": lambda rng, G, n: np.full((G, n), -8), "max": lambda rng, G, n: np.full((G, n), 7),
         "alt": lambda rng, G, n: np.where((np.arange(n) + np.arange(G)[:, None]) % 2, 7, -7),
         "min-max": lambda rng, G, n: np.where(np.arange(n) % 2, 7, -8) + 0 * np.arange(G)[:, None],
         "random": lambda rng, G, n: rng.integers(-8, 8, (G, n))}


@pytest.mark.parametrize("n", (8, 24, 32, 40, 4104, 70_008))      # ragged ends alone, whole chunks, both; a capped grid
@pytest.mark.parametrize("G", GS)
def test_slice_sum_is_exact(G, n):
    from ina_amd import i4
    rng = np.random.default_rng(G * 100_000 + n)
    for name, fill in FILLS.items():
        nib = fill(rng, G, n)
        out = torch.full((n + 40,), 0x5A5A, dtype=torch.int16, device=DEV)
        with grid_cap(1 if n == 70_008 else None):
            i4.sum_slices([dev(ref.pack(p)) for p in nib], out=out)
        got = host(out)
        assert np.array_equal(got[:n], nib.sum(0)) and (got[n:] == 0x5A5A).all(), name


PLANTS = {127: 0, 128: 1, 254: 1, -255: 2, -510: 3, -511: 3, -512: 3}          # a block's largest sum -> its shift


def slices(G, V, nblk):
    """Nibbles (G, nblk * V), a block at an amplitude of its own; the first blocks: a planted largest sum and exact ties."""
    rng = np.random.default_rng(G * 100_000 + V * nblk)
    amp = rng.choice([1, 2, 4, 7], (nblk, 1))
    p = rng.integers(-amp, amp + 1, (G, nblk, V))
    spread = lambda t: t // G + (np.arange(G) < t % G)                          # G nibbles that sum to t
    planted = {b: t for b, t in enumerate(PLANTS) if -8 * G <= t <= 7 * G}
    for b, t in planted.items():
        p[:, b], p[:, b, 0] = -8 if t == -8 * G else 0, spread(t)             # -512 at G = 64: a block of -8 alone
        for j, odd in enumerate((-5, -3, -1, 1, 3, 5) if PLANTS[t] else ()):
            p[:, b, 1 + j] = spread(odd << (PLANTS[t] - 1))
    return p.reshape(G, nblk * V), planted


@pytest.mark.parametrize("nblk", (37, 1061))           # n mod 32 = 8 at V = 8; several passes of a capped grid
@pytest.mark.parametrize("V", (8, 16, 32, 64, 256))
@pytest.mark.parametrize("G", GS)
def test_sum_requant_is_the_exact_rounding(G, V, nblk):
    from ina_amd import i4
    (nib, planted), n = slices(G, V, nblk), nblk * V
    parts = [ref.pack(p) for p in nib]
    want_q, want_sh = ref.requant(parts, V)
    assert all(want_sh[b] == PLANTS[t] for b, t in planted.items()) and want_sh.max() == (0 if G <= 18 else 2 if G == 33 else 3)
    assert G < 64 or (want_q[6 * V] == -64 and set(want_sh) == {0, 1, 2, 3})  # all -8 at G = 64: S = -512
    bufs = [dev(p) for p in parts]
    for cap in (None, 1) if nblk == 1061 else (None,):
        q = torch.full((n + 48,), 0x5A, dtype=torch.int8, device=DEV)
        sh = torch.full((nblk + 41,), 0x5A, dtype=torch.uint8, device=DEV)
        with grid_cap(cap):
            i4.sum_slices_requant(bufs, V, out=q, shift=sh[1:])          # the shifts at an odd address
        q, sh = host(q), host(sh)
        assert np.array_equal(q[:n], want_q) and np.array_equal(sh[1:1 + nblk], want_sh), cap
        assert (q[n:] == 0x5A).all() and sh[0] == 0x5A and (sh[1 + nblk:] == 0x5A).all(), cap


def step(xs, V, rotate, kblk=None, **key):
    """One step in process, both gathers, each stage equal to the replay: (xhat, kblk, int16 sums, any flag)."""
    from ina_amd import blk, i4, i8, rot
    bufs = [dev(x) for x in xs]
    want_kb = ref.block_scales(xs, V, rotate, **key) if kblk is None else kblk
    kb = i4.block_scales(bufs, V, rotate, **key) if kblk is None else dev(kblk)
    qs, flags = zip(*(i4.quantize(b, kb, V, rotate, **key) for b in bufs))
    s16, (q8, sh) = i4.sum_slices(qs), i4.sum_slices_requant(qs, V)
    want_s = ref.sum_slices([ref.quantize(x, want_kb, V, rotate, **key)[0] for x in xs])
    assert np.array_equal(host(kb), want_kb) and np.array_equal(host(s16), want_s)
    assert len(xs) > 18 or (not host(sh).any() and np.array_equal(host(q8), want_s))          # G <= 18: every shift is 0
    xhat = host(rot.dequantize(s16, kb, V, rotate, **key) if rotate is not None else blk.dequantize(s16, kb, V))
    assert same_bits(xhat, ref.dequantize(want_s, want_kb, V, rotate, **key))
    assert same_bits(host(i8.dequantize_gather(q8, sh, kb, V, rotate, **key)), xhat)
    return xhat, want_kb, want_s, any(host(f).any() for f in flags)


@pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
@pytest.mark.parametrize("V", (8, 256))
def test_round_trip(V, rotate):
    """G = 8: within test_gpu_i8's bound (it speaks in kblk) of the float64 sum, the numpy replay alone first; blocks of
    at most 7 non-zero +-1 a rank (every rotated value within 7) come back exactly at kblk = ceil(m/2), with no flag."""
    G, n = 8, 37 * V
    xs = ref.ref8.rref.bref.bucket(np.random.default_rng(V), G, n, V, lo=-4.0, hi=2.0)
    total, kb = xs.astype(np.float64).sum(0), ref.block_scales(xs, V, rotate)
    s16 = ref.sum_slices([ref.quantize(x, kb, V, rotate)[0] for x in xs])
    lim = t8.bound(xs, V, rotate, kb, s16)
    assert (t8.l2(ref.dequantize(s16, kb, V, rotate) - total, V) <= lim).all()          # before the device sees it
    assert (t8.l2(step(list(xs), V, rotate)[0] - total, V) <= lim).all()
    rng, ints = np.random.default_rng(V + 1), np.zeros((G, n // V, V), F32)
    np.put_along_axis(ints, rng.permuted(np.tile(np.arange(V), (G, n // V, 1)), axis=2)[..., :7],
                      rng.choice([-1, 0, 1], (G, n // V, 7)).astype(F32), axis=2)
    kblk = np.full(n // V, 0 if rotate is None else V.bit_length() // 2, np.int8)
    xhat, _, _, flagged = step(list(ints.reshape(G, n)), V, rotate, kblk=kblk)
    assert not flagged and np.array_equal(xhat, ints.reshape(G, n).sum(0))


@pytest.mark.parametrize("world,gather", ((1, "i8"), (1, "i16"), (2, "i8"), (3, "i8"), (3, "i16")))
def test_aggregator_ranks_hold_the_in_process_result(tmp_path, world, gather):
    """1-3 ranks over gloo hold, bit for bit, the calls written out in process; the byte counts are the arithmetic's."""
    n, V = 70_016, 64
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.join(REPO, "tests", "_i4_rank.py"),
           str(n), str(V), str(SEED), str(tmp_path), gather]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    want, kb, s16, _ = step([rank_bucket(w, n) for w in range(world)], V, SEED, step=1)     # the second step
    for rank in range(world):
        d = np.load(os.path.join(tmp_path, f"rank{rank}.npz"))
        shard, g = int(d["shard"]), world - 1
        assert same_bits(d["full"], want) and np.array_equal(d["kblk"], kb) and np.array_equal(d["sums"][:n], s16), rank
        assert not d["shift"].any() and shard % 128 == 0 and not d["q4"][n // 2:].any() and not d["sums"][n:].any(), rank
        assert d["bytes"].tolist() == [g * shard // 2, g * (shard + shard // V if gather == "i8" else 2 * shard), n // V if g else 0]
