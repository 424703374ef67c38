"""The requantised 8-bit gather on the device (include/ina_i8_gather.h, ina_amd.i8, dist.ByteWireAggregator
(gather="i8")), bit for bit: sum + requantise against exact numpy; the decode against the existing decodes of
(int16)q8 << shift and against tests/_rot_ref.py; the round trip within its bound; the aggregator on 1-3 ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _i8_ref as ref
from tests import test_gpu_i8 as t8
from tests._i8_rank import bucket as rank_bucket
from tests.conftest import REPO
from tests.test_gpu_dist import _free_port
from tests.test_gpu_rot import DEV, E0, F32, SEED, STEP, SUB, _need_gpu, dev, grid_cap, host, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
SH0 = {1: 1, 2: 2, 3: 2, 4: 3, 8: 4, 16: 5, 17: 5, 64: 7}                       # the shift of a block whose largest |sum| is 128 G


requant = ref.requant                # the yardstick lives in the ref module (tests/_graph.py shares it)


def slices(G, V, nblk):
    """Each block at an amplitude of its own; block 0 all -128, 1 all 127, 2 zero, 3 and 4 (G >= 3) with largest
    |sum| 254 and 255, 5 with -128 G and the odd multiples of 2^(sh-1) of both signs beside it (ties)."""
    rng = np.random.default_rng(G * 100_000 + V * nblk)
    amp = rng.choice([1, 2, 5, 16, 64, 127], (nblk, 1))
    p = rng.integers(-amp, amp + 1, (G, nblk, V))
    p[:, 0], p[:, 1], p[:, 2:6] = -128, 127, 0
    if G >= 3:
        p[:3, 3, 5], p[:3, 4, V - 1] = [127, 127, 0], [-127, -127, -1]
    p[:, 5, 0] = -128
    for j, t in enumerate(odd << (SH0[G] - 1) for odd in (-5, -3, -1, 1, 3, 5)):
        p[:, 5, 1 + j] = t // G + (np.arange(G) < t % G)             # G bytes that sum to t
    return p.reshape(G, nblk * V).astype(np.int8)


@pytest.mark.parametrize("nblk", (37, 1061))           # n mod 16 = 8 at V = 8; several passes of a capped grid
@pytest.mark.parametrize("V", (8, 16, 32, 256))
@pytest.mark.parametrize("G", (1, 2, 3, 4, 8, 16, 17, 64))    # compile-time and run-time slice counts
def test_sum_requant_is_the_exact_rounding(G, V, nblk):
    from ina_amd import i8
    parts, n = slices(G, V, nblk), nblk * V
    want_q, want_sh = requant(parts, V)
    assert want_sh[0] == want_sh[5] == SH0[G] and want_sh[2] == 0 and (G < 3 or (want_sh[3], want_sh[4]) == (1, 2))
    bufs = [dev(p) for p in parts]
    for cap in (None, 1) if nblk == 1061 else (None,):
        q = torch.full((n + 48,), 0x5A, dtype=torch.int8, device=DEV)
        sh = torch.full((nblk + 41,), 0x5A, dtype=torch.uint8, device=DEV)
        with grid_cap(cap):
            i8.sum_slices_requant(bufs, V, out=q, shift=sh[1:])          # the shifts at an odd address
        q, sh = host(q), host(sh)
        assert np.array_equal(q[:n], want_q) and np.array_equal(sh[1:1 + nblk], want_sh), cap
        assert (q[n:] == 0x5A).all() and sh[0] == 0x5A and (sh[1 + nblk:] == 0x5A).all() and q[:n].min() >= -127


@pytest.mark.parametrize("nblk", (37, 1061))
@pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
@pytest.mark.parametrize("V", (8, 32, 256))
def test_decode_is_the_int16_decode_of_the_shifted_bytes(V, rotate, nblk):
    from ina_amd import blk, i8, rot
    rng, n = np.random.default_rng(V + nblk), nblk * V
    q8, sh = rng.integers(-127, 128, n).astype(np.int8), (np.arange(nblk) % 8).astype(np.uint8)
    kb = rng.choice([-126, -3, 0, 14, 127], nblk).astype(np.int8)
    sh[9] = 200                                                          # a shift byte above 7 is read as 7
    s16 = q8.astype(np.int16) << np.repeat(np.minimum(sh, 7), V).astype(np.int16)
    key = dict(step=STEP, sub=SUB, e0=E0 if (V, nblk) == (32, 37) else 0) if rotate is not None else {}
    for cap in (None, 1) if nblk == 1061 else (None,):
        with grid_cap(cap):
            got = host(i8.dequantize_gather(dev(q8), dev(sh), dev(kb), V, rotate, **key))
            want = host(rot.dequantize(dev(s16), dev(kb), V, rotate, **key) if rotate is not None
                        else blk.dequantize(dev(s16), dev(kb), V))
        assert same_bits(got, want) and same_bits(got, ref.dequantize(s16, kb, V, rotate, **key)), cap


def gather_step(xs, V, rotate, kblk=None, **key):
    """One gather="i8" step in process on the device: (xhat, bytes, shifts), the bytes and shifts the numpy replay's."""
    from ina_amd import i8
    kb = dev(ref.block_scales(xs, V, rotate, **key) if kblk is None else kblk)
    qs = [i8.quantize(dev(x), kb, V, rotate, **key)[0] for x in xs]
    q8, sh = i8.sum_slices_requant(qs, V)
    want_q, want_sh = requant([ref.quantize(x, host(kb), V, rotate, **key)[0] for x in xs], V)
    assert np.array_equal(host(q8), want_q) and np.array_equal(host(sh), want_sh)
    return host(i8.dequantize_gather(q8, sh, kb, V, rotate, **key)), want_q, want_sh


def test_round_trip_within_the_bound():
    """G = 8, V = 256 on test_gpu_i8's "what the rotation buys" inputs: per block against the float64 sum the L2
    error is within test_gpu_i8's bound plus the requantiser's half quantum through the inverse rotation, 2^ceil(m/2)
    * 2^(sh - kblk - 1), the numpy replay alone first.  Integer inputs whose sums stay within +-127 come back exactly."""
    G, V, nblk, m = 8, 256, 64, 8
    rng = np.random.default_rng(2024)
    xs = rng.choice([-3e-3, 3e-3], (G, nblk, V)).astype(F32)
    np.put_along_axis(xs, rng.integers(0, V, (G, nblk))[..., None], F32(1.0), axis=2)
    xs = xs.reshape(G, nblk * V)
    total, kb = xs.astype(np.float64).sum(0), ref.block_scales(xs, V, SEED)
    q8, sh = requant([ref.quantize(x, kb, V, SEED)[0] for x in xs], V)
    s16 = q8.astype(np.int16) << np.repeat(sh, V).astype(np.int16)
    lim = t8.bound(xs, V, SEED, kb, s16) + 2.0 ** ((m + 1) // 2) * 2.0 ** (sh.astype(np.float64) - kb - 1)
    replay = ref.dequantize(s16, kb, V, SEED)
    assert (t8.l2(replay - total, V) <= lim).all()                       # before the device sees it
    xhat, _, got_sh = gather_step(list(xs), V, SEED)
    x16 = t8.step(list(xs), V, SEED)[0]
    err, rms8, rms16 = t8.l2(xhat - total, V), np.sqrt(((xhat - total) ** 2).mean()), np.sqrt(((x16 - total) ** 2).mean())
    print("max block err", err.max(), "bound", lim.min(), "shifts", got_sh.min(), got_sh.max(), "rms", rms8, rms16, rms8 / rms16)
    assert np.array_equal(xhat, replay) and (err <= lim).all()
    ints = np.random.default_rng(5).choice([-1, 0, 0, 0, 0, 0, 0, 1], (G, 37 * V)).astype(F32)
    xhat, _, got_sh = gather_step(list(ints), V, SEED, kblk=np.full(37, 4, np.int8))
    assert not got_sh.any() and np.array_equal(xhat, ints.sum(0))


def test_aggregator_on_one_rank():
    """gather="i8" is the calls written out; one rank's bytes need no shift, so it is also the gather="i16" result,
    which is test_gpu_i8's step (the int16 gather as it was) on the same bucket."""
    from ina_amd.dist import ByteWireAggregator
    n, V = 70_016, 64
    x = rank_bucket(0, n)
    full = {}
    for gather in ("i8", "i16"):
        agg = ByteWireAggregator(n, V=V, device=torch.device(DEV), seed=SEED, gather=gather)
        agg.step = STEP
        full[gather] = host(agg(dev(x)))
        assert agg.step == STEP + 1 and agg.gather_bytes == 0
    want, q8, sh = gather_step([x], V, SEED, step=STEP)
    assert same_bits(full["i8"], want) and np.array_equal(host(agg.kblk), ref.block_scales([x], V, SEED, step=STEP))
    assert same_bits(full["i16"], t8.step([x], V, SEED, step=STEP)[0]) and same_bits(full["i8"], full["i16"])


@pytest.mark.parametrize("world", (2, 3))
def test_aggregator_ranks_hold_the_in_process_result(tmp_path, world):
    """2 and 3 ranks on one GPU over gloo hold the in-process sequence's result, scales, bytes and shifts."""
    n, V = 70_016, 64
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.join(REPO, "tests", "_i8_gather_rank.py"),
           str(n), str(V), str(SEED), str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    xs = [rank_bucket(w, n) for w in range(world)]
    want, q8, sh = gather_step(xs, V, SEED, step=1)                      # the second step
    assert sh.max() >= 1
    for rank in range(world):
        d = np.load(os.path.join(tmp_path, f"rank{rank}.npz"))
        assert same_bits(d["full"], want) and np.array_equal(d["kblk"], ref.block_scales(xs, V, SEED, step=1)), rank
        assert np.array_equal(d["q8"][:n], q8) and np.array_equal(d["shift"], sh) and not d["q8"][n:].any(), rank
        shard = int(d["shard"])
        assert d["bytes"].tolist() == [(world - 1) * shard, (world - 1) * (shard + shard // V), n // V]
