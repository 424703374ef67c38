"""Stochastic rounding on the byte wire on the device (include/ina_i8_sr.h), bit for bit against
tests/_i8_sr_ref.py: quantiser, scales, requantised slice sum, the bias of both, the aggregator on 1 and 3 ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _i8_sr_ref as sref
from tests._i8_rank import bucket as rank_bucket
from tests.conftest import REPO
from tests.test_gpu_dist import _free_port
from tests.test_gpu_rot import DEV, DTYPES, F32, SEED, STEP, _need_gpu, dev, grid_cap, host, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
BIG = dict(e0=(1 << 34) + 4, sub=(1 << 32) - 1, rot_e0=(1 << 34) + 768)    # 64-bit offsets, the last stream
RND = dict(step=STEP, sub=9, e0=16 * 1_000_003)
PLANTED = (127, 128, 254, 255, 508, 509, 8128, 8129, 8192)


def bucket(dtype, n, V):                       # (device tensor, its float32 widening); blocks over four decades
    rng = np.random.default_rng(n + V)
    x = rng.standard_normal(n) * np.repeat(10.0 ** rng.uniform(-3, 1, n // V), V)
    t = torch.from_numpy(x.astype(F32)).to(dtype)
    return t.to(DEV), t.float().numpy()


@pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
@pytest.mark.parametrize("V,dtype,nblk,key", [(V, dt, 37, dict(sub=3)) for V in (8, 64, 256) for dt in DTYPES]
                         + [(64, DTYPES[0], 1061, dict(sub=3)), (256, DTYPES[1], 37, BIG)])
def test_quantiser_and_scales_replay(V, dtype, nblk, key, rotate):
    """Scales, bytes and flags equal the replay; own scales never flag; a slice under e0 = lo is that slice."""
    from ina_amd import i8
    n = nblk * V
    t, x = bucket(dtype, n, V)
    rk = dict(step=STEP, sub=key.get("rot_sub", 0), e0=key.get("rot_e0", 0))
    want_kb = sref.block_scales([x], V, rotate, **rk)
    want_q, want_f = sref.quantize(x, want_kb, V, SEED ^ 5, rotate, step=STEP, **key)
    for cap in (None, 1) if nblk == 1061 else (None,):
        with grid_cap(cap):
            kb = i8.block_scales_sr([t], V, rotate, **rk)
            q, f = i8.quantize_sr(t, kb, V, SEED ^ 5, rotate, step=STEP, **key)
        assert np.array_equal(host(kb), want_kb) and np.array_equal(host(q), want_q), cap
        assert np.array_equal(host(f), want_f) and not want_f.any() and host(q).min() >= -127
    lo, hi = 3 * 256, n - 256
    if nblk == 37 and V == 64:
        part = i8.quantize_sr(t[lo:hi], kb[lo // V:hi // V], V, SEED ^ 5, rotate, step=STEP, sub=3, e0=lo, rot_e0=lo)[0]
        assert np.array_equal(host(part), want_q[lo:hi])


@pytest.mark.parametrize("rotate", (None, SEED), ids=("plain", "rot"))
def test_integers_and_edges(rotate):
    """Integer t: i8.quantize's bytes for every seed.  A NaN and the infs stay in their blocks (0 / +-127 and the
    flag); a scale 8 too large clamps and flags; -128 never appears."""
    from ina_amd import i8
    V, nblk = 64, 37
    x = np.random.default_rng(3).integers(-1, 2, nblk * V).astype(F32)
    kb = dev(np.full(nblk, 0 if rotate is None else 3, np.int8))             # ceil(m/2) undoes the forward norm
    rne = host(i8.quantize(dev(x), kb, V, rotate, step=STEP)[0])
    for seed in (0, 1, SEED):
        q, f = i8.quantize_sr(dev(x), kb, V, seed, rotate, step=STEP, sub=2)
        assert np.array_equal(host(q), rne) and not host(f).any(), seed
    x = bucket(torch.float32, nblk * V, V)[1]
    x[5], x[2 * V + 1], x[4 * V] = np.nan, np.inf, -np.inf
    kb = sref.block_scales([x], V, rotate, step=STEP)
    kb[7:9] += 8
    q, f = (host(a) for a in i8.quantize_sr(dev(x), dev(kb), V, 77, rotate, step=STEP, sub=2))
    want_q, want_f = sref.quantize(x, kb, V, 77, rotate, step=STEP, sub=2)
    assert np.array_equal(q, want_q) and np.array_equal(f, want_f) and q.min() == -127 and q.max() == 127
    assert f[[0, 2, 4, 7, 8]].all() and f.sum() == 5 and (rotate or (q[5], q[2 * V + 1], q[4 * V]) == (0, 127, -127))


def slices(G, V, nblk):
    """Random bytes; block 0 all -128, block 1 all 127; from block 2 on, small sums and one planted sum of -A."""
    rng = np.random.default_rng(G * 100_000 + V * nblk)
    p = rng.integers(-(amp := rng.choice([1, 2, 5, 16, 64, 127], (nblk, 1))), amp + 1, (G, nblk, V))
    p[:, 0], p[:, 1] = -128, 127
    for b, A in enumerate((a for a in PLANTED if a <= 128 * G), start=2):
        p[:, b] = rng.integers(-1, 2, (G, V)) * (np.arange(G) % 2)[:, None]
        p[:, b, b % V] = -A // G + (np.arange(G) < -A % G)               # G bytes that sum to -A
    return p.reshape(G, nblk * V).astype(np.int8)


@pytest.mark.parametrize("nblk", (37, 1061))           # n mod 16 = 8 at V = 8; several passes of a capped grid
@pytest.mark.parametrize("V", (8, 16, 256))
@pytest.mark.parametrize("G", (1, 2, 3, 4, 8, 16, 17, 64))    # compile-time and run-time slice counts
def test_requantiser_replay(G, V, nblk):
    from ina_amd import i8
    parts, n = slices(G, V, nblk), nblk * V
    want_q, want_sh = sref.requant(parts, V, SEED, **RND)
    reach = [a for a in PLANTED if a <= 128 * G]
    assert want_sh[2:2 + len(reach)].tolist() == [(0, 1, 1, 2, 2, 3, 6, 7, 7)[PLANTED.index(a)] for a in reach]
    bufs = [dev(p) for p in parts]
    for cap in (None, 1) if nblk == 1061 else (None,):
        q = torch.full((n + 48,), 0x5A, dtype=torch.int8, device=DEV)
        sh = torch.full((nblk + 41,), 0x5A, dtype=torch.uint8, device=DEV)
        with grid_cap(cap):
            i8.sum_slices_requant_sr(bufs, V, SEED, out=q, shift=sh[1:], **RND)      # the shifts at an odd address
        q, sh = host(q), host(sh)
        assert np.array_equal(q[:n], want_q) and np.array_equal(sh[1:1 + nblk], want_sh), cap
        assert (q[n:] == 0x5A).all() and sh[0] == 0x5A and (sh[1 + nblk:] == 0x5A).all()
    rne_q, rne_sh = (host(a) for a in i8.sum_slices_requant(bufs, V))
    flat = want_sh == 0                                                      # A <= 127: the sibling's bytes and shifts
    assert flat.any() and not rne_sh[flat].any() and np.array_equal(rne_q.reshape(-1, V)[flat], want_q.reshape(-1, V)[flat])


def within_5_sigma(ups, p):
    print("mean", ups.mean(), "p", p, "sigma", sigma := np.sqrt(p * (1 - p) / ups.size))
    return abs(ups.mean() - p) <= 5 * sigma


def test_bias_of_the_quantiser():
    """65,536 values of t = 0.25: round-to-nearest sends zeros, stochastic rounding a mean within 5 sigma of 0.25."""
    from ina_amd import i8
    n, V = 65_536, 256
    x, kb = dev(np.full(n, 0.25, F32)), dev(np.zeros(n // V, np.int8))
    q = host(i8.quantize_sr(x, kb, V, 0x1234, step=3, sub=1)[0])
    assert not host(i8.quantize(x, kb, V)[0]).any()
    assert np.array_equal(q, sref.quantize(host(x), host(kb), V, 0x1234, step=3, sub=1)[0]) and within_5_sigma(q, 0.25)


@pytest.mark.parametrize("S,sh,plant", ((301, 2, 508), (-301, 2, 508), (8063, 7, -8192), (-8129, 7, -8192), (1000, 3, 1016)))
def test_bias_of_the_requantiser(S, sh, plant):
    """G = 64, blocks of 255 constant sums S and one planted sum that fixes the shift: q8 - (S >> sh) is 1 with
    probability (S mod 2^sh) / 2^sh.  (64 bytes sum to at most 8128, so 127/128 at shift 7 is S = 8063.)"""
    from ina_amd import i8
    G, V, nblk = 64, 256, 256
    s = np.full((nblk, V), S)
    s[:, 0] = plant
    parts = (s.reshape(-1) // G + (np.arange(G)[:, None] < s.reshape(-1) % G)).astype(np.int8)
    assert np.array_equal(parts.astype(np.int64).sum(0), s.reshape(-1))
    key = dict(step=5, sub=65, e0=1024)
    q, got_sh = (host(a) for a in i8.sum_slices_requant_sr([dev(p) for p in parts], V, 0x1234, **key))
    want_q, want_sh = sref.requant(parts, V, 0x1234, **key)
    assert np.array_equal(q, want_q) and np.array_equal(got_sh, want_sh) and (got_sh == sh).all()
    ups, p = q.reshape(nblk, V)[:, 1:].astype(np.int64) - (S >> sh), (S % (1 << sh)) / (1 << sh)
    assert (ups == 0).all() if p == 0 else within_5_sigma(ups, p)


def sr_step(xs, V, seed, step, gather, shard):
    """One stochastic step of the aggregator written out in i8 calls: (full, q8, shifts)."""
    from ina_amd import i8, rot
    from ina_amd._lib import MAX_WORKERS
    n, pad = xs[0].size, shard * len(xs) - xs[0].size
    kb = torch.stack([i8.block_scales_sr([dev(x)], V, seed, step=step) for x in xs]).amin(0)
    qs = [torch.nn.functional.pad(i8.quantize_sr(dev(x), kb, V, seed, seed, step=step, sub=1 + r)[0], (0, pad))
          for r, x in enumerate(xs)]
    kb = torch.nn.functional.pad(kb, (0, pad // V), value=127)
    if gather == "i16":
        return host(rot.dequantize(i8.sum_slices(qs), kb, V, seed, step=step))[:n], None, None
    own = [i8.sum_slices_requant_sr([q[r * shard:(r + 1) * shard] for q in qs], V, seed, step=step, sub=1 + MAX_WORKERS,
                                    e0=r * shard) for r in range(len(xs))]
    q8, sh = torch.cat([o[0] for o in own]), torch.cat([o[1] for o in own])
    return host(i8.dequantize_gather(q8, sh, kb, V, seed, step=step))[:n], host(q8), host(sh)[:n // V]


@pytest.mark.parametrize("gather", ("i16", "i8"))
def test_aggregator_on_one_rank(gather):
    from ina_amd.dist import ByteWireAggregator
    n, V = 70_016, 64
    x = rank_bucket(0, n)
    agg = ByteWireAggregator(n, V=V, device=torch.device(DEV), seed=SEED, gather=gather, rounding="stochastic")
    agg.step = STEP
    for step in (STEP, STEP + 1):
        assert same_bits(host(agg(dev(x))), sr_step([x], V, SEED, step, gather, agg.plan.shard)[0]) and agg.step == step + 1


def test_aggregator_ranks_hold_the_in_process_result(tmp_path):
    """3 ranks on one GPU over gloo hold the in-process sequence's result, bytes and shifts."""
    from ina_amd.dist import ShardPlan
    n, V, world = 70_016, 64, 3
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.join(REPO, "tests", "_i8_sr_rank.py"),
           str(n), str(V), str(SEED), str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    shard = ShardPlan(n, world, 1024).shard
    want, q8, sh = sr_step([rank_bucket(w, n) for w in range(world)], V, SEED, 1, "i8", shard)     # the second step
    assert sh.max() >= 1
    for rank in range(world):
        d = np.load(os.path.join(tmp_path, f"rank{rank}.npz"))
        assert same_bits(d["full"], want) and np.array_equal(d["q8"], q8) and np.array_equal(d["shift"], sh), rank
        assert d["bytes"].tolist() == [(world - 1) * shard, (world - 1) * (shard + shard // V), n // V]
