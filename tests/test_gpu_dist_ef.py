"""ShardedAggregator(error_feedback=True) at world size > 1 with the device kernels: 2 and 3 ranks
launched by torch.distributed.run, all on cuda:0 with a gloo group (as tests/test_gpu_dist_blk.py),
T = 3 steps on seeded per-rank, per-step buckets.  After every step each rank's aggregate, residual,
flags and agreed scales equal, bit for bit, a numpy replay of all ranks together: each rank's
v = x + r, the MIN of the ranks' scales (_ef_ref.block_scales over all ranks' v), the oracle's wires,
their int64 sum cast to int32, the oracle's finish and decode, and each rank's carry of its own q."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import _blk_ref as bref
from tests import _ef_ref as eref
from tests import _shard_blk_ref as sref
from tests._dist_ef_rank import bucket
from tests.conftest import REPO

LIB_NAME = os.path.basename(os.environ.get("INA_LIBRARY", "libina.so"))
RANK_SCRIPT = os.path.join(REPO, "tests", "_dist_ef_rank.py")
F32 = np.float32


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world, n, V, wire, k, coll, chunks, steps=3, data="random"):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", RANK_SCRIPT,
           "--size", str(n), "--wire", wire, "--k", str(k), "--V", str(V), "--steps", str(steps), "--out", str(tmp_path),
           "--collective", coll, "--chunks", str(chunks), "--data", data]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{i}.npz"))) for i in range(world)]


def _q16_of(word):
    w = np.asarray(word, np.int64) & 0x3FFFFF
    return np.where(w >= 1 << 21, w - (1 << 22), w).astype(np.int32)


def _carry(v, q, kb, k, V):
    if kb is None:
        return eref.carry(v, q, k)
    return np.concatenate([eref.carry(v[sl], q[sl], bref.keff(kb[s])) for s, sl in enumerate(bref.blocks(v.size, V))])


def _replay_step(xs, rs, wire, k, V):
    """All ranks' buckets and residuals of one step -> (full, flags or None, kblk or None, new residuals)."""
    world = len(xs)
    vs = [eref.v_of(x, r) for x, r in zip(xs, rs)]
    kb = eref.block_scales(xs, rs, V, world, 16 if wire == "i16" else 32) if k == "block" else None
    flags = None
    if wire == "i16":
        words = [sref.wire_ref(v, kb, V) if kb is not None else orc.quantize_i16_wire(v, k) for v in vs]
        wsum = np.sum([w.astype(np.int64) for w in words], axis=0).astype(np.int32)
        if kb is not None:
            o16, _, flags = sref.finish_ref(wsum, kb, V)
            full = bref.dequantize(o16, kb, V)
        else:
            o16, _, flags = orc.i16_wire_finish(wsum, k, V)
            full = orc.dequantize_i16(o16, k)
        qs = [_q16_of(w) for w in words]
    else:
        qs = [bref.quantize_i32(v, kb, V) if kb is not None else orc.quantize_i32(v, k) for v in vs]
        total = np.sum([q.astype(np.int64) for q in qs], axis=0)
        qsum = ((total + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32)           # the wrapping int32 SUM
        full = bref.dequantize(qsum, kb, V) if kb is not None else orc.dequantize_i32(qsum, k)
    return full, flags, kb, [_carry(v, q, kb, k, V) for v, q in zip(vs, qs)]


def _check(res, world, n, V, wire, k, steps, data="random"):
    rs = [np.zeros(n, F32) for _ in range(world)]
    inputs = []
    for t in range(steps):
        xs = [bucket(r, t, n, V, k, data) for r in range(world)]
        inputs.append(xs)
        full, flags, kb, rs = _replay_step(xs, rs, wire, k, V)
        for r, d in enumerate(res):
            assert d["lib"][0].endswith(LIB_NAME) and int(d["world"][0]) == world
            sref.same(d[f"full{t}"], full, f"full, step {t}, rank {r}")
            sref.same(d[f"residual{t}"].view(np.uint32), rs[r].view(np.uint32), f"residual, step {t}, rank {r}")
            if flags is not None:
                sref.same(d[f"ovf{t}"], flags, f"flags, step {t}, rank {r}")
            if kb is not None:
                sref.same(d[f"kblk{t}"], kb, f"kblk, step {t}, rank {r}")
        assert all(r.any() for r in rs), t                                  # something was carried
    return inputs


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,V,wire,k,coll,chunks", [(2, 300, 100, "i16", 9, "rs_ag", 1),
                                                         (3, 50_000, 32, "i16", "block", "rs_ag", 1),
                                                         (3, 50_000, 32, "i16", "block", "allreduce", 1),
                                                         (2, 50_000, 32, "i16", 9, "rs_ag", 2),
                                                         (3, 70_001, 256, "i32", "block", "rs_ag", 1)])
def test_sharded_error_feedback_device_kernels(tmp_path, world, n, V, wire, k, coll, chunks):
    """(2, 300, 100): the value-by-value path, with a last shard that is mostly padding.  chunks = 2: each
    chunk's quantise takes its slice of the residual.  The bytes on the wire are the plain step's."""
    res = _run_ranks(tmp_path, world, n, V, wire, k, coll, chunks)
    _check(res, world, n, V, wire, k, 3)
    for d in res:
        assert int(d["scale_bytes"][0]) == (-(-n // V) if k == "block" else 0)
        assert int(d["gather_bytes"][0]) > 0


@pytest.mark.gpu
def test_conservation_is_exact_across_three_ranks_on_the_int16_wire(tmp_path):
    """Inputs on the 2^-(k+8) grid, where every fp32 operation of a step is exact: the sum over steps of
    the aggregate plus the sum over ranks of the residual left is, in float64 and with ==, the sum of
    every input, with no flag set; the first half alone rounds to nothing on every single step."""
    world, n, V, k, T = 3, 4096, 32, 10, 6
    res = _run_ranks(tmp_path, world, n, V, "i16", k, "rs_ag", 1, steps=T, data="grid")
    inputs = _check(res, world, n, V, "i16", k, T, data="grid")
    meant = np.zeros(n, np.float64)
    for xs in inputs:
        for x in xs:
            g = x.astype(np.float64) * 2.0 ** (k + 8)
            assert np.array_equal(g, np.rint(g))
            assert not orc.quantize_i16_wire(x, k)[: n // 2].any()            # without a residual: nothing
            meant += x.astype(np.float64)
    left = sum(d[f"residual{T - 1}"].astype(np.float64) for d in res)
    for d in res:
        sent = sum(d[f"full{t}"].astype(np.float64) for t in range(T))
        assert not any(d[f"ovf{t}"].any() for t in range(T))
        assert np.all(sent + left == meant)
        assert np.any(sent[: n // 2] != 0)
