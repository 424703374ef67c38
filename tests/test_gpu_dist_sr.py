"""ShardedAggregator(rounding="stochastic") at world size > 1 with the device kernels: 2 and 3 ranks
launched by torch.distributed.run, all on cuda:0 with a gloo group (as tests/test_gpu_dist_ef.py), T = 3
steps on seeded per-rank, per-step buckets.  After every step each rank's aggregate and flags equal, bit
for bit, a numpy replay of all ranks together: each rank's bucket rounded by tests/_sr_ref.py with
sub = rank and the step's number, the words' int64 sum cast to int32, the oracle's finish and decode.
Setting .step back reproduces that step."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import _sr_ref as sref
from tests._dist_sr_rank import SEED, bucket
from tests.conftest import REPO

LIB_NAME = os.path.basename(os.environ.get("INA_LIBRARY", "libina.so"))
RANK_SCRIPT = os.path.join(REPO, "tests", "_dist_sr_rank.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world, n, V, wire, k, coll, chunks, dtype, steps=3):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", RANK_SCRIPT,
           "--size", str(n), "--wire", wire, "--k", str(k), "--V", str(V), "--steps", str(steps), "--out", str(tmp_path),
           "--collective", coll, "--chunks", str(chunks), "--dtype", dtype]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{i}.npz"))) for i in range(world)]


def _replay_step(xs, t, wire, k, V):
    """All ranks' widened buckets of step t -> (full, flags or None)."""
    if wire == "i16":
        words = [sref.quantize_i16_wire(x, k, SEED, step=t, sub=r) for r, x in enumerate(xs)]
        wsum = np.sum([w.astype(np.int64) for w in words], axis=0).astype(np.int32)
        o16, _, flags = orc.i16_wire_finish(wsum, k, V)
        return orc.dequantize_i16(o16, k), flags
    qs = [sref.quantize(x, k, SEED, step=t, sub=r) for r, x in enumerate(xs)]
    total = np.sum([q.astype(np.int64) for q in qs], axis=0)
    qsum = ((total + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32)               # the wrapping int32 SUM
    return orc.dequantize_i32(qsum, k), None


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,V,wire,k,coll,chunks,dtype", [(2, 300, 100, "i16", 9, "rs_ag", 1, "float32"),
                                                               (3, 50_000, 32, "i16", 9, "allreduce", 1, "float32"),
                                                               (3, 70_001, 256, "i32", 9, "rs_ag", 1, "float32"),
                                                               (2, 50_000, 32, "i16", 9, "rs_ag", 2, "float32"),
                                                               (3, 50_000, 32, "i16", 9, "rs_ag", 1, "bfloat16")])
def test_sharded_stochastic_rounding_device_kernels(tmp_path, world, n, V, wire, k, coll, chunks, dtype):
    """(2, 300, 100): the value-by-value path, with a last shard that is mostly padding.  chunks = 2: each
    chunk's quantise passes its offset as e0, so the bytes are those of chunks = 1.  bfloat16: the bucket
    is read as it is, where error feedback refuses it."""
    T = 3
    res = _run_ranks(tmp_path, world, n, V, wire, k, coll, chunks, dtype, steps=T)
    fulls = []
    for t in range(T):
        xs = [bucket(r, t, n, k, dtype).float().numpy() for r in range(world)]
        full, flags = _replay_step(xs, t, wire, k, V)
        fulls.append(full)
        for r, d in enumerate(res):
            assert d["lib"][0].endswith(LIB_NAME) and int(d["world"][0]) == world
            assert np.array_equal(d[f"full{t}"].view(np.uint32), full.view(np.uint32)), (t, r)
            if flags is not None:
                assert np.array_equal(d[f"ovf{t}"], flags), (t, r)
        if t == 1:
            assert flags is None or flags.any()                              # the NaN and the inf of step 1
        # the small half is below half a quantum on every rank: nearest sends none of it, this does
        near = orc.quantize_i32(xs[0], k)[::2]
        assert not near[np.isfinite(xs[0][::2])].any() and np.any(full[::2][np.isfinite(full[::2])] != 0)
    assert not np.array_equal(fulls[0], fulls[2])
    for r, d in enumerate(res):                                              # .step = 1 repeated step 1
        assert np.array_equal(d["full_redo1"].view(np.uint32), fulls[1].view(np.uint32)), r
        if wire == "i16":
            assert np.array_equal(d["ovf_redo1"], d["ovf1"]), r
        assert int(d["gather_bytes"][0]) > 0
