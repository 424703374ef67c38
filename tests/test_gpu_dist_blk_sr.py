"""dist.BlockStochasticAggregator and dist.BlockStochasticRangeAggregator with the device kernels: 1 rank and
2 ranks launched by torch.distributed.run, all on cuda:0 with a gloo group (as tests/test_gpu_dist_sr.py),
n = 5,000, V = 32, both wires on every collective, float32, bfloat16 and float16 buckets.  After every step
each rank's aggregate, flags and scales equal, bit for bit, a numpy replay of all ranks together: each
rank's scales for `world` summands under the stochastic rule (tests/_blk_sr_ref.py), their MIN, each
rank's bucket rounded on stream `rank` at the step's number, the words' wrapping sum, the block decode.
The result depends on the step; setting .step back reproduces it; and the range aggregator's integers,
flags and scales equal the sharded aggregator's shard."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import _blk_ref as bref
from tests import _blk_sr_ref as bsr
from tests import _shard_blk_ref as shref
from tests._dist_blk_sr_rank import CASES, SEED, bucket
from tests.conftest import REPO

LIB_NAME = os.path.basename(os.environ.get("INA_LIBRARY", "libina.so"))
RANK_SCRIPT = os.path.join(REPO, "tests", "_dist_blk_sr_rank.py")
N, V = 5000, 32


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", RANK_SCRIPT,
           "--size", str(N), "--V", str(V), "--out", str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)     # this launch's own limit
    assert r.returncode == 0, r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{i}.npz"))) for i in range(world)]


def _replay_step(xs, t, wire):
    """All ranks' widened buckets of step t -> (full, flags or None, agreed scales)."""
    world = len(xs)
    kb = np.min([bsr.kblk_ref([x], V, world, 32 if wire == "i32" else 16) for x in xs], axis=0).astype(np.int8)
    if wire == "i16":
        words = [bsr.quantize_i16_wire(x, kb, V, SEED, step=t, sub=r) for r, x in enumerate(xs)]
        wsum = np.sum([w.astype(np.int64) for w in words], axis=0).astype(np.int32)
        o16, _, flags = shref.finish_ref(wsum, kb, V)
        return bref.dequantize(o16, kb, V), flags, kb
    qs = [bsr.quantize(x, kb, V, SEED, step=t, sub=r) for r, x in enumerate(xs)]
    total = np.sum([q.astype(np.int64) for q in qs], axis=0)
    qsum = ((total + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32)               # the wrapping int32 SUM
    return bref.dequantize(qsum, kb, V), None, kb


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2])
def test_block_stochastic_aggregators_device_kernels(tmp_path, world):
    res = _run_ranks(tmp_path, world)
    for c, (wire, coll, dtype) in enumerate(CASES):
        fulls = []
        for t in (0, 1):
            xs = [bucket(r, t, N, V, dtype).float().numpy() for r in range(world)]
            full, flags, kb = _replay_step(xs, t, wire)
            fulls.append(full)
            for r, d in enumerate(res):
                what = (wire, coll, dtype, t, r)
                assert d["lib"][0].endswith(LIB_NAME) and int(d["world"][0]) == world
                assert np.array_equal(d[f"c{c}_kblk{t}"], kb), what
                assert np.array_equal(d[f"c{c}_full{t}"].view(np.uint32), full.view(np.uint32)), what
                if flags is not None:
                    assert np.array_equal(d[f"c{c}_ovf{t}"], flags), what
            if t == 1:
                assert flags is None or flags.any()                          # the NaN and the inf of step 1
        # the step is part of the random stream: step 0's bucket at step 1 gives other bits (seen on the int16
        # wire; at 32 bits a quantum lies below the float32 aggregate's last place and the decode hides it)
        if wire == "i16":
            xs0 = [bucket(r, 0, N, V, dtype).float().numpy() for r in range(world)]
            assert not np.array_equal(_replay_step(xs0, 1, wire)[0], fulls[0])
        for r, d in enumerate(res):
            what = (wire, coll, dtype, r)
            assert np.array_equal(d[f"c{c}_full_redo1"].view(np.uint32), fulls[1].view(np.uint32)), what   # .step = 1
            assert np.array_equal(d[f"c{c}_kblk_redo1"], d[f"c{c}_kblk1"]), what
            if wire == "i16":
                assert np.array_equal(d[f"c{c}_ovf_redo1"], d[f"c{c}_ovf1"]), what
            gather, scale = (int(v) for v in d[f"c{c}_bytes"])
            assert (gather > 0 and scale == -(-N // V)) if world > 1 else (gather == 0 and scale == 0), what
            # layouts A and B: the same integers, flags and scales on this rank's range
            assert d[f"c{c}_range_int"].size > 0 and d[f"c{c}_range_int"].any(), what
            assert np.array_equal(d[f"c{c}_range_int"], d[f"c{c}_shard_int"]), what
            assert np.array_equal(d[f"c{c}_range_k"], d[f"c{c}_shard_k"]), what
            if wire == "i16":
                assert np.array_equal(d[f"c{c}_range_ovf"], d[f"c{c}_shard_ovf"]), what
                assert d[f"c{c}_range_int"].dtype == np.int16
