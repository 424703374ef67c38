"""The two layouts of config 5 under stochastic rounding at world size > 1 (include/ina_reduce_sr.h,
"Layouts"): 2 and 3 ranks launched by torch.distributed.run, all on cuda:0 with a gloo group (as
tests/test_gpu_dist_sr.py).  Every rank runs StochasticRangeAggregator on the W = world slices of its
range and ShardedAggregator(rounding="stochastic") on its own bucket, the same seed, two steps.  `full`
and the int16 wire's flags are bit-identical between the two layouts on every rank, and equal the numpy
replay of tests/_sr_reduce_ref.py over all workers' whole buckets (sub = 0, the step's number, e0 = 0)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from tests import _sr_reduce_ref as rref
from tests._dist_sr_rank import SEED, bucket
from tests.conftest import REPO

LIB_NAME = os.path.basename(os.environ.get("INA_LIBRARY", "libina.so"))
RANK_SCRIPT = os.path.join(REPO, "tests", "_dist_reduce_sr_rank.py")
T = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world, n, V, wire, k, dtype):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", RANK_SCRIPT,
           "--size", str(n), "--wire", wire, "--k", str(k), "--V", str(V), "--steps", str(T), "--out", str(tmp_path),
           "--dtype", dtype]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{i}.npz"))) for i in range(world)]


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,V,wire,k,dtype", [(3, 5000, 32, "i32", 9, "float32"),
                                                    (2, 5000, 32, "i16", 9, "float32"),
                                                    (3, 5000, 32, "i16", 9, "bfloat16")])
def test_the_two_layouts_agree_and_follow_the_replay(tmp_path, world, n, V, wire, k, dtype):
    res = _run_ranks(tmp_path, world, n, V, wire, k, dtype)
    assert sorted(tuple(d["range"]) for d in res)[0][0] == 0 and max(d["range"][1] for d in res) == n
    fulls = []
    for t in range(T):
        xs = [bucket(w, t, n, k, dtype).float().numpy() for w in range(world)]
        if wire == "i32":
            full, flags = orc.dequantize_i32(rref.quantize_reduce(xs, k, SEED, step=t), k), None
        else:
            s16, flags = rref.quantize_reduce_i16(xs, k, V, SEED, step=t)
            full = orc.dequantize_i16(s16, k)
        fulls.append(full)
        for r, d in enumerate(res):
            assert d["lib"][0].endswith(LIB_NAME) and int(d["world"][0]) == world
            for lay in "ab":
                assert np.array_equal(d[f"full_{lay}{t}"].view(np.uint32), full.view(np.uint32)), (t, r, lay)
                if flags is not None:
                    assert np.array_equal(d[f"ovf_{lay}{t}"], flags), (t, r, lay)
        if t == 1:
            assert flags is None or (flags.any() and not flags.all())            # the NaN and the inf of step 1
    assert not np.array_equal(fulls[0], fulls[1])
