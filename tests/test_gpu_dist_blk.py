"""k="block" under sharding at world size > 1 with the device kernels: 2, 3 and 8 ranks launched by
torch.distributed.run, all on cuda:0 with a gloo group (as tests/test_gpu_dist.py), every rank's
aggregate, flags and agreed scales bit for bit against the per-block oracle over ALL ranks' buckets
(tests/_blk_ref.py): the scales of all buckets taken together for `world` (layout B: W) summands,
the block-scaled reduce with them, its dequantise -- what one GPU's AUTO reduce gives."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import _blk_ref as ref
from tests._dist_gpu_rank import bucket
from tests.conftest import REPO

LIB_NAME = os.path.basename(os.environ.get("INA_LIBRARY", "libina.so"))
RANK_SCRIPT = os.path.join(REPO, "tests", "_dist_blk_rank.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world, n, wire, V, layout="A", workers=0, collective="rs_ag"):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", RANK_SCRIPT,
           "--size", str(n), "--wire", wire, "--V", str(V), "--out", str(tmp_path),
           "--layout", layout, "--workers", str(workers), "--collective", collective]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{i}.npz"))) for i in range(world)]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got.view(f"u{got.itemsize}"), want.view(f"u{want.itemsize}")), what


def _check(res, bufs, degree, wire, V, n):
    bits = 16 if wire == "i16" else 32
    kb = ref.kblk_ref(bufs, V, degree=degree, bits=bits)
    if wire == "i16":
        want_int, want_ovf = ref.quantize_reduce_i16(bufs, kb, V)
        assert want_ovf.sum() == 1                       # the NaN every bucket carries; the rest clear
    else:
        want_int = ref.quantize_reduce_i32(bufs, kb, V)
    want = ref.dequantize(want_int, kb, V)
    for r, d in enumerate(res):
        assert d["lib"][0].endswith(LIB_NAME)
        _same(d["full"], want, f"full, rank {r}")
        _same(d["kblk"], kb, f"kblk, rank {r}")
        if wire == "i16":
            _same(d["ovf"], want_ovf, f"flags, rank {r}")
        lo, hi = d["range"]
        _same(d["shard"], want_int[lo:hi], f"integer shard, rank {r}")
    return kb


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,V,wire,coll", [(2, 300, 100, "i16", "rs_ag"), (3, 50_000, 32, "i16", "rs_ag"),
                                                 (3, 50_000, 32, "i16", "allreduce"), (8, 200_000, 32, "i16", "a2a"),
                                                 (3, 70_001, 256, "i32", "rs_ag")])
def test_sharded_block_scales_device_kernels(tmp_path, world, n, V, wire, coll):
    """Layout A.  In (2, 300, 100) the last rank's shard is padding beyond its first 44 values and
    the scale array must cover the padded bucket for its slice to exist."""
    res = _run_ranks(tmp_path, world, n, wire, V, collective=coll)
    _check(res, [bucket(r, n, wire) for r in range(world)], world, wire, V, n)
    for d in res:
        assert int(d["world"][0]) == world
        gb, shard = (int(v) for v in d["gather_bytes"])
        assert shard % V == 0
        per = 4 * shard if wire == "i32" or coll == "allreduce" else 2 * shard + shard // V
        assert gb == (world - 1) * per                   # the gather carries no scales
        assert int(d["scale_bytes"][0]) == -(-n // V)


@pytest.mark.gpu
def test_range_layout_b_block_scales_device_kernels(tmp_path):
    world, n, V, W = 3, 50_000, 32, 4
    res = _run_ranks(tmp_path, world, n, "i16", V, layout="B", workers=W)
    _check(res, [bucket(w, n, "i16") for w in range(W)], W, "i16", V, n)
    for d in res:
        gb, shard = (int(v) for v in d["gather_bytes"])  # int16 sums + flags + scales gathered
        assert gb == (world - 1) * (2 * shard + 2 * (shard // V))
        assert int(d["scale_bytes"][0]) == 0


@pytest.mark.gpu
def test_rccl_world1_block_scale_collectives_on_this_image():
    """all_reduce(int8, MIN) -- agree_block_scales' call -- and the int8 all-gather through RCCL
    itself (backend nccl, one rank), so the calls are known to exist on this ROCm / RCCL image."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}",
           os.path.join(REPO, "tests", "_rccl_world1_blk.py")]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "rccl world-1 block-scale collectives ok" in r.stdout
