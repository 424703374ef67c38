"""bf16 / fp16 buckets under both aggregators at world size > 1 with the device kernels: 2 and 3 ranks
launched by torch.distributed.run, all on cuda:0 with a gloo group (as tests/test_gpu_dist_ef.py), one
step on seeded per-rank 16-bit buckets.  Every rank's aggregate, flags and agreed scales equal, bit for
bit, a numpy replay of all ranks together on the WIDENED buckets (.float(), exact): the MIN of the ranks'
scales (_blk_ref.kblk_ref over all ranks' buckets), the oracle's wires, their int64 sum cast to int32, the
oracle's finish and decode -- and, where out_dtype is 16-bit, that fp32 aggregate rounded once to nearest
even (torch's CPU conversion)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _blk_ref as bref
from tests import _shard_blk_ref as sref
from tests._dist_x16_rank import DTYPES, bucket
from tests.conftest import REPO

LIB_NAME = os.path.basename(os.environ.get("INA_LIBRARY", "libina.so"))
RANK_SCRIPT = os.path.join(REPO, "tests", "_dist_x16_rank.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world, n, V, wire, k, coll, chunks, dtype, out_dtype, workers=0):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", RANK_SCRIPT,
           "--size", str(n), "--wire", wire, "--k", str(k), "--V", str(V), "--out", str(tmp_path),
           "--collective", coll, "--chunks", str(chunks), "--dtype", dtype, "--out-dtype", out_dtype,
           "--workers", str(workers)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{i}.npz"))) for i in range(world)]


def _replay(xs, wire, k, V, fused=False):
    """The summands' widened buckets -> (fp32 aggregate, flags or None, kblk or None).  fused: layout B,
    where one GPU holds all the summands of a block and runs the fused int16 quantise + reduce."""
    kb = bref.kblk_ref(xs, V, degree=len(xs), bits=16 if wire == "i16" else 32) if k == "block" else None
    flags = None
    if wire == "i16" and fused:
        o16, flags = bref.quantize_reduce_i16(xs, kb, V) if kb is not None else orc.quantize_reduce_i16_sat(xs, k, V)
        full = bref.dequantize(o16, kb, V) if kb is not None else orc.dequantize_i16(o16, k)
    elif wire == "i16":
        words = [sref.wire_ref(x, kb, V) if kb is not None else orc.quantize_i16_wire(x, k) for x in xs]
        wsum = np.sum([w.astype(np.int64) for w in words], axis=0).astype(np.int32)
        if kb is not None:
            o16, _, flags = sref.finish_ref(wsum, kb, V)
            full = bref.dequantize(o16, kb, V)
        else:
            o16, _, flags = orc.i16_wire_finish(wsum, k, V)
            full = orc.dequantize_i16(o16, k)
    else:
        qs = [bref.quantize_i32(x, kb, V) if kb is not None else orc.quantize_i32(x, k) for x in xs]
        total = np.sum([q.astype(np.int64) for q in qs], axis=0)
        qsum = ((total + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32)           # the wrapping int32 SUM
        full = bref.dequantize(qsum, kb, V) if kb is not None else orc.dequantize_i32(qsum, k)
    return full, flags, kb


def _check(res, summands, n, V, wire, k, dtype, out_dtype, fused=False):
    xs = [bucket(w, n, V, k, dtype).float().numpy() for w in range(summands)]
    full, flags, kb = _replay(xs, wire, k, V, fused)
    want = torch.from_numpy(full).to(DTYPES[out_dtype])                     # fp32: unchanged; else one rounding
    want_bits = want.view({2: torch.int16, 4: torch.int32}[want.element_size()]).numpy()
    for r, d in enumerate(res):
        assert d["lib"][0].endswith(LIB_NAME) and int(d["world"][0]) == len(res)
        sref.same(d["full_bits"], want_bits, f"full, rank {r}")
        if flags is not None:
            sref.same(d["ovf"], flags, f"flags, rank {r}")
            assert flags.any()
        if kb is not None:
            sref.same(d["kblk"], kb, f"kblk, rank {r}")


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,V,wire,k,coll,chunks,dtype,out_dtype",
                         [(2, 300, 100, "i16", 9, "rs_ag", 1, "bf16", "fp32"),
                          (3, 50_000, 32, "i16", "block", "rs_ag", 1, "bf16", "bf16"),
                          (3, 50_000, 32, "i16", "block", "allreduce", 1, "fp16", "fp16"),
                          (2, 50_000, 32, "i16", 9, "rs_ag", 2, "bf16", "bf16")])
def test_sharded_16_bit_buckets_device_kernels(tmp_path, world, n, V, wire, k, coll, chunks, dtype, out_dtype):
    """(2, 300, 100): the value-by-value path, with a last shard that is mostly padding, and the fp32
    aggregate of a bf16 bucket.  allreduce: the 16-bit y of the block finish over the whole bucket.
    chunks = 2: the chunked loop's quantise and expand follow the bucket's and out_dtype's types."""
    res = _run_ranks(tmp_path, world, n, V, wire, k, coll, chunks, dtype, out_dtype)
    _check(res, world, n, V, wire, k, dtype, out_dtype)


@pytest.mark.gpu
def test_int32_wire_gathers_two_bytes_a_value(tmp_path):
    """bf16 -> bf16 on the i32 wire: the owner decodes its shard into bf16 and the all-gather carries it;
    gather_bytes is half that of the same job with out_dtype float32 (3 ranks, shards of 23,552 values:
    2 x 23,552 x 2 bytes)."""
    world, n, V, k = 3, 70_001, 256, 9
    res = _run_ranks(tmp_path, world, n, V, "i32", k, "rs_ag", 1, "bf16", "bf16")
    _check(res, world, n, V, "i32", k, "bf16", "bf16")
    for d in res:
        assert int(d["gather_bytes"][0]) == 2 * 23_552 * 2
        assert int(d["gather_bytes_fp32_out"][0]) == 2 * int(d["gather_bytes"][0])


@pytest.mark.gpu
def test_range_aggregator_16_bit_slices(tmp_path):
    """Layout B, 2 ranks, W = 3 workers' fp16 slices, block scales on the int16 wire, fp16 out."""
    world, n, V, W = 2, 300, 32, 3
    res = _run_ranks(tmp_path, world, n, V, "i16", "block", "rs_ag", 1, "fp16", "fp16", workers=W)
    _check(res, W, n, V, "i16", "block", "fp16", "fp16", fused=True)
