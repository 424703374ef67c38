"""One rank of the block-scaled sharded-aggregation GPU test (tests/test_gpu_dist_blk.py), launched by
torch.distributed.run like tests/_dist_gpu_rank.py: every rank on cuda:0, a gloo group (the
collectives, the MIN of the block scales included, stage through host memory), the device kernels
through libina.so.  ShardedAggregator (layout A) or RangeAggregator (layout B) with k="block";
writes full, the flags, the scales, its integer shard and range, gather_bytes, scale_bytes and the
library path to OUT/rank<r>.npz."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-training-ina_amd"))
sys.path.insert(0, REPO)

from tests._dist_gpu_rank import bucket  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--wire", choices=("i32", "i16"), required=True)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out", required=True)
    ap.add_argument("--layout", choices=("A", "B"), default="A")
    ap.add_argument("--workers", type=int, default=0, help="layout B: W buckets (default: world)")
    ap.add_argument("--collective", choices=("rs_ag", "a2a", "allreduce"), default="rs_ag")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    from ina_amd import _lib
    from ina_amd.dist import RangeAggregator, ShardedAggregator
    dev = torch.device("cuda", 0)
    if a.layout == "A":
        x = torch.from_numpy(bucket(rank, a.size, a.wire)).to(dev)
        agg = ShardedAggregator(a.size, k="block", device=dev, wire=a.wire, V=a.V, collective=a.collective)
    else:                                      # every worker's slice of this rank's range
        agg = RangeAggregator(a.size, k="block", device=dev, wire=a.wire, V=a.V)
        lo, hi = agg.range
        x = [torch.from_numpy(bucket(w, a.size, a.wire)[lo:hi].copy()).to(dev)
             for w in range(a.workers or world)]
    for _ in range(a.steps):                   # buffers are reused across calls
        full = agg(x)
    torch.cuda.synchronize()
    res = {"full": full.cpu().numpy(), "world": np.array([world]), "kblk": agg.kblk.cpu().numpy(),
           "gather_bytes": np.array([agg.gather_bytes, agg.plan.shard]), "scale_bytes": np.array([agg.scale_bytes])}
    if a.wire == "i16":
        res["ovf"] = agg.overflow.cpu().numpy()
    shard = agg.aggregate_int(x)
    torch.cuda.synchronize()
    lo, hi = agg.plan.range_of(rank)
    res["shard"] = shard[: hi - lo].cpu().numpy()
    res["range"] = np.array([lo, hi])
    res["lib"] = np.array([os.path.realpath(_lib.LIB_PATH)])
    np.savez(os.path.join(a.out, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
