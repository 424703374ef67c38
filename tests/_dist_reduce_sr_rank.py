"""One rank of the two-layouts stochastic-rounding GPU test (tests/test_gpu_dist_reduce_sr.py), launched by
torch.distributed.run like tests/_dist_sr_rank.py: every rank on cuda:0, a gloo group, the device kernels
through libina.so.
Every rank builds all W = world workers' seeded buckets of a step (tests/_dist_sr_rank.py's).  Layout B:
StochasticRangeAggregator on the W slices of this rank's range.  Layout A: ShardedAggregator(rounding=
"stochastic") on this rank's own bucket, the same seed.  After each of T steps it keeps both layouts'
`full` and flags (i16 wire) and asserts they are bit-identical; all of it goes with the library path to
OUT/rank<r>.npz."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-training-ina_amd"))
sys.path.insert(0, REPO)

from tests._dist_sr_rank import DTYPES, SEED, bucket  # noqa: E402

ALIGN = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--wire", choices=("i32", "i16"), required=True)
    ap.add_argument("--k", type=int, required=True)
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out", required=True)
    ap.add_argument("--dtype", choices=tuple(DTYPES), default="float32")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    from ina_amd import _lib
    from ina_amd.dist import ShardedAggregator, StochasticRangeAggregator
    dev = torch.device("cuda", 0)
    kw = dict(k=a.k, device=dev, align=ALIGN, wire=a.wire, V=a.V, seed=SEED)
    lay_b = StochasticRangeAggregator(a.size, **kw)
    lay_a = ShardedAggregator(a.size, rounding="stochastic", **kw)
    lo, hi = lay_b.range
    assert (lo, hi) == lay_a.plan.range_of(rank) and lo % 4 == 0 and lo % a.V == 0
    res = {"world": np.array([world]), "lib": np.array([os.path.realpath(_lib.LIB_PATH)]), "range": np.array([lo, hi])}
    for t in range(a.steps):
        assert lay_a.step == lay_b.step == t
        xs = [bucket(w, t, a.size, a.k, a.dtype) for w in range(world)]
        fb = lay_b([x[lo:hi].contiguous().to(dev) for x in xs])
        fa = lay_a(xs[rank].to(dev))
        torch.cuda.synchronize()
        assert torch.equal(fa.view(torch.int32), fb.view(torch.int32)), f"step {t}: the layouts differ"
        res[f"full_a{t}"], res[f"full_b{t}"] = fa.cpu().numpy(), fb.cpu().numpy()
        if a.wire == "i16":
            assert torch.equal(lay_a.overflow, lay_b.overflow), f"step {t}: the layouts' flags differ"
            res[f"ovf_a{t}"], res[f"ovf_b{t}"] = lay_a.overflow.cpu().numpy(), lay_b.overflow.cpu().numpy()
    np.savez(os.path.join(a.out, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
