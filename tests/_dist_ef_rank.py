"""One rank of the error-feedback sharded-aggregation GPU test (tests/test_gpu_dist_ef.py), launched by
torch.distributed.run like tests/_dist_blk_rank.py: every rank on cuda:0, a gloo group (the
collectives, the MIN of the block scales included, stage through host memory), the device kernels
through libina.so.  ShardedAggregator(error_feedback=True) over T steps on seeded per-rank, per-step
buckets; after each step it keeps full, residual, the flags (i16 wire) and the agreed scales
(k="block"), and writes them with the library path to OUT/rank<r>.npz."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-training-ina_amd"))
sys.path.insert(0, REPO)

from tests import _blk_ref as bref  # noqa: E402


def bucket(rank: int, step: int, n: int, V: int, k, data: str) -> np.ndarray:
    """Rank `rank`'s bucket of step `step`.  data="grid": m * 2^-(k+8) with |m| < 128 on the first half
    and |m| < 2^15 on the second (every fp32 operation of a step is exact).  Otherwise: k="block":
    _blk_ref.bucket (neighbouring blocks carry different k); an integer k: values a few units of the
    int16 range at k, where single ranks and the sum clip.  One NaN and one inf in step 1."""
    rng = np.random.default_rng(5000 + 100 * rank + step)
    if data == "grid":
        m = np.concatenate([rng.integers(-127, 128, n // 2), rng.integers(-(2**15) + 1, 2**15, n - n // 2)])
        return (m * 2.0 ** -(k + 8)).astype(np.float32)
    if k == "block":
        x = bref.bucket(rng, 1, n, V)[0]
    else:
        x = (rng.standard_normal(n) * 0.25 * 32767.0 * 2.0 ** -k).astype(np.float32)
    if step == 1 and n > 16:
        x[7 + rank] = np.nan
        x[n - 3 - rank] = np.inf
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--wire", choices=("i32", "i16"), required=True)
    ap.add_argument("--k", required=True, help="an integer, or 'block'")
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", required=True)
    ap.add_argument("--collective", choices=("rs_ag", "a2a", "allreduce"), default="rs_ag")
    ap.add_argument("--chunks", type=int, default=1)
    ap.add_argument("--data", choices=("random", "grid"), default="random")
    a = ap.parse_args()
    k = a.k if a.k == "block" else int(a.k)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    from ina_amd import _lib
    from ina_amd.dist import ShardedAggregator
    dev = torch.device("cuda", 0)
    agg = ShardedAggregator(a.size, k=k, device=dev, wire=a.wire, V=a.V, collective=a.collective, chunks=a.chunks,
                            error_feedback=True)
    res = {"world": np.array([world]), "lib": np.array([os.path.realpath(_lib.LIB_PATH)]),
           "gather_bytes": np.array([agg.gather_bytes]), "scale_bytes": np.array([agg.scale_bytes])}
    for t in range(a.steps):
        full = agg(torch.from_numpy(bucket(rank, t, a.size, a.V, k, a.data)).to(dev))
        torch.cuda.synchronize()
        res[f"full{t}"] = full.cpu().numpy()
        res[f"residual{t}"] = agg.residual.cpu().numpy()
        if a.wire == "i16":
            res[f"ovf{t}"] = agg.overflow.cpu().numpy()
        if k == "block":
            res[f"kblk{t}"] = agg.kblk.cpu().numpy()
    np.savez(os.path.join(a.out, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
