"""One rank of the stochastic-rounding sharded-aggregation GPU test (tests/test_gpu_dist_sr.py), launched
by torch.distributed.run like tests/_dist_ef_rank.py: every rank on cuda:0, a gloo group (the collectives
stage through host memory), the device kernels through libina.so.
ShardedAggregator(rounding="stochastic") over T steps on seeded per-rank, per-step buckets; after each
step it keeps full and the flags (i16 wire); then it sets .step back to 1 and repeats that step.  All of
it goes with the library path to OUT/rank<r>.npz."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-training-ina_amd"))
sys.path.insert(0, REPO)

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
SEED = 0x5EED0000CAFE


def bucket(rank: int, step: int, n: int, k: int, dtype: str) -> torch.Tensor:
    """Rank `rank`'s bucket of step `step` as a CPU tensor of `dtype`: values a few units of the int16
    range at k, where single ranks and the sum clip, half of them scaled down below one quantum (what
    round-to-nearest would drop).  One NaN and one inf in step 1."""
    rng = np.random.default_rng(7000 + 100 * rank + step)
    x = (rng.standard_normal(n) * 0.25 * 32767.0 * 2.0 ** -k).astype(np.float32)
    x[::2] *= np.float32(2.0 ** -18)               # |t| of about 0.03
    if step == 1 and n > 16:
        x[7 + rank] = np.nan
        x[n - 3 - rank] = np.inf
    return torch.from_numpy(x).to(DTYPES[dtype])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--wire", choices=("i32", "i16"), required=True)
    ap.add_argument("--k", type=int, required=True)
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", required=True)
    ap.add_argument("--collective", choices=("rs_ag", "a2a", "allreduce"), default="rs_ag")
    ap.add_argument("--chunks", type=int, default=1)
    ap.add_argument("--dtype", choices=tuple(DTYPES), default="float32")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    from ina_amd import _lib
    from ina_amd.dist import ShardedAggregator
    dev = torch.device("cuda", 0)
    agg = ShardedAggregator(a.size, k=a.k, device=dev, wire=a.wire, V=a.V, collective=a.collective, chunks=a.chunks,
                            rounding="stochastic", seed=SEED)
    res = {"world": np.array([world]), "lib": np.array([os.path.realpath(_lib.LIB_PATH)]),
           "gather_bytes": np.array([agg.gather_bytes])}

    def step(t, tag):
        assert agg.step == t
        full = agg(bucket(rank, t, a.size, a.k, a.dtype).to(dev))
        torch.cuda.synchronize()
        res[f"full{tag}"] = full.cpu().numpy()
        if a.wire == "i16":
            res[f"ovf{tag}"] = agg.overflow.cpu().numpy()

    for t in range(a.steps):
        step(t, t)
    assert agg.step == a.steps
    agg.step = 1                                   # a resumed job: step 1 again, bit for bit
    step(1, "_redo1")
    np.savez(os.path.join(a.out, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
