"""One rank of the block-scaled stochastic-rounding aggregation GPU test (tests/test_gpu_dist_blk_sr.py),
launched by torch.distributed.run like tests/_dist_sr_rank.py: every rank on cuda:0, a gloo group (the
collectives stage through host memory), the device kernels through libina.so.
For every case of CASES: BlockStochasticAggregator over two steps on seeded per-rank, per-step buckets
(full, flags and scales kept after each), .step set back to 1 and that step repeated, then step 1 once
more as aggregate_int next to BlockStochasticRangeAggregator.aggregate_int at step 1 over all ranks'
slices of this rank's range.  All of it goes with the library path to OUT/rank<r>.npz."""
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
SEED = 0xB10C5EED0000CAFE
# (wire, collective, bucket dtype): both wires on every collective, a bf16 bucket on each wire
CASES = (("i32", "rs_ag", "float32"), ("i16", "rs_ag", "bfloat16"), ("i32", "a2a", "bfloat16"),
         ("i16", "a2a", "float32"), ("i32", "allreduce", "float32"), ("i16", "allreduce", "float16"))


def bucket(rank: int, step: int, n: int, V: int, dtype: str) -> torch.Tensor:
    """Rank `rank`'s bucket of step `step` as a CPU tensor of `dtype`: block magnitudes log-uniform over
    five decades (neighbouring blocks carry different scales).  One NaN and one inf in step 1."""
    rng = np.random.default_rng(9000 + 100 * rank + step)
    nblk = -(-n // V)
    mag = np.repeat(10.0 ** rng.uniform(-4.0, 1.0, nblk), V)[:n]
    x = (rng.standard_normal(n) * mag).astype(np.float32)
    if step == 1 and n > 16:
        x[7 + rank] = np.nan
        x[n - 3 - rank] = np.inf
    return torch.from_numpy(x).to(DTYPES[dtype])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--V", type=int, default=32)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    from ina_amd import _lib
    from ina_amd.dist import BlockStochasticAggregator, BlockStochasticRangeAggregator
    dev = torch.device("cuda", 0)
    n, V = a.size, a.V
    res = {"world": np.array([world]), "lib": np.array([os.path.realpath(_lib.LIB_PATH)])}
    for c, (wire, coll, dtype) in enumerate(CASES):
        agg = BlockStochasticAggregator(n, device=dev, wire=wire, V=V, collective=coll, seed=SEED)
        res[f"c{c}_bytes"] = np.array([agg.gather_bytes, agg.scale_bytes])

        def step(t, tag):
            assert agg.step == t
            full = agg(bucket(rank, t, n, V, dtype).to(dev))
            torch.cuda.synchronize()
            res[f"c{c}_full{tag}"] = full.cpu().numpy()
            res[f"c{c}_kblk{tag}"] = agg.kblk.cpu().numpy()
            if wire == "i16":
                res[f"c{c}_ovf{tag}"] = agg.overflow.cpu().numpy()

        step(0, 0)
        step(1, 1)
        assert agg.step == 2
        agg.step = 1                                   # a resumed job: step 1 again, bit for bit
        step(1, "_redo1")
        # the two layouts at step 1: this rank's integer shard of the sharded step, and the fused AUTO
        # reduce over every rank's slice of the same range
        agg.step = 1
        shard = agg.aggregate_int(bucket(rank, 1, n, V, dtype).to(dev))
        rag = BlockStochasticRangeAggregator(n, device=dev, wire=wire, V=V, seed=SEED)
        assert rag.plan.shard == agg.plan.shard and rag.range == agg.plan.range_of(rank)
        lo, hi = rag.range
        rag.step = 1
        mine = rag.aggregate_int([bucket(r, 1, n, V, dtype)[lo:hi].to(dev) for r in range(world)])
        assert rag.step == 2
        torch.cuda.synchronize()
        m, nb = hi - lo, -(-(hi - lo) // V)
        res[f"c{c}_shard_int"] = shard[:m].cpu().numpy()
        res[f"c{c}_range_int"] = mine.cpu().numpy()
        res[f"c{c}_shard_k"] = agg._kshard()[:nb].cpu().numpy()
        res[f"c{c}_range_k"] = rag.k_shard[:nb].cpu().numpy()
        if wire == "i16":
            res[f"c{c}_shard_ovf"] = agg.ovf_shard[:nb].cpu().numpy()
            res[f"c{c}_range_ovf"] = rag.ovf_shard[:nb].cpu().numpy()
    np.savez(os.path.join(a.out, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
