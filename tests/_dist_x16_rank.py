"""One rank of the bf16 / fp16 sharded-aggregation GPU test (tests/test_gpu_dist_x16.py), launched by
torch.distributed.run like tests/_dist_ef_rank.py: every rank on cuda:0, a gloo group (the collectives,
the MIN of the block scales included, stage through host memory), the device kernels through libina.so.
One step of ShardedAggregator (layout A) on this rank's seeded 16-bit bucket, or of RangeAggregator
(layout B) on the W workers' slices of this rank's range; writes full (as its bits), the flags (i16 wire),
the scales (k="block"), gather_bytes (layout A: also that of the same job with out_dtype float32) and the
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

from tests import _blk_ref as bref  # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def bucket(who: int, n: int, V: int, k, dtype: str) -> torch.Tensor:
    """Rank (layout A) or worker (layout B) `who`'s bucket, a CPU tensor of the 16-bit type; .float() of
    it is exact.  k="block": _blk_ref.bucket (neighbouring blocks carry different k); an integer k: values
    a few units of the int16 range at k, where single ranks and the sum clip.  One NaN and one inf."""
    rng = np.random.default_rng(7000 + 100 * who)
    if k == "block":
        x = bref.bucket(rng, 1, n, V)[0]
    else:
        x = (rng.standard_normal(n) * 0.25 * 32767.0 * 2.0 ** -k).astype(np.float32)
    t = torch.from_numpy(x).to(DTYPES[dtype])
    if n > 16:
        t[7 + who] = float("nan")
        t[n - 3 - who] = float("inf")
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--wire", choices=("i32", "i16"), required=True)
    ap.add_argument("--k", required=True, help="an integer, or 'block'")
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--out", required=True)
    ap.add_argument("--collective", choices=("rs_ag", "a2a", "allreduce"), default="rs_ag")
    ap.add_argument("--chunks", type=int, default=1)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), required=True)
    ap.add_argument("--out-dtype", choices=tuple(DTYPES), required=True)
    ap.add_argument("--workers", type=int, default=0, help="> 0: RangeAggregator over that many workers' slices")
    a = ap.parse_args()
    k = a.k if a.k == "block" else int(a.k)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    from ina_amd import _lib
    from ina_amd.dist import RangeAggregator, ShardedAggregator
    dev = torch.device("cuda", 0)
    if a.workers:
        agg = RangeAggregator(a.size, k=k, device=dev, wire=a.wire, V=a.V, out_dtype=DTYPES[a.out_dtype])
        lo, hi = agg.range
        full = agg([bucket(w, a.size, a.V, k, a.dtype)[lo:hi].contiguous().to(dev) for w in range(a.workers)])
    else:
        agg = ShardedAggregator(a.size, k=k, device=dev, wire=a.wire, V=a.V, collective=a.collective,
                                chunks=a.chunks, out_dtype=DTYPES[a.out_dtype])
        full = agg(bucket(rank, a.size, a.V, k, a.dtype).to(dev))
        f32 = ShardedAggregator(a.size, k=k, device=dev, wire=a.wire, V=a.V, collective=a.collective, chunks=a.chunks)
    torch.cuda.synchronize()
    assert full.dtype == DTYPES[a.out_dtype]
    raw = {2: torch.int16, 4: torch.int32}[full.element_size()]
    res = {"world": np.array([world]), "lib": np.array([os.path.realpath(_lib.LIB_PATH)]),
           "gather_bytes": np.array([agg.gather_bytes]), "full_bits": full.contiguous().view(raw).cpu().numpy()}
    if not a.workers:
        res["gather_bytes_fp32_out"] = np.array([f32.gather_bytes])      # the same job with out_dtype float32
    if a.wire == "i16":
        res["ovf"] = agg.overflow.cpu().numpy()
    if k == "block":
        res["kblk"] = agg.kblk.cpu().numpy()
    np.savez(os.path.join(a.out, f"rank{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
