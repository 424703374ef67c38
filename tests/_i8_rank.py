"""One rank of the 8-bit wire's multi-rank test (tests/test_gpu_i8.py), launched by torch.distributed.run: every
rank on cuda:0, the group gloo (the collectives stage through host memory), the kernels libina.so's.  Two
steps of dist.ByteWireAggregator; what the rank then holds goes to OUT/rank<r>.npz."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "distributed-training-ina_amd")]


def bucket(rank: int, n: int) -> np.ndarray:
    """Block magnitudes over four decades, one NaN."""
    rng = np.random.default_rng(7000 + rank)
    x = (rng.standard_normal(n) * np.repeat(10.0 ** rng.uniform(-3, 1, -(-n // 64)), 64)[:n]).astype(np.float32)
    x[7] = np.nan
    return x


if __name__ == "__main__":
    n, V, seed, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    from ina_amd.dist import ByteWireAggregator
    agg = ByteWireAggregator(n, V=V, device=torch.device("cuda", 0), seed=seed)
    x = torch.from_numpy(bucket(dist.get_rank(), n)).to("cuda:0")
    for _ in range(2):                          # buffers are reused; the second step rotates under step = 1
        full = agg(x)
    torch.cuda.synchronize()
    np.savez(os.path.join(out, f"rank{dist.get_rank()}.npz"), full=full.cpu().numpy(), kblk=agg.kblk.cpu().numpy(),
             s16=agg.s16_full.cpu().numpy(), shard=np.array(agg.plan.shard),
             bytes=np.array([agg.wire_bytes, agg.gather_bytes, agg.scale_bytes]))
    dist.barrier()
    dist.destroy_process_group()
