"""One rank of tests/test_gpu_i4.py's multi-rank test, launched by torch.distributed.run like tests/_i8_rank.py: every
rank on cuda:0 over gloo, two steps of dist.NibbleWireAggregator; what the rank then holds goes to OUT/rank<r>.npz."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "distributed-training-ina_amd")]

if __name__ == "__main__":
    from tests._i8_rank import bucket
    n, V, seed, out, gather = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    from ina_amd.dist import NibbleWireAggregator
    agg = NibbleWireAggregator(n, V=V, device=torch.device("cuda", 0), seed=seed, gather=gather)
    x = torch.from_numpy(bucket(dist.get_rank(), n)).to("cuda:0")
    for _ in range(2):                          # buffers are reused; the second step rotates under step = 1
        full = agg(x)
    torch.cuda.synchronize()
    sums, shift = (agg.q8_full, agg.gather_shift) if gather == "i8" else (agg.s16_full, torch.zeros(1))
    np.savez(os.path.join(out, f"rank{dist.get_rank()}.npz"), full=full.cpu().numpy(), kblk=agg.kblk.cpu().numpy(),
             sums=sums.cpu().numpy(), shift=shift.cpu().numpy(), q4=agg.q4.cpu().numpy(), shard=np.array(agg.plan.shard),
             bytes=np.array([agg.wire_bytes, agg.gather_bytes, agg.scale_bytes]))
    dist.barrier()
    dist.destroy_process_group()
