"""One rank of the stochastic byte wire's multi-rank test (tests/test_gpu_i8_sr.py), as tests/_i8_gather_rank.py is
of the requantised gather's: two steps of dist.ByteWireAggregator(gather="i8", rounding="stochastic") on cuda:0 over
gloo, the result to OUT/rank<r>.npz."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

from _i8_rank import bucket                     # beside this script; importing it puts the repository on sys.path

if __name__ == "__main__":
    n, V, seed, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    from ina_amd.dist import ByteWireAggregator
    agg = ByteWireAggregator(n, V=V, device=torch.device("cuda", 0), seed=seed, gather="i8", rounding="stochastic")
    x = torch.from_numpy(bucket(dist.get_rank(), n)).to("cuda:0")
    for _ in range(2):                          # buffers are reused; the second step draws under step = 1
        full = agg(x)
    torch.cuda.synchronize()
    np.savez(os.path.join(out, f"rank{dist.get_rank()}.npz"), full=full.cpu().numpy(), kblk=agg.kblk.cpu().numpy(),
             q8=agg.q8_full.cpu().numpy(), shift=agg.gather_shift.cpu().numpy(),
             bytes=np.array([agg.wire_bytes, agg.gather_bytes, agg.scale_bytes]))
    dist.barrier()
    dist.destroy_process_group()
