"""One RCCL rank (backend nccl, world size 1), launched by torch.distributed.run from
tests/test_gpu_dist_blk.py: the one collective k="block" adds to the sharded path --
all_reduce(int8, MIN) of the block scales, as dist.agree_block_scales issues it at N > 1 -- through
RCCL on this image, in place on a view of a larger buffer (ShardedAggregator's scale array with its
pad blocks), and the int8 all-gather of RangeAggregator's scales.  At world size 1 both are copies,
so the results are checked exactly; what this run proves is that RCCL takes the dtype and the op."""
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-training-ina_amd"))


def main():
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev)
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    from ina_amd import ops
    from ina_amd.dist import ShardPlan
    n, V = 100_003, 32
    nblk = (n + V - 1) // V
    g = torch.Generator(device=dev).manual_seed(6)
    x = torch.randn(n, device=dev, generator=g) * torch.logspace(-6, 8, n, device=dev)
    buf = torch.full((nblk + 40,), 127, dtype=torch.int8, device=dev)
    kb = buf[:nblk]
    ops.block_scales([x], V, bits=16, degree=1, out=kb)
    want = kb.clone()
    assert want.min().item() < 0 < want.max().item()          # both signs go through the MIN
    dist.all_reduce(kb, op=dist.ReduceOp.MIN)                 # the call agree_block_scales makes at N > 1
    assert torch.equal(kb, want) and bool((buf[nblk:] == 127).all())
    plan = ShardPlan(n, 1, align=V)
    shard = torch.full((plan.shard // V,), 127, dtype=torch.int8, device=dev)
    shard[:nblk] = want
    out = torch.empty(plan.padded // V, dtype=torch.int8, device=dev)
    dist.all_gather_into_tensor(out, shard)                   # RangeAggregator's gather of the scales
    assert torch.equal(out, shard)
    dist.barrier()
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("rccl world-1 block-scale collectives ok")


if __name__ == "__main__":
    main()
