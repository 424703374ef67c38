"""Multi-GPU aggregation of one bucket that outgrows a GPU (BASELINE config 5).

Layout A of SURVEY.md 8e (ShardedAggregator): every rank is one worker holding its full fp32
gradient bucket.  Each rank quantises its bucket on its GPU, RCCL reduce-scatters
the integers with SUM over xGMI, the owner of each shard decodes it, and an
all-gather returns the full aggregate to every rank (the PS broadcast).  The
switch aggregates every slot independently (ngaa.p4:87-168), so contiguous slot
ranges can live on different GPUs.

Two wires:
  "i32"  int32 fixed point (2^k).  Integer addition mod 2^32 is associative and
         commutative, so the shard each rank receives is bit-identical to the
         switch's per-slot sum (processor.p4:14-24) in any ring or tree order.
  "i16"  config 4's int16 saturating quantiser.  Saturation is not associative,
         so int16 values never go through the collective: each rank sends the
         int32 wire q16 + (saturated << 22) (ina_quantize_f32_i16_wire), the SUM
         carries the exact int16 sum and the count of saturating ranks together,
         and the owner saturates once and sets the per-slot overflow flag (the
         ngaa_h overflow bit, headers.p4:30) -- bit-identical to the single-GPU
         ina_quantize_reduce_f32_i16_sat over the same W buckets.  The all-gather
         then moves the saturated int16 sums (2 bytes a value, half of fp32's xGMI
         bytes) and the flags, and every rank dequantises the gathered int16 vector
         (an HBM pass of 6 bytes a value, cheap next to the xGMI bytes it saves).

Layout B (RangeAggregator): the workers' buckets arrive already split by range -- rank
r holds every worker's slice of slot range r -- so each rank reduces its W slices
locally with the fused quantise + reduce kernel (no reduce-scatter), decodes, and one
all-gather returns the full aggregate; the xGMI traffic is that all-gather alone (fp32
on the i32 wire; the int16 sums + flags, decoded after the gather, on the i16 wire).

Shards are contiguous slot ranges padded to `align` values (default 1024 values =
4 KiB, rounded up to a whole number of V-value slots), so no slot straddles two
ranks.  The collective plumbing (ShardPlan, reduce_scatter_sum, all_gather_shards)
is device-agnostic and covered on CPU with gloo; with a gloo group and device
tensors the collectives stage through host memory (a test harness for several
ranks on one GPU, never the RCCL path).  Quantise and decode are the device
kernels (no CPU path).

k="block" (both classes): one scale per block of V values (include/ina_blk.h) in place of the one
global k.  Layout A: every rank takes ops.block_scales of its bucket for `world` summands, the
ranks agree on the element-wise MIN (agree_block_scales: ceil(n / V) bytes), quantise with the
agreed scales (on the i16 wire: ops.quantize_i16_wire_blk), run the same integer collective, and
the owner decodes its shard with its slice of the scales (ops.i16_wire_finish_blk /
ops.dequantize_blk).  Layout B: a rank holds all the summands of its range, so its fused AUTO
reduce computes the scales and the all-gather carries them, one byte per block.  Either way the
result equals one GPU's AUTO ops.quantize_reduce_blk / quantize_reduce_i16_blk over the same
buckets, scales included; `kblk` holds the scales of the last call.

error_feedback=True (ShardedAggregator only; include/ina_shard_ef.h, ina_amd.ef): the rank keeps what
its rounding to the wire dropped in an fp32 residual on its GPU and adds it to the next step's
bucket, in the quantiser's own launch.  The collectives, the decode and every byte on xGMI are those
of the plain step: the residual never leaves the rank.

bf16 / fp16 buckets (both classes; include/ina_shard_x16.h, ina_amd.wire, ina_amd.blk): a call takes a
float32, bfloat16 or float16 bucket (RangeAggregator: slices, one dtype for all of them) and reads
it as it is -- no widened fp32 copy.  Widening is exact, so with the default out_dtype=torch.float32
the aggregate, the flags and `kblk` are bit for bit those of the same aggregator on grad.float().
out_dtype=torch.bfloat16 / torch.float16 makes `full` and the decoded shard that dtype: the result is
that fp32 aggregate rounded once to nearest even.  On the i32 wire the owner decodes its shard
straight into 16 bits and the all-gather moves 2 bytes a value instead of 4 (gather_bytes says so);
on the i16 wire the gather moves the int16 sums as before and the expand after it writes 16 bits;
on one rank or after an all-reduce the whole-bucket decode writes them (wire.finish* with a 16-bit
y).  Error feedback takes fp32 buckets only: a 16-bit bucket with error_feedback=True is refused at
the call.

rounding="stochastic" (ShardedAggregator only; include/ina_sr.h, ina_amd.sr): the rank's quantise to the
wire rounds up with the probability of the fraction it would drop, from Philox4x32-10 under the key
`seed` at (element index, step, rank).  Nothing is kept between steps but a step counter and no byte
more moves, so it is there where error feedback is not: 16-bit buckets, and any out_dtype.  Global k
only, and not together with error feedback.  Layout B has it as a class of its own,
StochasticRangeAggregator (include/ina_reduce_sr.h): the fused quantise + reduce rounds worker w's slice
on stream w, so its integer aggregate is the sharded step's, bit for bit.

Per-block scales and stochastic rounding together (include/ina_blk_sr.h, ina_amd.blk_sr) are two classes of
their own, since the constructors above refuse the pair by name: BlockStochasticAggregator (layout A: the
ranks' scales under sr.scale_for's rule, their MIN, the stochastic block quantise on stream `rank`) and
BlockStochasticRangeAggregator (layout B: the fused AUTO reduce with sub = 0, e0 = lo), whose integers, flags
and scales agree bit for bit on both wires.
"""
from __future__ import annotations

import math

import torch
import torch.distributed as dist

from . import _lib, blk, blk_sr, ef, ops, sr
from . import wire as _wire          # (the aggregators' `wire` argument is the wire's name)


class ShardPlan:
    def __init__(self, n: int, world: int, align: int = 1024):
        if n < 0 or world < 1 or align < 1:
            raise ValueError("bad shard plan")
        self.n, self.world, self.align = n, world, align
        per = -(-n // world) if n else 0
        self.shard = -(-per // align) * align
        self.padded = self.shard * world

    def range_of(self, rank: int):
        lo = min(rank * self.shard, self.n)
        return lo, min(lo + self.shard, self.n)


def _host_staged(group) -> bool:
    return dist.get_backend(group) == "gloo"


def reduce_scatter_sum(x_padded: torch.Tensor, plan: ShardPlan, group=None, out=None,
                       async_op: bool = False):
    """int32 [padded] -> this rank's [shard] of the element-wise sum over ranks.  With
    async_op the RCCL work handle is returned as well ((out, work); work is None when
    the call completed synchronously): the collective runs on RCCL's stream and the
    caller's stream waits for it only at work.wait()."""
    if x_padded.numel() != plan.padded:
        raise ValueError("input must be padded to plan.padded")
    out = torch.empty(plan.shard, dtype=x_padded.dtype, device=x_padded.device) if out is None else out
    work = None
    if plan.world == 1:
        out.copy_(x_padded)
    elif x_padded.is_cuda and _host_staged(group):
        h = torch.empty(plan.shard, dtype=x_padded.dtype)
        dist.reduce_scatter_tensor(h, x_padded.cpu(), op=dist.ReduceOp.SUM, group=group)
        out.copy_(h)
    else:
        work = dist.reduce_scatter_tensor(out, x_padded, op=dist.ReduceOp.SUM, group=group,
                                          async_op=async_op)
    return (out, work) if async_op else out


def reduce_scatter_a2a(x_padded: torch.Tensor, plan: ShardPlan, group=None, out=None, recv=None):
    """int32 [padded] -> this rank's [shard] of the element-wise sum over ranks, as ONE
    all-to-all (rank r's slice j goes straight to rank j: on a fully connected xGMI mesh
    every pair of GPUs has its own link, so all 7 links carry (G-1)/G x S at once instead
    of a ring's hops) followed by the device W-way wrapping sum of the G received slices
    (ina_sum_reduce_i32, HBM-bound) -- the same bits as the RCCL SUM (mod-2^32 adds in any
    order).  recv: a [padded] int32 scratch (allocated when None)."""
    if x_padded.numel() != plan.padded:
        raise ValueError("input must be padded to plan.padded")
    out = torch.empty(plan.shard, dtype=torch.int32, device=x_padded.device) if out is None else out
    if plan.world == 1:
        out.copy_(x_padded)
        return out
    recv = torch.empty(plan.padded, dtype=torch.int32, device=x_padded.device) if recv is None else recv
    if x_padded.is_cuda and _host_staged(group):
        h = torch.empty(plan.padded, dtype=torch.int32)
        dist.all_to_all_single(h, x_padded.cpu(), group=group)
        recv.copy_(h)
    else:
        dist.all_to_all_single(recv, x_padded, group=group)
    parts = [recv[r * plan.shard:(r + 1) * plan.shard] for r in range(plan.world)]
    if out.is_cuda:
        ops.sum_reduce(parts, out=out)
    else:                                       # CPU tensors (the gloo tests): the same sum
        acc = parts[0].to(torch.int64)
        for q in parts[1:]:
            acc += q
        out.copy_(((acc + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32))
    return out


def all_reduce_sum(x: torch.Tensor, group=None):
    """int32 in place -> the element-wise sum over ranks (RCCL all-reduce; host-staged
    with gloo and device tensors)."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return x
    if x.is_cuda and _host_staged(group):
        h = x.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        x.copy_(h)
        return x
    dist.all_reduce(x, op=dist.ReduceOp.SUM, group=group)
    return x


def agree_block_scales(kb: torch.Tensor, group=None) -> torch.Tensor:
    """int8 [nblk] in place -> the element-wise MIN over ranks (nothing to do on one rank; host-staged
    with gloo and a device tensor, like the other collectives here).

    ina_scale_for is non-increasing in amax, so the MIN over ranks of each rank's
    ops.block_scales(its buckets, V, bits, degree=world) is the scale of the block's max over ALL
    ranks' buckets: block_scales of all the buckets taken together.  Quantising with the agreed
    scales and summing therefore equals one GPU's AUTO quantize_reduce_blk / quantize_reduce_i16_blk
    over the same buckets with degree = world, scales included."""
    if kb.dtype != torch.int8:
        raise TypeError(f"block scales are torch.int8, got {kb.dtype}")
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return kb
    if kb.is_cuda and _host_staged(group):
        h = kb.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.MIN, group=group)
        kb.copy_(h)
        return kb
    dist.all_reduce(kb, op=dist.ReduceOp.MIN, group=group)
    return kb


def _block_k(k) -> bool:
    """True for k="block"; an integer k is the global scale; any other string is refused."""
    if isinstance(k, str):
        if k != "block":
            raise ValueError(f"k must be an integer or 'block', got {k!r}")
        return True
    return False


_OUT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _out_dtype(out_dtype) -> torch.dtype:
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"out_dtype must be torch.float32, torch.bfloat16 or torch.float16, got {out_dtype!r}")
    return out_dtype


def all_gather_shards(shard: torch.Tensor, plan: ShardPlan, group=None, out=None,
                      async_op: bool = False):
    """[count] per rank -> [world * count] (count = plan.shard values, or its slot flags).
    async_op: returns (out, work) as reduce_scatter_sum does."""
    out = torch.empty(plan.world * shard.numel(), dtype=shard.dtype, device=shard.device) \
        if out is None else out
    work = None
    if plan.world == 1:
        out.copy_(shard)
    elif _host_staged(group):
        # gloo gathers bytes: an all-gather only moves data, so any dtype (gloo has no
        # int16) goes through as its uint8 view, bit for bit
        h = torch.empty(out.numel() * out.element_size(), dtype=torch.uint8)
        dist.all_gather_into_tensor(h, shard.contiguous().cpu().view(torch.uint8), group=group)
        out.copy_(h.view(out.dtype).view(out.shape))
    elif shard.dtype == torch.int16:
        # RCCL has no int16 type; a gather only moves bytes, so int16 goes as its uint8 view
        work = dist.all_gather_into_tensor(out.view(torch.uint8), shard.contiguous().view(torch.uint8),
                                           group=group, async_op=async_op)
    else:
        work = dist.all_gather_into_tensor(out, shard, group=group, async_op=async_op)
    return (out, work) if async_op else out


def _wait(work):
    if work is not None:
        work.wait()          # the caller's stream waits for RCCL's; the host does not block


class ShardedAggregator:
    """Reusable buffers for repeated sharded aggregation of same-sized buckets.

    wire="i32": __call__ returns the dequantised fp32 sum over ranks.
    wire="i16": the same from the int16 saturating path; `overflow` then holds the
    per-slot flags (ceil(n / V) bytes) of the last call.
    collective="rs_ag" (default): reduce-scatter the integer wire, the owner decodes its
    shard, all-gather.  collective="a2a": the reduce-scatter as one all-to-all of the wire
    slices plus the device sum of the G received slices (reduce_scatter_a2a), then the
    same decode and all-gather.  collective="allreduce": one RCCL all-reduce of the
    integer wire (the same (G-1)/G bytes each way per rank inside one collective) and
    every rank decodes the whole bucket.  All give the same bits; which one xGMI runs
    faster is measured by bench.py at N > 1 (sharded_c5 / .a2a / .allreduce).
    chunks=C > 1 (rs_ag, world > 1): the bucket is cut into C contiguous chunks, each
    reduce-scattered and all-gathered on its own (async RCCL work), so chunk c+1's
    quantise runs under chunk c's reduce-scatter and the decodes under the later
    collectives; same bits (integer sums are order-free, the decode is elementwise).
    k="block": per-block scales (V values a block; the module docstring gives the sequence);
    `kblk` then holds the agreed scales of the last call and `scale_bytes` the bytes of their
    exchange.  Not with chunks > 1.
    error_feedback=True: the rank owns `residual` (fp32 [n], zeros at first, reset_residual() zeroes
    it again) and every quantise is the error-feedback one of ina_amd.ef -- v = grad + residual goes
    to the wire and residual becomes v - dequantised(own wire value) (+0 where v is NaN or inf).
    With k="block" the rank's scales are those of v (ef.block_scales) before the ranks take their
    MIN; with chunks > 1 each chunk's quantise takes the matching slice of the residual.  Everything
    after the quantise -- collectives, decode, gather, gather_bytes, scale_bytes -- is unchanged,
    and with the default False so is every byte of the step.  Device buckets only.
    A bucket may be float32, bfloat16 or float16 (not with error_feedback=True) and is read as it is;
    out_dtype (float32, bfloat16 or float16) is the dtype of `full`, of the decoded shard and, on the
    i32 wire, of the all-gather -- the module docstring states what equals what.
    rounding="stochastic" (default "nearest", which leaves every byte of the step as it is): every
    quantise is ina_amd.sr's with the key `seed`, sub = this rank and step = `step`, a counter that
    starts at 0, advances by one per call (aggregate_int and phase_quantize included) and may be set,
    so that a resumed job rounds as the uninterrupted one would; with chunks > 1 each chunk passes its
    offset in the bucket as e0, so the bytes do not depend on chunks.  Any bucket dtype, any out_dtype,
    both wires, every collective; everything after the quantise is unchanged.  Global k only, and not
    with error_feedback=True.  Choose k with sr.scale_for, which leaves a whole quantum of headroom.
    """

    def __init__(self, n: int, k: int = 16, group=None, device=None, align: int = 1024,
                 wire: str = "i32", V: int = 256, collective: str = "rs_ag", chunks: int = 1,
                 error_feedback: bool = False, out_dtype: torch.dtype = torch.float32,
                 rounding: str = "nearest", seed: int = 0):
        self.out_dtype = _out_dtype(out_dtype)
        if rounding not in ("nearest", "stochastic"):
            raise ValueError(f"rounding must be 'nearest' or 'stochastic', got {rounding!r}")
        self.stochastic = rounding == "stochastic"
        if self.stochastic and isinstance(k, str):
            raise ValueError(f"rounding='stochastic' takes a global integer k, got k={k!r}: per-block scales "
                             f"(k='block') go with rounding='nearest'")
        if self.stochastic and error_feedback:
            raise ValueError("rounding='stochastic' and error_feedback=True exclude each other: stochastic rounding "
                             "is the stateless alternative to the residual")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
        self.rounding, self.seed, self._step = rounding, seed, 0
        if wire not in ("i32", "i16"):
            raise ValueError("wire must be 'i32' or 'i16'")
        if collective not in ("rs_ag", "a2a", "allreduce"):
            raise ValueError("collective must be 'rs_ag', 'a2a' or 'allreduce'")
        if chunks < 1 or (chunks > 1 and collective != "rs_ag"):
            raise ValueError("chunks must be >= 1, and > 1 only with collective='rs_ag'")
        self.blk = _block_k(k)
        if self.blk and chunks > 1:
            raise ValueError("k='block' takes chunks=1: the pipelined step would need the whole bucket's "
                             "MIN of the block scales before it quantises its first chunk")
        self.collective = collective
        if V <= 0:
            raise ValueError("V must be > 0")
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        if wire == "i16" and self.world > _lib.I16_WIRE_MAX_RANKS:
            raise ValueError(f"the int16 wire sums at most {_lib.I16_WIRE_MAX_RANKS} ranks")
        if wire == "i16" or self.blk:
            align = align * V // math.gcd(align, V)        # shards hold whole slots / blocks
        self.plan = ShardPlan(n, self.world, align)
        self.k, self.group, self.wire, self.V = k, group, wire, V
        dev = device or torch.device("cuda", torch.cuda.current_device())
        self.error_feedback = bool(error_feedback)
        if self.error_feedback and torch.device(dev).type != "cuda":
            raise ValueError(f"error_feedback=True keeps its residual on the GPU and quantises there; the INA path "
                             f"has no CPU fallback (device {torch.device(dev)})")
        self.chunks = chunks if self.world > 1 else 1
        tot = self.plan.padded
        if self.chunks > 1:
            # chunk c = values [c*L, (c+1)*L), L = world * Sc; rank r owns [c*L + r*Sc, +Sc)
            sc = -(-n // (self.world * self.chunks)) if n else 0
            self.sc = max(-(-sc // align) * align, align)
            self.cplan = ShardPlan(self.world * self.sc, self.world, align=self.sc)
            self.cpad = self.chunks * self.cplan.padded
            tot = max(tot, self.cpad)
            if self.stochastic and self.cplan.padded % 4:
                raise ValueError(f"rounding='stochastic' with chunks > 1 needs chunks of a multiple of 4 values (a "
                                 f"chunk's offset is its e0), got {self.cplan.padded}: use an align that is one")
        # one allocation backs both the whole-bucket and the chunked views; pad stays 0
        self._qbuf = torch.zeros(tot, dtype=torch.int32, device=dev)
        self._fbuf = torch.empty(tot, dtype=self.out_dtype, device=dev)
        self.q, self.full = self._qbuf[: self.plan.padded], self._fbuf[: self.plan.padded]
        # whole-bucket shard buffers (sum_shard, f_shard, s16_shard): used by the unchunked
        # step, aggregate_int and the phase_* methods; the pipelined step (chunks > 1) has
        # its own per-chunk buffers, so there they are allocated on first use only
        self._dev = dev
        self._shard_bufs = {}
        if self.chunks == 1:                     # allocate now, outside any timed step
            self._shard_buf("sum", torch.int32)
            self._shard_buf("f", self.out_dtype)
        if wire == "i16":
            self.slots_per_shard = self.plan.shard // V
            self.ovf_shard = torch.empty(self.slots_per_shard, dtype=torch.uint8, device=dev)
            self._obuf = torch.zeros(tot // V, dtype=torch.uint8, device=dev)
            self.ovf_full = self._obuf[: self.slots_per_shard * self.world]
            if self.world > 1 and collective != "allreduce":   # gather int16 sums, decode after
                if self.chunks == 1:
                    self._shard_buf("s16", torch.int16)
                self._s16buf = torch.empty(tot, dtype=torch.int16, device=dev)
                self.s16_full = self._s16buf[: self.plan.padded]
        if self.blk:
            # one scale per block of the PADDED bucket, the pad blocks at 127: every rank's slice is
            # whole even where its shard lies past n
            self._kbuf = torch.full((self.plan.padded // V,), 127, dtype=torch.int8, device=dev)
        # the all-to-all's receive buffer (world slices of one shard each)
        self._recv = (torch.empty(self.plan.padded, dtype=torch.int32, device=dev)
                      if collective == "a2a" and self.world > 1 else None)
        # error feedback: what this rank's rounding dropped, added to its next bucket
        self.residual = torch.zeros(n, dtype=torch.float32, device=dev) if self.error_feedback else None
        if self.chunks > 1:
            m = self.chunks * self.sc
            self.sum_c = torch.empty(m, dtype=torch.int32, device=dev)
            if wire == "i32":
                self.f_c = torch.empty(m, dtype=self.out_dtype, device=dev)
            else:
                self.s16_c = torch.empty(m, dtype=torch.int16, device=dev)
                self.ovf_c = torch.empty(m // V, dtype=torch.uint8, device=dev)

    def _shard_buf(self, name, dtype):
        b = self._shard_bufs.get(name)
        if b is None:
            b = self._shard_bufs[name] = torch.empty(self.plan.shard, dtype=dtype, device=self._dev)
        return b

    def reset_residual(self):
        """error_feedback=True: forget what earlier steps dropped (the residual back to zeros)."""
        if self.residual is None:
            raise AttributeError("a residual exists only with error_feedback=True")
        self.residual.zero_()

    @property
    def step(self) -> int:
        """rounding="stochastic": the step the next call rounds with (counter word 2 of include/ina_sr.h);
        it advances by one per call, modulo 2^32."""
        return self._step

    @step.setter
    def step(self, value: int):
        if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value < 1 << 32:
            raise ValueError(f"step must be an int in [0, 2^32), got {value!r}")
        self._step = value

    def _advance(self):
        if self.stochastic:
            self._step = (self._step + 1) & 0xFFFFFFFF

    @property
    def sum_shard(self) -> torch.Tensor:
        """This rank's int32 shard of the summed wire (whole-bucket step)."""
        return self._shard_buf("sum", torch.int32)

    @property
    def f_shard(self) -> torch.Tensor:
        return self._shard_buf("f", self.out_dtype)

    @property
    def s16_shard(self) -> torch.Tensor:
        return self._shard_buf("s16", torch.int16)

    @property
    def overflow(self) -> torch.Tensor:
        """Per-slot overflow flags of the last i16 aggregation (ceil(n / V) bytes)."""
        if self.wire != "i16":
            raise AttributeError("overflow flags exist only on the i16 wire")
        return self._obuf[: -(-self.plan.n // self.V)]

    @property
    def kblk(self) -> torch.Tensor:
        """k="block": the agreed scales of the last call (ceil(n / V) int8)."""
        if not self.blk:
            raise AttributeError("block scales exist only with k='block'")
        return self._kbuf[: -(-self.plan.n // self.V)]

    def _kshard(self) -> torch.Tensor:
        """The scales of this rank's shard."""
        b = self.plan.shard // self.V
        return self._kbuf[self.rank * b:(self.rank + 1) * b]

    @property
    def scale_bytes(self) -> int:
        """Bytes of the block-scale exchange (agree_block_scales) per step: one per block."""
        return -(-self.plan.n // self.V) if self.blk and self.world > 1 else 0

    @property
    def gather_bytes(self) -> int:
        """Bytes one all-gather step brings to each rank over xGMI (values + flags);
        with collective="allreduce" the all-reduce's gather half (int32 wire words)."""
        if self.world == 1:
            return 0
        shard = self.chunks * self.sc if self.chunks > 1 else self.plan.shard
        if self.collective == "allreduce":
            return (self.world - 1) * shard * 4
        per = shard * (2 if self.wire == "i16" else self._fbuf.element_size())
        if self.wire == "i16":
            per += shard // self.V
        return (self.world - 1) * per

    # The step's phases, in order (bench.py times each one between HIP events).
    def phase_quantize(self, grad: torch.Tensor):
        self._quantize(grad)

    def phase_reduce_scatter(self):
        """The integer collective: reduce-scatter, or the whole all-reduce."""
        if self.world == 1:
            return
        if self.collective == "allreduce":
            all_reduce_sum(self.q, self.group)
        elif self.collective == "a2a":
            reduce_scatter_a2a(self.q, self.plan, self.group, out=self.sum_shard, recv=self._recv)
        else:
            reduce_scatter_sum(self.q, self.plan, self.group, out=self.sum_shard)

    def phase_decode(self):
        """The owner's decode of its shard (one rank, or after an all-reduce: the whole
        bucket on every rank)."""
        if self.world == 1 or self.collective == "allreduce":
            self._decode(self.q, self.full, self.ovf_full if self.wire == "i16" else None)
        elif self.blk and self.wire == "i32":
            blk.dequantize(self.sum_shard, self._kshard(), self.V, out=self.f_shard)
        elif self.blk:
            ops.i16_wire_finish_blk(self.sum_shard, self._kshard(), self.V, out16=self.s16_shard,
                                    overflow=self.ovf_shard, want_y=False)
        elif self.wire == "i32":
            ops.dequantize(self.sum_shard, self.k, out=self.f_shard)
        else:
            ops.i16_wire_finish(self.sum_shard, self.k, self.V, out16=self.s16_shard,
                                overflow=self.ovf_shard, want_y=False)

    def phase_all_gather(self):
        if self.world == 1 or self.collective == "allreduce":
            return
        if self.wire == "i32":
            all_gather_shards(self.f_shard, self.plan, self.group, out=self.full)
        else:
            all_gather_shards(self.s16_shard, self.plan, self.group, out=self.s16_full)
            all_gather_shards(self.ovf_shard, self.plan, self.group, out=self.ovf_full)

    def phase_expand(self):
        """i16 wire at world > 1: dequantise the gathered int16 sums on every rank."""
        if self.world > 1 and self.wire == "i16" and self.collective != "allreduce":
            if self.blk:
                blk.dequantize(self.s16_full, self._kbuf, self.V, out=self.full)
            else:
                ops.dequantize(self.s16_full, self.k, out=self.full)

    def _bucket(self, grad: torch.Tensor) -> torch.Tensor:
        """The call's bucket, flat: float32, bfloat16 or float16 (the quantisers dispatch on it)."""
        if grad.numel() != self.plan.n:
            raise ValueError("bucket size changed")
        if self.error_feedback and isinstance(grad, torch.Tensor) and grad.dtype in (torch.bfloat16, torch.float16):
            raise TypeError(f"error_feedback=True takes float32 buckets, got {grad.dtype}: the error-feedback wire "
                            f"quantisers and block scales have no 16-bit source")
        return grad.reshape(-1)

    def _quantize(self, grad: torch.Tensor):
        n = self.plan.n
        x = self._bucket(grad)
        r = self.residual
        if self.blk:
            # this rank's scales for `world` summands (error feedback: of x + residual), the MIN over
            # ranks, then the wire
            kb = self.kblk
            bits = 32 if self.wire == "i32" else 16
            if r is None:
                blk.block_scales([x], self.V, bits=bits, degree=self.world, out=kb)
            else:
                ef.block_scales([x], [r], self.V, bits=bits, degree=self.world, out=kb)
            agree_block_scales(kb, self.group)
            if self.wire == "i32":
                if r is None:
                    blk.quantize(x, kb, self.V, out=self.q[:n])
                else:
                    ef.quantize_blk(x, r, self.V, kblk=kb, out=self.q[:n])
            elif r is None:
                _wire.quantize_blk(x, kb, self.V, out=self.q[:n])
            else:
                ef.quantize_i16_wire_blk(x, r, kb, self.V, out=self.q[:n])
        else:
            self._quantize_global(x, r, self.q[:n])
        self._advance()

    def _quantize_global(self, x: torch.Tensor, r, out: torch.Tensor, e0: int = 0):
        """x (the bucket or a chunk of it) to the wire at the global k; r: the same values of the
        residual, or None without error feedback; e0: x's offset in the bucket (stochastic rounding)."""
        if self.stochastic:
            if self.wire == "i32":
                sr.quantize(x, self.k, self.seed, step=self._step, sub=self.rank, e0=e0, out=out)
            else:
                sr.quantize_i16_wire(x, self.k, self.seed, step=self._step, sub=self.rank, e0=e0, out=out)
        elif self.wire == "i32":
            if r is None:
                ops.quantize(x, self.k, out=out)
            else:
                ef.quantize(x, r, self.k, out=out)
        elif r is None:
            _wire.quantize(x, self.k, out=out)
        else:
            ef.quantize_i16_wire(x, r, self.k, out=out)

    def _decode(self, src: torch.Tensor, y: torch.Tensor, ovf=None):
        """The whole (padded) bucket: one rank, or after an all-reduce."""
        if self.blk and self.wire == "i32":
            blk.dequantize(src, self._kbuf, self.V, out=y)
        elif self.blk:
            _wire.finish_blk(src, self._kbuf, self.V, y=y, overflow=ovf, want_out16=False)
        elif self.wire == "i32":
            ops.dequantize(src, self.k, out=y)
        else:
            _wire.finish(src, self.k, self.V, y=y, overflow=ovf, want_out16=False)

    def _call_chunked(self, grad: torch.Tensor) -> torch.Tensor:
        n, L, sc, V = self.plan.n, self.cplan.padded, self.sc, self.V
        x = self._bucket(grad)
        rs = []
        for c in range(self.chunks):           # quantise chunk c, then its RS on RCCL's stream
            lo, hi = c * L, min((c + 1) * L, n)
            if hi > lo:         # (lo is a multiple of align: the slices stay on the vector path)
                self._quantize_global(x[lo:hi], None if self.residual is None else self.residual[lo:hi],
                                      self._qbuf[lo:hi], e0=lo)
            rs.append(reduce_scatter_sum(self._qbuf[c * L:(c + 1) * L], self.cplan, self.group,
                                         out=self.sum_c[c * sc:(c + 1) * sc], async_op=True)[1])
        self._advance()
        ag = []
        for c in range(self.chunks):           # decode shard c once its RS is done, gather it
            _wait(rs[c])
            part = self.sum_c[c * sc:(c + 1) * sc]
            if self.wire == "i32":
                ops.dequantize(part, self.k, out=self.f_c[c * sc:(c + 1) * sc])
                ag.append(all_gather_shards(self.f_c[c * sc:(c + 1) * sc], self.cplan, self.group,
                                            out=self._fbuf[c * L:(c + 1) * L], async_op=True)[1])
            else:
                o16 = self.s16_c[c * sc:(c + 1) * sc]
                of = self.ovf_c[c * sc // V:(c + 1) * sc // V]
                ops.i16_wire_finish(part, self.k, V, out16=o16, overflow=of, want_y=False)
                ag.append(all_gather_shards(o16, self.cplan, self.group,
                                            out=self._s16buf[c * L:(c + 1) * L], async_op=True)[1])
                ag.append(all_gather_shards(of, self.cplan, self.group,
                                            out=self._obuf[c * L // V:(c + 1) * L // V], async_op=True)[1])
        for w in ag:
            _wait(w)
        if self.wire == "i16":
            ops.dequantize(self._s16buf[: self.cpad], self.k, out=self._fbuf[: self.cpad])
        return self._fbuf[:n]

    def __call__(self, grad: torch.Tensor) -> torch.Tensor:
        """[n] local bucket (float32, bfloat16 or float16) -> [n] dequantised sum over all ranks as
        out_dtype (one rank: the collectives are identities, quantise -> decode)."""
        if self.chunks > 1:
            return self._call_chunked(grad)
        self.phase_quantize(grad)
        self.phase_reduce_scatter()
        self.phase_decode()
        self.phase_all_gather()
        self.phase_expand()
        return self.full[: self.plan.n]

    def aggregate_int(self, grad: torch.Tensor) -> torch.Tensor:
        """[n] bucket -> this rank's integer shard of the aggregate (no gather): the
        int32 wrapped sum, or on the i16 wire the int16 saturated sum (its slot flags
        in `ovf_shard`).  k="block": the integers are scaled per block; read `kblk` next to them.
        error_feedback=True: this is a step like any other -- it quantises grad + residual and
        advances the residual."""
        self._quantize(grad)
        if self.collective == "a2a":
            s = reduce_scatter_a2a(self.q, self.plan, self.group, out=self.sum_shard, recv=self._recv)
        else:
            s = reduce_scatter_sum(self.q, self.plan, self.group, out=self.sum_shard)
        if self.wire == "i32":
            return s
        if self.blk:
            out16, _, _ = ops.i16_wire_finish_blk(s, self._kshard(), self.V, overflow=self.ovf_shard, want_y=False)
        else:
            out16, _, _ = ops.i16_wire_finish(s, self.k, self.V, overflow=self.ovf_shard, want_y=False)
        return out16


class RangeAggregator:
    """Layout B of SURVEY.md 8e: rank r holds the W workers' fp32 slices of its own range
    `plan.range_of(r)` (the workers sent slot range r to GPU r: per-slot independence,
    ngaa.p4:87-168).  __call__ reduces them on this GPU -- the fused quantise + wrapping
    int32 sum (processor.p4:14-24), or on wire="i16" the int16 saturating sum with its
    per-slot overflow flags (headers.p4:30) -- dequantises, and all-gathers the fp32
    aggregate (and the flags) to every rank.  Each rank's shard is bit-identical to the
    single-GPU ina_quantize_reduce_f32_i32 / _i16_sat over the same W buckets, since the
    ranges hold whole slots.  k="block": the fused reduces in AUTO mode (ops.quantize_reduce_blk /
    quantize_reduce_i16_blk, degree = W) with one scale per block of V values; the all-gather also
    carries the shard's scales and `kblk` holds the bucket's after a call.
    No error feedback here, and no such argument: a rank holds OTHER workers' slices, and the
    residual of a slice lives with the worker that rounded it, not with the GPU that sums it (the
    reason include/ina_ef.h gives for leaving out the fused quantise + reduce calls).  A worker that
    wants it applies ina_amd.ef before it sends its slices.
    The slices may be float32, bfloat16 or float16, one dtype for all of them, and are read as they
    are; out_dtype (float32, bfloat16 or float16) is the dtype of `full` and of the decoded range, and
    on the i32 wire the all-gather then moves 2 bytes a value.
    """

    def __init__(self, n: int, k: int = 16, group=None, device=None, align: int = 1024,
                 wire: str = "i32", V: int = 256, out_dtype: torch.dtype = torch.float32):
        self.out_dtype = _out_dtype(out_dtype)
        if wire not in ("i32", "i16"):
            raise ValueError("wire must be 'i32' or 'i16'")
        if V <= 0:
            raise ValueError("V must be > 0")
        self.blk = _block_k(k)
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        if wire == "i16" or self.blk:
            align = align * V // math.gcd(align, V)        # ranges hold whole slots / blocks
        self.plan = ShardPlan(n, self.world, align)
        self.k, self.group, self.wire, self.V = k, group, wire, V
        dev = device or torch.device("cuda", torch.cuda.current_device())
        self.lo, self.hi = self.plan.range_of(self.rank)
        sdt = torch.int32 if wire == "i32" else torch.int16
        self.sum_shard = torch.zeros(self.plan.shard, dtype=sdt, device=dev)
        self.f_shard = torch.zeros(self.plan.shard, dtype=self.out_dtype, device=dev)   # pad stays 0
        # one rank: the gather is an identity, so the decode writes the aggregate in place
        self.full = self.f_shard if self.world == 1 else torch.empty(self.plan.padded, dtype=self.out_dtype,
                                                                     device=dev)
        if wire == "i16":
            self.slots_per_shard = self.plan.shard // V
            self.ovf_shard = torch.zeros(self.slots_per_shard, dtype=torch.uint8, device=dev)
            self.ovf_full = self.ovf_shard if self.world == 1 else torch.empty(
                self.slots_per_shard * self.world, dtype=torch.uint8, device=dev)
            if self.world > 1:        # the gather moves the int16 sums, decoded afterwards
                self.s16_full = torch.empty(self.plan.padded, dtype=torch.int16, device=dev)
        if self.blk:                  # one scale per block of the padded range, the pad blocks at 127
            self.k_shard = torch.full((self.plan.shard // V,), 127, dtype=torch.int8, device=dev)
            self.k_full = self.k_shard if self.world == 1 else torch.empty(self.plan.padded // V,
                                                                          dtype=torch.int8, device=dev)

    @property
    def range(self):
        """(lo, hi): the values of the bucket whose worker slices this rank holds."""
        return self.lo, self.hi

    @property
    def overflow(self) -> torch.Tensor:
        """Per-slot overflow flags of the last i16 aggregation (ceil(n / V) bytes)."""
        if self.wire != "i16":
            raise AttributeError("overflow flags exist only on the i16 wire")
        return self.ovf_full[: -(-self.plan.n // self.V)]

    @property
    def kblk(self) -> torch.Tensor:
        """k="block": the scales of the last call's aggregate (ceil(n / V) int8)."""
        if not self.blk:
            raise AttributeError("block scales exist only with k='block'")
        return self.k_full[: -(-self.plan.n // self.V)]

    @property
    def scale_bytes(self) -> int:
        """No exchange before the reduce: a rank holds every summand of its range (the scales ride
        in the all-gather, counted in gather_bytes)."""
        return 0

    def _reduce(self, slices) -> int:
        m = self.hi - self.lo
        if isinstance(slices, torch.Tensor):
            slices = list(slices.unbind(0)) if slices.dim() > 1 else [slices]
        slices = [t.reshape(-1) for t in slices]
        if not slices or any(t.numel() != m for t in slices):
            raise ValueError(f"every worker slice must hold this rank's {m} values")
        if m == 0:                    # more ranks than ranges: nothing here, zeros gathered
            return 0
        nb = -(-m // self.V)
        if self.blk and self.wire == "i32":
            blk.quantize_reduce(slices, self.V, out=self.sum_shard[:m], kblk_out=self.k_shard[:nb])
        elif self.blk:
            blk.quantize_reduce_i16(slices, self.V, out=self.sum_shard[:m], overflow=self.ovf_shard[:nb],
                                    kblk_out=self.k_shard[:nb])
        elif self.wire == "i32":
            ops.quantize_reduce(slices, self.k, out=self.sum_shard[:m])
        else:
            ops.quantize_reduce_i16(slices, self.k, self.V, out=self.sum_shard[:m],
                                    overflow=self.ovf_shard[: -(-m // self.V)])
        return m

    @property
    def gather_bytes(self) -> int:
        """Bytes the all-gather brings to each rank over xGMI (values + flags)."""
        if self.world == 1:
            return 0
        per = self.plan.shard * (2 if self.wire == "i16" else self.f_shard.element_size())
        if self.wire == "i16":
            per += self.slots_per_shard
        if self.blk:
            per += self.plan.shard // self.V
        return (self.world - 1) * per

    # The step's phases, in order (bench.py times each one between HIP events).
    def phase_reduce_decode(self, slices) -> int:
        """Local fused quantise + reduce; on the i32 wire (or one rank) also the decode."""
        m = self._reduce(slices)
        if m and (self.wire == "i32" or self.world == 1):
            if self.blk:
                blk.dequantize(self.sum_shard[:m], self.k_shard, self.V, out=self.f_shard[:m])
            else:
                ops.dequantize(self.sum_shard[:m], self.k, out=self.f_shard[:m])
        return m

    def phase_all_gather(self):
        if self.world == 1:
            return
        if self.wire == "i32":
            all_gather_shards(self.f_shard, self.plan, self.group, out=self.full)
        else:
            all_gather_shards(self.sum_shard, self.plan, self.group, out=self.s16_full)
            all_gather_shards(self.ovf_shard, self.plan, self.group, out=self.ovf_full)
        if self.blk:
            all_gather_shards(self.k_shard, self.plan, self.group, out=self.k_full)

    def phase_expand(self):
        """i16 wire at world > 1: dequantise the gathered int16 sums on every rank."""
        if self.world > 1 and self.wire == "i16":
            if self.blk:
                blk.dequantize(self.s16_full, self.k_full, self.V, out=self.full)
            else:
                ops.dequantize(self.s16_full, self.k, out=self.full)

    def __call__(self, slices) -> torch.Tensor:
        """W slices of this rank's range (float32, bfloat16 or float16) -> [n] aggregate on every rank,
        as out_dtype."""
        self.phase_reduce_decode(slices)
        self.phase_all_gather()
        self.phase_expand()
        return self.full[: self.plan.n]

    def aggregate_int(self, slices) -> torch.Tensor:
        """W slices -> this rank's integer aggregate (int32 wrapped, or int16
        saturated with its slot flags in `ovf_shard`), no gather.  k="block": scaled per block, the
        scales in `k_shard`."""
        m = self._reduce(slices)
        return self.sum_shard[:m]


class StochasticRangeAggregator(RangeAggregator):
    """RangeAggregator with every summand rounded stochastically (include/ina_reduce_sr.h, ina_amd.sr): layout
    B's answer to ShardedAggregator(rounding="stochastic").  The reduce is sr.quantize_reduce /
    sr.quantize_reduce_i16 with the key `seed`, sub = 0 -- worker w of the slices draws from stream w --
    e0 = this rank's `lo` and step = `step`, a counter that starts at 0, advances by one per __call__ /
    aggregate_int / phase_reduce_decode (modulo 2^32) and may be set, so that a resumed job rounds as the
    uninterrupted one would.  With worker w's slices coming from the rank-w bucket of a sharded step, this
    rank's integer aggregate is bit for bit that range of ShardedAggregator(rounding="stochastic", seed)'s
    at the same step, on both wires: the two layouts of config 5 agree.  Everything after the reduce --
    decode, gather, gather_bytes -- is RangeAggregator's.  Global k only (choose it with sr.scale_for), and
    `lo` must be a multiple of 4: a plan whose align is one gives that.  A class of its own, since
    RangeAggregator's arguments are fixed."""

    def __init__(self, n: int, k: int = 16, group=None, device=None, align: int = 1024,
                 wire: str = "i32", V: int = 256, out_dtype: torch.dtype = torch.float32, seed: int = 0):
        if isinstance(k, str) or k is None or isinstance(k, torch.Tensor):
            raise ValueError(f"StochasticRangeAggregator takes a global integer k, got k={k!r}: per-block scales "
                             f"(k='block') go with RangeAggregator, which rounds to nearest")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
        super().__init__(n, k=k, group=group, device=device, align=align, wire=wire, V=V, out_dtype=out_dtype)
        if self.hi > self.lo and self.lo % 4:
            raise ValueError(f"this rank's range starts at {self.lo}, not a multiple of 4 (it is the e0 of the "
                             f"rounding): use an align that is a multiple of 4")
        self.rounding, self.seed, self._step = "stochastic", seed, 0

    @property
    def step(self) -> int:
        """The step the next call rounds with (counter word 2 of include/ina_sr.h); it advances by one per
        call, modulo 2^32."""
        return self._step

    @step.setter
    def step(self, value: int):
        if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value < 1 << 32:
            raise ValueError(f"step must be an int in [0, 2^32), got {value!r}")
        self._step = value

    def _reduce(self, slices) -> int:
        # (the slice normalisation and the length check are RangeAggregator._reduce's, repeated here
        # because that class stays as it is; a change to either belongs in both)
        m = self.hi - self.lo
        if isinstance(slices, torch.Tensor):
            slices = list(slices.unbind(0)) if slices.dim() > 1 else [slices]
        slices = [t.reshape(-1) for t in slices]
        if not slices or any(t.numel() != m for t in slices):
            raise ValueError(f"every worker slice must hold this rank's {m} values")
        if m:                         # more ranks than ranges: nothing here, zeros gathered
            if self.wire == "i32":
                sr.quantize_reduce(slices, self.k, self.seed, step=self._step, e0=self.lo, out=self.sum_shard[:m])
            else:
                sr.quantize_reduce_i16(slices, self.k, self.V, self.seed, step=self._step, e0=self.lo,
                                       out=self.sum_shard[:m], overflow=self.ovf_shard[: -(-m // self.V)])
        self._step = (self._step + 1) & 0xFFFFFFFF
        return m


def _check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an int in [0, 2^64), got {seed!r}")
    return seed


class BlockStochasticAggregator(ShardedAggregator):
    """ShardedAggregator(k="block") with the rank's quantise rounded stochastically (include/ina_blk_sr.h,
    ina_amd.blk_sr): per-block scales and unbiased rounding together, the pair an int16 job of many ranks
    wants.  Every rank takes blk_sr.block_scales of its bucket for `world` summands (sr.scale_for's rule: a
    whole quantum of headroom per summand), the ranks agree on the element-wise MIN (agree_block_scales --
    sr.scale_for is monotone in amax, so the MIN is the scale of the ranks' joint max), and the rank
    quantises with blk_sr.quantize (wire="i32") or blk_sr.quantize_i16_wire (wire="i16") under the key
    `seed` with sub = this rank, e0 = 0 and step = `step`, the counter of
    ShardedAggregator(rounding="stochastic"): it starts at 0, advances by one per call (aggregate_int and
    phase_quantize included) and may be set, so that a resumed job rounds as the uninterrupted one would.
    Everything after the quantise -- the collectives, the decode, gather_bytes, scale_bytes -- is the
    k="block" step's, unchanged.  Every collective, both wires, any bucket dtype, any out_dtype.  No
    chunks and no error feedback, and no such arguments; a class of its own, since ShardedAggregator
    refuses rounding="stochastic" with k="block" by name."""

    def __init__(self, n: int, group=None, device=None, align: int = 1024, wire: str = "i32", V: int = 256,
                 collective: str = "rs_ag", out_dtype: torch.dtype = torch.float32, seed: int = 0):
        _check_seed(seed)
        super().__init__(n, k="block", group=group, device=device, align=align, wire=wire, V=V,
                         collective=collective, out_dtype=out_dtype, seed=seed)
        self.rounding, self.stochastic = "stochastic", True      # the step counter advances

    def _quantize(self, grad: torch.Tensor):
        n = self.plan.n
        x = self._bucket(grad)
        kb = self.kblk
        blk_sr.block_scales([x], self.V, bits=32 if self.wire == "i32" else 16, degree=self.world, out=kb)
        agree_block_scales(kb, self.group)
        fn = blk_sr.quantize if self.wire == "i32" else blk_sr.quantize_i16_wire
        fn(x, kb, self.V, self.seed, step=self._step, sub=self.rank, e0=0, out=self.q[:n])
        self._advance()


class BlockStochasticRangeAggregator(RangeAggregator):
    """RangeAggregator(k="block") with every summand rounded stochastically (include/ina_blk_sr.h,
    ina_amd.blk_sr): layout B's answer to BlockStochasticAggregator.  The reduce is the AUTO
    blk_sr.quantize_reduce / blk_sr.quantize_reduce_i16 with degree = W (the number of slices), the key
    `seed`, sub = 0 -- worker w of the slices draws from stream w -- e0 = this rank's `lo` and
    step = `step`, StochasticRangeAggregator's counter.  With worker w's slices coming from the rank-w
    bucket of a BlockStochasticAggregator step of W ranks, this rank's integer aggregate, flags and
    scales are bit for bit that range of the sharded step's, on both wires.  Everything after the reduce
    is RangeAggregator's.  `lo` must be a multiple of 4: a plan whose align is one gives that."""

    def __init__(self, n: int, group=None, device=None, align: int = 1024, wire: str = "i32", V: int = 256,
                 out_dtype: torch.dtype = torch.float32, seed: int = 0):
        _check_seed(seed)
        super().__init__(n, k="block", group=group, device=device, align=align, wire=wire, V=V, out_dtype=out_dtype)
        if self.hi > self.lo and self.lo % 4:
            raise ValueError(f"this rank's range starts at {self.lo}, not a multiple of 4 (it is the e0 of the "
                             f"rounding): use an align that is a multiple of 4")
        self.rounding, self.seed, self._step = "stochastic", seed, 0

    step = StochasticRangeAggregator.step

    def _reduce(self, slices) -> int:
        # (the slice normalisation and the length check are RangeAggregator._reduce's, as in
        # StochasticRangeAggregator)
        m = self.hi - self.lo
        if isinstance(slices, torch.Tensor):
            slices = list(slices.unbind(0)) if slices.dim() > 1 else [slices]
        slices = [t.reshape(-1) for t in slices]
        if not slices or any(t.numel() != m for t in slices):
            raise ValueError(f"every worker slice must hold this rank's {m} values")
        if m:                         # more ranks than ranges: nothing here, zeros gathered
            nb = -(-m // self.V)
            kw = dict(degree=len(slices), step=self._step, sub=0, e0=self.lo, out=self.sum_shard[:m],
                      kblk_out=self.k_shard[:nb])
            if self.wire == "i32":
                blk_sr.quantize_reduce(slices, self.V, self.seed, **kw)
            else:
                blk_sr.quantize_reduce_i16(slices, self.V, self.seed, overflow=self.ovf_shard[:nb], **kw)
        self._step = (self._step + 1) & 0xFFFFFFFF
        return m
