"""Unbiased stochastic rounding for the quantisers (include/ina_sr.h): the stateless alternative to
error feedback (ina_amd.ef).

Each function is the ops / wire function of the same name with the rounding replaced:

    t = (x - base) * 2^k;   y = floor(t) + (u < t - floor(t));   q = the sibling's clamp of y

u is 24 bits of Philox4x32-10 under the key `seed` at the counter ((e0 + e) >> 2, step, sub), word
(e0 + e) & 3 -- a pure function of (seed, step, sub, element index), so every result can be replayed
(tests/_sr_ref.py) and depends on neither the grid nor the alignment.  E[q] = t where nothing clips;
where t is an integer q is the round-to-nearest result for every seed.  No bytes beyond the sibling's
move and nothing is kept between calls.

    k = sr.scale_for(amax, world, 16)                        # one more quantum of headroom than ops.scale_for
    w = sr.quantize_i16_wire(grad_bf16, k, seed, step=t, sub=rank)
    w = sr.quantize_i16_wire(grad[lo:hi], k, seed, step=t, sub=rank, e0=lo)   # that slice of the line above

x is float32, bfloat16 or float16; base is float32.  `step` is the training step, `sub` the stream within
it (ranks that share a seed must differ here, or they all round the same way), `e0` the offset of x in
its bucket, a multiple of 4.  No CPU fallback.

On the packet path (include/ina_pkt_sr.h) the worker packs round the same way in their own launch:

    pkts = sr.quantize_pack_nga(grad, k, V, bitmap, count, switch_id, seq0, seed, step=t, sub=worker)
    hdrs, pays = sr.quantize_pack_nga_multi_split(grads, k, V, bitmaps, count, switch_id, seq0, seed, step=t)

the rows of ops.pack_nga / ops.pack_nga_split on sr.quantize's words, worker w of a multi-worker call
drawing from stream sub + w.  With per-packet scales (k an int8 tensor, or None to compute them) the
buckets are float32, and sr.block_scales gives the scales with sr.scale_for's extra quantum.

On the GPU that sums W workers' buckets (include/ina_reduce_sr.h) the fused quantise + reduce rounds every
summand the same way in its one launch, worker w on stream sub + w:

    s = sr.quantize_reduce(grads, k, seed, step=t)                       # ops.sum_reduce of W sr.quantize
    s16, ovf = sr.quantize_reduce_i16(slices, k, V, seed, step=t, e0=lo)  # that range of the bucket's result

Global k only.  dist.StochasticRangeAggregator is layout B of config 5 on these two calls.
"""
from __future__ import annotations

import ctypes as C
import numbers

import torch

from . import _lib, ops
from ._lib import NUM_REGISTER, check, load
from .ops import _X16, _blk_scales_arg, _blk_v, _fits, _ptr, _ptrs, _req, _req_grad, _same_device, _stream


def _params(seed: int, step: int, sub: int, e0: int) -> _lib.SrParams:
    for name, v, bits in (("seed", seed, 64), ("step", step, 32), ("sub", sub, 32), ("e0", e0, 64)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
        if not 0 <= v < 1 << bits:
            raise ValueError(f"{name} must be in [0, 2^{bits}), got {v}")
    if e0 % 4:
        raise ValueError(f"e0 must be a multiple of 4, got {e0}: a lane's 4 values share one Philox call")
    return _lib.SrParams(seed, e0, step, sub)


def check_seed(seed) -> int:
    """The key of a random stream: an int in [0, 2^64), refused by name otherwise.  For callers that
    take a seed long before they round with it (loopback.worker_serve)."""
    _params(seed, 0, 0, 0)
    return seed


def _out(x: torch.Tensor, out, dtype):
    out = torch.empty(x.shape, dtype=dtype, device=x.device) if out is None else out
    _fits(out, x.numel())
    _req(out, dtype, "out")
    _same_device(x, out)
    return out


def quantize(x: torch.Tensor, k: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
             base: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize of x - base, rounded stochastically: int32."""
    xt = _req_grad(x, "x")
    prm = _params(seed, step, sub, e0)
    ops._base_arg(base, x.numel(), x, "x")
    out = _out(x, out, torch.int32)
    if xt:
        rc = load().ina_quantize_sr_x16_i32(x.data_ptr(), xt, _ptr(base), out.data_ptr(), x.numel(), k,
                                            C.byref(prm), _stream(x))
    else:
        rc = load().ina_quantize_sr_f32_i32(x.data_ptr(), _ptr(base), out.data_ptr(), x.numel(), k, C.byref(prm),
                                            _stream(x))
    check(rc, "sr.quantize")
    return out


def quantize_i16(x: torch.Tensor, k: int, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
                 base: torch.Tensor | None = None, out=None, overflow=None):
    """ops.quantize_i16 of x - base, rounded stochastically: (out int16, overflow), one flag per slot
    of V values (a slot is V values of x: with e0 != 0 the caller keeps lo a multiple of V)."""
    xt = _req_grad(x, "x")
    prm = _params(seed, step, sub, e0)
    if V <= 0:
        raise ValueError("V must be > 0")
    ops._base_arg(base, x.numel(), x, "x")
    out = _out(x, out, torch.int16)
    nslot = (x.numel() + V - 1) // V
    overflow = torch.empty(nslot, dtype=torch.uint8, device=x.device) if overflow is None else overflow
    _fits(overflow, nslot, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(x, overflow)
    if xt:
        rc = load().ina_quantize_sr_x16_i16_sat(x.data_ptr(), xt, _ptr(base), out.data_ptr(), x.numel(), k, V,
                                                overflow.data_ptr(), C.byref(prm), _stream(x))
    else:
        rc = load().ina_quantize_sr_f32_i16_sat(x.data_ptr(), _ptr(base), out.data_ptr(), x.numel(), k, V,
                                                overflow.data_ptr(), C.byref(prm), _stream(x))
    check(rc, "sr.quantize_i16")
    return out, overflow


def quantize_i16_wire(x: torch.Tensor, k: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """wire.quantize rounded stochastically: the int32 wire words q16 + (saturated << 22) of
    dist.ShardedAggregator(wire="i16", rounding="stochastic")."""
    xt = _req_grad(x, "x")
    prm = _params(seed, step, sub, e0)
    out = _out(x, out, torch.int32)
    if xt:
        rc = load().ina_quantize_sr_x16_i16_wire(x.data_ptr(), xt, out.data_ptr(), x.numel(), k, C.byref(prm),
                                                 _stream(x))
    else:
        rc = load().ina_quantize_sr_f32_i16_wire(x.data_ptr(), out.data_ptr(), x.numel(), k, C.byref(prm), _stream(x))
    check(rc, "sr.quantize_i16_wire")
    return out


# ---- the fused quantise + reduce calls (include/ina_reduce_sr.h) ---------------------------------
def _global_k(k, what: str) -> int:
    """The fused reduces round stochastically under one global k: scales per block are refused by name."""
    if k is None or isinstance(k, (str, torch.Tensor)):
        raise ValueError(f"{what} takes a global integer k, got {'an int8 tensor' if isinstance(k, torch.Tensor) else repr(k)}: "
                         f"block scales are not combined with stochastic rounding on the fused reduces "
                         f"(blk.quantize_reduce rounds to nearest)")
    if isinstance(k, bool) or not isinstance(k, numbers.Integral):
        raise TypeError(f"k must be an int, got {type(k).__name__}")
    return int(k)


def quantize_reduce(bufs, k: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.quantize_reduce with every summand rounded stochastically, one launch: the int32 sum (mod 2^32)
    over w of sr.quantize(bufs[w], k, seed, step, sub + w, e0) -- worker w draws from stream sub + w.  The
    buckets are float32, bfloat16 or float16, one dtype per call."""
    k = _global_k(k, "sr.quantize_reduce")
    bufs, n, xt = ops._grad_bufs(bufs)
    prm = _params(seed, step, sub, e0)
    out = torch.empty(n, dtype=torch.int32, device=bufs[0].device) if out is None else out
    _fits(out, n)
    _req(out, torch.int32, "out")
    _same_device(bufs[0], out)
    if xt:
        rc = load().ina_quantize_reduce_sr_x16_i32(_ptrs(bufs), xt, len(bufs), out.data_ptr(), n, k, C.byref(prm),
                                                   _stream(out))
    else:
        rc = load().ina_quantize_reduce_sr_f32_i32(_ptrs(bufs), len(bufs), out.data_ptr(), n, k, C.byref(prm),
                                                   _stream(out))
    check(rc, "sr.quantize_reduce")
    return out


def quantize_reduce_i16(bufs, k: int, V: int, seed: int, step: int = 0, sub: int = 0, e0: int = 0, out=None,
                        overflow=None):
    """ops.quantize_reduce_i16 with every summand rounded stochastically, one launch: (out int16, overflow) --
    each summand saturated at int16, the sum saturated once, one flag per slot of V values (1 where a
    summand or the sum saturated or a value was NaN).  With e0 != 0 the caller keeps e0 a multiple of V."""
    k = _global_k(k, "sr.quantize_reduce_i16")
    bufs, n, xt = ops._grad_bufs(bufs)
    prm = _params(seed, step, sub, e0)
    if isinstance(V, bool) or not isinstance(V, numbers.Integral) or V <= 0:
        raise ValueError("V must be > 0")
    dev = bufs[0].device
    out = torch.empty(n, dtype=torch.int16, device=dev) if out is None else out
    _fits(out, n)
    _req(out, torch.int16, "out")
    nslot = (n + V - 1) // V
    overflow = torch.empty(nslot, dtype=torch.uint8, device=dev) if overflow is None else overflow
    _fits(overflow, nslot, "overflow")
    _req(overflow, torch.uint8, "overflow")
    _same_device(bufs[0], out, overflow)
    if xt:
        rc = load().ina_quantize_reduce_sr_x16_i16_sat(_ptrs(bufs), xt, len(bufs), out.data_ptr(), n, k, V,
                                                       overflow.data_ptr(), C.byref(prm), _stream(out))
    else:
        rc = load().ina_quantize_reduce_sr_f32_i16_sat(_ptrs(bufs), len(bufs), out.data_ptr(), n, k, V,
                                                       overflow.data_ptr(), C.byref(prm), _stream(out))
    check(rc, "sr.quantize_reduce_i16")
    return out, overflow


def scale_for(amax: float, W: int, bits: int) -> int:
    """ops.scale_for with a whole quantum of rounding a value: the largest k in [-126, 127] with
    W * (amax * 2^k + 1) <= 2^(bits-1) - 1, so no W-way sum of stochastically rounded values clips."""
    k = C.c_int(0)
    check(load().ina_scale_for_sr(float(amax), int(W), int(bits), C.byref(k)), "sr.scale_for")
    return k.value


# ---- the packet path (include/ina_pkt_sr.h) ------------------------------------------------------
def _blk_degree(degree, W: int, bits: int) -> int:
    """ops._blk_degree under sr.scale_for's rule: a whole quantum of rounding a summand."""
    degree = W if degree is None else int(degree)
    if bits not in (16, 32):
        raise ValueError("bits must be 16 or 32")
    if degree < 1 or ((1 << (bits - 1)) - 1) / degree - 1.0 <= 0:
        raise ValueError(f"degree {degree} cannot be summed at {bits} bits")
    return degree


def _blk_f32(t, name: str):
    """Block scales under stochastic rounding take fp32 buckets: a bf16 / fp16 tensor is refused as such."""
    if isinstance(t, torch.Tensor) and t.dtype in _X16:
        raise ValueError(f"stochastic rounding with block scales takes fp32 buckets: {name} is {t.dtype}")


def _k_arg(k, auto: bool):
    """True for per-packet scales (an int8 tensor; None where the call can compute them)."""
    if isinstance(k, bool) or not (isinstance(k, (numbers.Integral, torch.Tensor)) or (auto and k is None)):
        raise TypeError("k must be an int" + (", an int8 tensor of per-packet scales, or None" if auto
                                              else " or an int8 tensor of per-packet scales"))
    return not isinstance(k, numbers.Integral)


def block_scales(xs, V: int, bits: int = 32, degree: int | None = None, base: torch.Tensor | None = None,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """ops.block_scales under sr.scale_for's rule: for each block of V values the k that
    ina_scale_for_sr gives for the block's max |xs[w][i] - base[i]|, `degree` summands (default: the
    number of buckets) and `bits`.  Ranks agree on a block's scale by taking the MIN of theirs."""
    V = _blk_v(V)
    if degree is not None:
        _blk_degree(degree, 0, bits)
    for i, x in enumerate([xs] if isinstance(xs, torch.Tensor) else list(xs)):
        _blk_f32(x, f"xs[{i}]")
    xs, n = ops._blk_bufs(xs, "xs")
    degree = _blk_degree(degree, len(xs), bits)
    ops._base_arg(base, n, xs[0], "xs")
    out = _blk_scales_arg(out, (n + V - 1) // V, xs[0], "out")
    check(load().ina_block_scales_sr_f32(_ptrs(xs), len(xs), _ptr(base), n, V, degree, bits, out.data_ptr(),
                                         _stream(xs[0])), "sr.block_scales")
    return out


def quantize_pack_nga(x: torch.Tensor, k, V: int, bitmap: int, count: int, switch_id: int, seq0: int, seed: int,
                      step: int = 0, sub: int = 0, e0: int = 0, base: torch.Tensor | None = None, flags: int = 0,
                      num_slots: int = NUM_REGISTER, stride: int | None = None, out: torch.Tensor | None = None,
                      desc=None):
    """ops.quantize_pack_nga rounded stochastically, one launch: the packets of ops.pack_nga on
    sr.quantize(x, k, seed, step, sub, e0, base).  k an int (x float32, bfloat16 or float16), or an int8
    tensor of per-packet scales as in ops.quantize_pack_nga_blk (x float32).  Returns what
    ops.quantize_pack_nga returns."""
    prm_sr = _params(seed, step, sub, e0)
    blk = _k_arg(k, auto=False)
    if blk:
        V = _blk_v(V)
        _blk_f32(x, "x")
        _req(x, torch.float32, "x")
        xt = 0
    else:
        xt = _req_grad(x, "x")
    ops._base_arg(base, x.numel(), x, "x")
    stride = stride or ops.nga_stride(V)
    npk = (x.numel() + V - 1) // V
    if blk:
        k = _blk_scales_arg(k, npk, x, given=True)
    out = torch.empty((npk, stride), dtype=torch.uint8, device=x.device) if out is None else out
    _req(out, torch.uint8, "out")
    _fits(out, npk * stride)
    _same_device(x, out)
    prm = ops._nga_params(V, bitmap, count, switch_id, seq0, flags, num_slots)
    d = ops._desc_arg(desc, npk, x.device)
    bp, dp, sp = _ptr(base), _ptr(d), C.byref(prm_sr)
    if blk:
        rc = load().ina_quantize_pack_nga_blk_sr_desc(x.data_ptr(), bp, x.numel(), k.data_ptr(), C.byref(prm),
                                                      out.data_ptr(), stride, dp, sp, _stream(x))
    elif xt:
        rc = load().ina_quantize_pack_nga_x16_sr_desc(x.data_ptr(), xt, bp, x.numel(), int(k), C.byref(prm),
                                                      out.data_ptr(), stride, dp, sp, _stream(x))
    else:
        rc = load().ina_quantize_pack_nga_sr_desc(x.data_ptr(), bp, x.numel(), int(k), C.byref(prm), out.data_ptr(),
                                                  stride, dp, sp, _stream(x))
    check(rc, "sr.quantize_pack_nga")
    return (out, d) if d is not None else out


def quantize_pack_nga_multi_split(xs, k, V: int, bitmaps, count: int, switch_id: int, seq0, seed: int,
                                  step: int = 0, sub: int = 0, e0: int = 0, base: torch.Tensor | None = None,
                                  degree: int | None = None, kblk_out: torch.Tensor | None = None, flags: int = 0,
                                  num_slots: int = NUM_REGISTER, hdrs=None, pays=None, descs=None):
    """W workers' stochastic quantise + split pack in one launch, worker w drawing from stream sub + w.
    k an int: ops.quantize_pack_nga_multi_split (float32, bfloat16 or float16 buckets of one dtype),
    returns (hdrs, pays) or (hdrs, pays, descs).  k an int8 tensor (one scale per packet) or None (the
    scales computed from these workers' deltas for `degree` summands under sr.scale_for's rule):
    ops.quantize_pack_nga_multi_split_blk (float32 buckets), returns the same plus the scales."""
    prm_sr = _params(seed, step, sub, e0)
    blk = _k_arg(k, auto=True)
    if blk:
        V = _blk_v(V)
        for i, x in enumerate([xs] if isinstance(xs, torch.Tensor) else list(xs)):
            _blk_f32(x, f"xs[{i}]")
        xs, n = ops._blk_bufs(xs, "xs")
        xt = 0
    else:
        xs, n, xt = ops._grad_bufs(xs, "xs")
    W, dev = len(xs), xs[0].device
    ops._base_arg(base, n, xs[0], "xs")
    keys = ops._worker_keys(W, bitmaps, seq0)
    npk = (n + V - 1) // V
    if blk:
        mode = _lib.BLK_AUTO if k is None else _lib.BLK_GIVEN
        degree = _blk_degree(degree, W, 32) if k is None else 1
        kblk = _blk_scales_arg(k if k is not None else kblk_out, npk, xs[0])
    hdrs, pays = ops._worker_rows(hdrs, pays, W, npk, V, dev)
    _same_device(xs[0], *hdrs, *pays)
    ds = ops._worker_descs(descs, W, npk, dev)
    prm = ops._worker_params(V, keys, count, switch_id, flags, num_slots)
    xa, bp, ha, pa, da, sp = _ptrs(xs), _ptr(base), _ptrs(hdrs), _ptrs(pays), _ptrs(ds), C.byref(prm_sr)
    if blk:
        rc = load().ina_quantize_pack_nga_multi_split_blk_sr(xa, W, bp, n, kblk.data_ptr(), mode, degree, prm, ha, pa,
                                                             da, sp, _stream(xs[0]))
    elif xt:
        rc = load().ina_quantize_pack_nga_multi_split_x16_sr(xa, xt, W, bp, n, int(k), prm, ha, pa, da, sp,
                                                             _stream(xs[0]))
    else:
        rc = load().ina_quantize_pack_nga_multi_split_sr(xa, W, bp, n, int(k), prm, ha, pa, da, sp, _stream(xs[0]))
    check(rc, "sr.quantize_pack_nga_multi_split")
    res = (hdrs, pays, ds) if ds is not None else (hdrs, pays)
    return res + (kblk,) if blk else res
