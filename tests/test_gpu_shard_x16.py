"""bf16 / fp16 buckets on the sharded int16 wire (include/ina_shard_x16.h, ina_amd.wire) and under both
aggregators at world 1, on the GPU.

One rule throughout: widening is exact, so a wire word is bit for bit the oracle's on the widened bucket
(tests/_shard_blk_ref.wire_ref for the block form); in the finishes out16 and the flags are the fp32
sibling's, and a 16-bit y is bit for bit ops.dequantize / blk.dequantize of out16 into that dtype and the
sibling's fp32 y converted on the CPU with .to(dtype) (one rounding to nearest even).  Every equality is
on the bits.  The widened references are made on the CPU (tensor.float(), exact) and shared."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _shard_blk_ref as sref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
SIZES = (1, 5, 255, 256, 257, 4099)
VS = (8, 32, 256, 12)                    # 12: no power of two, the value-by-value kernels
GUARD = 8
WSHIFT = 22


def bits(t):
    """A tensor's values as unsigned integers of its width (numpy)."""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).numpy().view(f"u{t.element_size()}")


def same(got, want, what):
    g, w = bits(got), (bits(want) if isinstance(want, torch.Tensor) else np.ascontiguousarray(want).view(f"u{want.itemsize}"))
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, g.dtype, w.shape, w.dtype)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {g[bad[0]]:#x} != {w[bad[0]]:#x}"


class Guarded:
    """n elements `off` elements into an allocation with GUARD sentinel elements on either side: .t is
    the view a call gets, check() that nothing around it was written."""

    def __init__(self, n, dtype, off=0, fill=None):
        self.n, self.off = n, off
        raw = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]
        self.buf = torch.full((GUARD + off + n + GUARD,), 0x5A, dtype=raw, device=DEV).view(dtype)
        self.t = self.buf[GUARD + off: GUARD + off + n]
        if fill is not None:
            self.t.copy_(fill)
        self.before = bits(self.buf)

    def check(self, what):
        now = bits(self.buf)
        lo = GUARD + self.off
        assert np.array_equal(now[:lo], self.before[:lo]) and np.array_equal(now[lo + self.n:], self.before[lo + self.n:]), \
            f"{what}: bytes outside the buffer were written"


@functools.lru_cache(maxsize=None)
def patterns(dtype):
    """All 65,536 bit patterns of a 16-bit type, and their exact fp32 values."""
    t = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16)).view(dtype)
    return t, t.float().numpy()


@functools.lru_cache(maxsize=None)
def bucket(dtype, n, seed=0):
    """n values of the type: a few units of the int16 range at k = 9 (single values clip), small ones,
    a NaN, both infinities and a zero where there is room.  (16-bit tensor, its exact fp32 values)"""
    rng = np.random.default_rng(1000 * seed + n)
    x = rng.standard_normal(n) * rng.choice([1e-3, 1.0, 40.0, 200.0], n)
    t = torch.from_numpy(x.astype(np.float32)).to(dtype)
    if n >= 16:
        t[3], t[n - 2], t[n // 2], t[7] = float("nan"), float("inf"), float("-inf"), 0.0
    return t, t.float().numpy()


def scales(n, V, seed=0):
    """One int8 per block: scales around 9 (values clip at the higher ones), with -128, -127 (read as
    -126) and 127 where there are blocks for them."""
    nblk = (n + V - 1) // V
    kb = np.random.default_rng(77 + seed + n + V).choice(np.array([5, 9, 12, 14], np.int8), nblk)
    for i, k in ((1, -128), (2, -127), (3, 127)):
        if nblk > i:
            kb[i] = k
    return kb


# ---- the wire quantisers ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_bit_pattern_in_one_call(dtype):
    """n = 65,536: every value of the type, NaNs, infinities, subnormals and both zeros included, at k = 9
    and at k = 120, where nearly every non-zero value clips."""
    from ina_amd import wire
    t, wide = patterns(dtype)
    x = t.to(DEV)
    for k in (9, 120):
        want = orc.quantize_i16_wire(wide, k)
        if k == 120:
            assert np.count_nonzero((want + (1 << (WSHIFT - 1))) >> WSHIFT) > 0.8 * np.count_nonzero(wide != 0)
        same(wire.quantize(x, k), want, f"{dtype} k={k}")
    for V in (32, 12):
        kb = np.random.default_rng(V).choice(np.array([-128, -127, -20, 0, 9, 15, 100, 127], np.int8), 65536 // V + 1)
        got = wire.quantize_blk(x, torch.from_numpy(kb).to(DEV), V)
        same(got, sref.wire_ref(wide, kb, V), f"{dtype} block form V={V}")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantisers_sizes_paths_and_guard_bytes(dtype, off):
    """off = 1: the bucket starts 2 bytes and the wire 4 bytes into an aligned allocation, so both miss the
    vector path's alignment."""
    from ina_amd import wire
    for n in SIZES:
        t, wide = bucket(dtype, n)
        x = Guarded(n, dtype, off, fill=t.to(DEV))
        for k in (9, 127, -126):
            w = Guarded(n, torch.int32, off)
            assert wire.quantize(x.t, k, out=w.t) is w.t
            same(w.t, orc.quantize_i16_wire(wide, k), f"{dtype} n={n} off={off} k={k}")
            w.check(f"wire n={n} k={k}")
        for V in VS:
            kb = scales(n, V)
            kbd = Guarded(kb.size, torch.int8, 0, fill=torch.from_numpy(kb).to(DEV))
            w = Guarded(n, torch.int32, off)
            wire.quantize_blk(x.t, kbd.t, V, out=w.t)
            same(w.t, sref.wire_ref(wide, kb, V), f"{dtype} n={n} off={off} V={V}")
            w.check(f"block wire n={n} V={V}")
        x.check("the bucket")


# ---- the finishes ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def summed_wire(n, ranks):
    """The int32 SUM of `ranks` ranks' wire words: int16 values over the whole range (the sum clips in
    places once ranks > 1), a rank's saturation bit set on about one value in 50."""
    rng = np.random.default_rng(31 * ranks + n)
    q = rng.integers(-32768, 32768, (ranks, n)) // rng.choice([1, 1, 7, 300], (ranks, n))
    sat = rng.random((ranks, n)) < 0.02
    return (q + (sat.astype(np.int64) << WSHIFT)).sum(axis=0).astype(np.int32)


def check_finish(dtype, n, ranks, V, off, k=None, kb=None):
    """One summed wire through the 16-bit finish in its four call shapes, against the fp32 sibling, the
    oracle and the 16-bit dequantise."""
    from ina_amd import blk, ops, wire
    tag = f"{dtype} n={n} ranks={ranks} V={V} off={off} k={k if kb is None else 'block'}"
    ws = summed_wire(n, ranks)
    src = Guarded(n, torch.int32, off, fill=torch.from_numpy(ws).to(DEV))
    nslot = (n + V - 1) // V
    if kb is None:
        fin = lambda **kw: wire.finish(src.t, k, V, **kw)                                     # noqa: E731
        s16, sy, sf = ops.i16_wire_finish(src.t, k, V)
        deq = lambda o16: ops.dequantize(o16, k, dtype=dtype)                                 # noqa: E731
        r16, ry, rf = orc.i16_wire_finish(ws, k, V)
    else:
        kbd = torch.from_numpy(kb).to(DEV)
        fin = lambda **kw: wire.finish_blk(src.t, kbd, V, **kw)                               # noqa: E731
        s16, sy, sf = ops.i16_wire_finish_blk(src.t, kbd, V)
        deq = lambda o16: blk.dequantize(o16, kbd, V, dtype=dtype)                            # noqa: E731
        r16, ry, rf = sref.finish_ref(ws, kb, V)
    same(s16, r16, "sibling out16 " + tag), same(sy, ry, "sibling y " + tag), same(sf, rf, "sibling flags " + tag)
    want_y = sy.cpu().to(dtype)                          # the fp32 result rounded once, on the CPU
    # everything, flags given (every one is written)
    o16, y, f = Guarded(n, torch.int16, off), Guarded(n, dtype, off), Guarded(nslot, torch.uint8)
    got = fin(out16=o16.t, y=y.t, overflow=f.t)
    assert got[0] is o16.t and got[1] is y.t and got[2] is f.t
    same(o16.t, s16, "out16 " + tag), same(f.t, sf, "flags " + tag)
    same(y.t, want_y, "y against the sibling's rounded " + tag)
    same(y.t, deq(s16), "y against the 16-bit dequantise of out16 " + tag)
    for g, what in ((o16, "out16"), (y, "y"), (f, "flags")):
        g.check(f"{what} {tag}")
    # flags not given, dtype= in place of y
    a16, ay, af = fin(dtype=dtype)
    assert ay.dtype == dtype and af.numel() == nslot
    same(a16, s16, "out16, allocated " + tag), same(ay, want_y, "y, allocated " + tag), same(af, sf, "flags, allocated " + tag)
    # y alone, and out16 alone (the type code then comes from dtype=)
    y2 = Guarded(n, dtype, off)
    b16, by, bf = fin(y=y2.t, want_out16=False)
    assert b16 is None and by is y2.t
    same(y2.t, want_y, "y alone " + tag), same(bf, sf, "flags, y alone " + tag)
    y2.check("y alone " + tag)
    c16, cy, cf = fin(want_y=False, dtype=dtype)
    assert cy is None
    same(c16, s16, "out16 alone " + tag), same(cf, sf, "flags, out16 alone " + tag)
    src.check("the summed wire")
    return y.t


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_finishes_sizes_paths_and_guard_bytes(dtype, off):
    for n, ranks in zip(SIZES, (1, 2, 3, 17, 64, 64)):
        for V in VS:
            check_finish(dtype, n, ranks, V, off, k=9)
            check_finish(dtype, n, ranks, V, off, kb=scales(n, V))
    check_finish(dtype, 257, 64, 32, off, k=127)
    check_finish(dtype, 257, 64, 32, off, k=-126)


def test_fp16_results_past_the_largest_finite_value_become_inf():
    """k = -2: |sum| * 4 rounds past 65,504, the largest finite fp16, from |sum| = 16,380 on; bf16 holds every such value."""
    for V, kb in ((32, None), (32, np.full(129, -2, np.int8))):
        y = check_finish(torch.float16, 4099, 3, V, 0, k=-2, kb=kb)
        ws16 = orc.i16_wire_finish(summed_wire(4099, 3), -2, V)[0].astype(np.int64)
        big = np.abs(ws16) * 4 >= 65520                  # rounds to 2^16, past the largest finite fp16
        assert big.sum() > 100
        assert np.array_equal(np.isinf(y.float().cpu().numpy()), big)
        assert not np.isinf(check_finish(torch.bfloat16, 4099, 3, V, 0, k=-2, kb=kb).float().cpu().numpy()).any()


# ---- the grid-stride passes --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_stride_at_a_grid_of_two_workgroups(dtype):
    """set_tuning(max_blocks=2) holds the four launches to 512 threads: n = 4099 is 1025 chunks, three
    passes of the vector kernels, and nine of the value-by-value ones (V = 12, or one element in)."""
    from ina_amd import ops, wire
    n = 4099
    t, wide = bucket(dtype, n)
    ops.set_tuning(max_blocks=2)
    try:
        for off in (0, 1):
            x = Guarded(n, dtype, off, fill=t.to(DEV))
            w = Guarded(n, torch.int32, off)
            wire.quantize(x.t, 9, out=w.t)
            same(w.t, orc.quantize_i16_wire(wide, 9), f"{dtype} off={off}")
            w.check("wire")
            for V in (32, 12):
                kb = scales(n, V)
                w = Guarded(n, torch.int32, off)
                wire.quantize_blk(x.t, torch.from_numpy(kb).to(DEV), V, out=w.t)
                same(w.t, sref.wire_ref(wide, kb, V), f"{dtype} off={off} V={V}")
                w.check("block wire")
                check_finish(dtype, n, 64, V, off, k=9)
                check_finish(dtype, n, 64, V, off, kb=kb)
    finally:
        ops.set_tuning(max_blocks=16384)


# ---- the aggregators at world 1 ----------------------------------------------------------------------
def agg_bucket(dtype, n, V, k):
    """A bucket whose values clip in places at k = 9 and whose blocks carry different scales."""
    rng = np.random.default_rng(n + V)
    x = rng.standard_normal(n) * np.repeat(2.0 ** rng.integers(-6, 8, (n + V - 1) // V), V)[:n]
    t = torch.from_numpy(x.astype(np.float32)).to(dtype)
    t[5], t[n - 3] = float("nan"), float("inf")
    return t.to(DEV)


@pytest.mark.parametrize("coll", ["rs_ag", "allreduce"])
@pytest.mark.parametrize("k", [9, "block"])
@pytest.mark.parametrize("wire_name", ["i16", "i32"])
def test_sharded_aggregator_world_1(wire_name, k, coll):
    from ina_amd.dist import ShardedAggregator
    n, V = 4099, 32
    for dtype in DTYPES:
        g = agg_bucket(dtype, n, V, k)
        ref = ShardedAggregator(n, k=k, wire=wire_name, V=V, collective=coll, device=torch.device(DEV))
        want = ref(g.float()).clone()
        for out_dtype in (torch.float32, dtype):
            agg = ShardedAggregator(n, k=k, wire=wire_name, V=V, collective=coll, device=torch.device(DEV),
                                    out_dtype=out_dtype)
            got = agg(g)
            tag = f"{wire_name} k={k} {coll} {dtype} -> {out_dtype}"
            assert got.dtype == out_dtype and agg.gather_bytes == 0
            same(got, want if out_dtype == torch.float32 else want.cpu().to(dtype), tag)
            if wire_name == "i16":
                same(agg.overflow, ref.overflow, "flags " + tag)
                assert bits(agg.overflow).any()
            if k == "block":
                same(agg.kblk, ref.kblk, "kblk " + tag)
        with pytest.raises(TypeError, match=f"error_feedback=True takes float32 buckets, got {dtype}"):
            ShardedAggregator(n, k=k, wire=wire_name, V=V, collective=coll, device=torch.device(DEV),
                              error_feedback=True)(g)


@pytest.mark.parametrize("k", [9, "block"])
@pytest.mark.parametrize("wire_name", ["i16", "i32"])
def test_range_aggregator_world_1(wire_name, k):
    from ina_amd.dist import RangeAggregator
    W, V = 3, 32
    n = 3 * V + 5
    for dtype in DTYPES:
        slices = [agg_bucket(dtype, n, V, k) * (w + 1) for w in range(W)]
        ref = RangeAggregator(n, k=k, wire=wire_name, V=V, device=torch.device(DEV))
        want = ref([s.float() for s in slices]).clone()
        for out_dtype in (torch.float32, dtype):
            agg = RangeAggregator(n, k=k, wire=wire_name, V=V, device=torch.device(DEV), out_dtype=out_dtype)
            got = agg(slices)
            tag = f"range {wire_name} k={k} {dtype} -> {out_dtype}"
            assert got.dtype == out_dtype
            same(got, want if out_dtype == torch.float32 else want.cpu().to(dtype), tag)
            if wire_name == "i16":
                same(agg.overflow, ref.overflow, "flags " + tag)
            if k == "block":
                same(agg.kblk, ref.kblk, "kblk " + tag)
        with pytest.raises(TypeError, match="all workers of one call share one dtype"):
            RangeAggregator(n, k=k, wire=wire_name, V=V, device=torch.device(DEV))([slices[0], slices[1].float()])
