"""GPU parity of the block-scaled int16 wire (include/ina_shard_blk.h) and of k="block" in
ina_amd.dist on one rank, bit for bit against the CPU oracle called with each block's own k
(tests/_blk_ref.py, tests/_shard_blk_ref.py).  The library is never compared with itself."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _blk_ref as ref
from tests._shard_blk_ref import DEV, Expected, finish_ref, given_scales, ranks_bucket, run_case, same
from tests.conftest import REPO

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 255, 1000, 65_536 + 5)
VEC_V, SCALAR_V = (8, 32, 256), (100, 512, 1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


# ---- the two kernels --------------------------------------------------------------------------
@pytest.mark.parametrize("V", VEC_V + SCALAR_V)
@pytest.mark.parametrize("n", NS)
def test_kernel_parity_given_and_agreed_scales(n, V):
    """Three ranks' wires, their int64 sum and its finish (int16, y as bit patterns, flags, and the
    flags-only call over a buffer of 7s), every buffer aligned and offset by one element (the scalar
    path).  Given scales: the agreed ones + 3 on every third block, where single ranks and the sum
    saturate.  Agreed scales: the finish is the one-GPU reduce and only NaN / inf blocks are flagged."""
    x = ranks_bucket(n, V, 7000 + 13 * V + n)
    nblk = (n + V - 1) // V
    given = Expected(x, given_scales(x, V), V)
    if nblk >= 3:                                   # fewer blocks cannot hold both kinds
        assert given.flags.any() and not given.flags.all()
        assert any(((w.astype(np.int64) + (1 << 21)) >> 22).any() for w in given.wires)   # a single rank saturates too
    kb = ref.kblk_ref(x, V, degree=3, bits=16)
    agreed = Expected(x, kb, V)
    r16, rf = ref.quantize_reduce_i16(x, kb, V)                     # the one-GPU path
    same(agreed.o16, r16, "oracle: wire finish == fused reduce")
    same(agreed.flags, rf, "oracle: wire flags == fused reduce flags")
    special = np.array([not np.isfinite(x[:, sl]).all() for sl in ref.blocks(n, V)], np.uint8)
    same(agreed.flags, special, "only NaN / inf blocks are flagged")
    for off in (0, 1):
        run_case(given, off, f"given n={n} V={V} off={off}")
        run_case(agreed, off, f"agreed n={n} V={V} off={off}")


@pytest.mark.parametrize("V", (32, 100))
def test_a_given_minus_128_is_read_as_minus_126(V):
    from ina_amd import ops
    n = 5 * V + 3
    rng = np.random.default_rng(128)
    x = (rng.standard_normal(n) * 1e38).astype(np.float32)           # a few units at 2^-126
    for low in (-128, -127):
        kb = np.full(6, low, np.int8)
        at126 = np.full(6, -126, np.int8)
        want = np.concatenate([ref.orc.quantize_i16_wire(x[sl], -126) for sl in ref.blocks(n, V)])
        assert np.abs(want & 0xFFFF).max() > 0
        same(ops.quantize_i16_wire_blk(dev(x), dev(kb), V), want, f"wire at {low}")
        wsum = (want.astype(np.int64) * 2).astype(np.int32)
        w16, wy, wf = finish_ref(wsum, at126, V)
        g16, gy, gf = ops.i16_wire_finish_blk(dev(wsum), dev(kb), V)
        same(g16, w16, f"finish int16 at {low}")
        same(gy, wy, f"finish y at {low}")
        same(gf, wf, f"finish flags at {low}")


@pytest.mark.parametrize("V", (32, 100))
def test_shard_offset_reads_its_slice_and_writes_inside_its_outputs(V):
    """A slice starting at block 5, finished with kblk[5:], equals the same rows of the whole-bucket
    finish; the bytes around out16, y and the flags stay as they were."""
    from ina_amd import ops
    n, first = 40 * V + 5, 5
    x = ranks_bucket(n, V, 555)
    exp = Expected(x, given_scales(x, V), V)
    m, mblk = n - first * V, 41 - first
    G = 64                                                               # guard elements on either side
    kbd = dev(exp.kb)
    src = dev(exp.wsum)[first * V:]
    assert src.data_ptr() % 16 == 0
    o16 = torch.full((m + 2 * G,), 0x5555, dtype=torch.int16, device=DEV)
    y = torch.full((m + 2 * G,), float("nan"), dtype=torch.float32, device=DEV)
    fl = torch.full((mblk + 2 * G,), 7, dtype=torch.uint8, device=DEV)
    ops.i16_wire_finish_blk(src, kbd[first:], V, out16=o16[G:G + m], y=y[G:G + m], overflow=fl[G:G + mblk])
    same(o16[G:G + m], exp.o16[first * V:], "shard int16")
    same(y[G:G + m], exp.y[first * V:], "shard y")
    same(fl[G:G + mblk], exp.flags[first:], "shard flags")
    for t, fill in ((o16, 0x5555), (fl, 7)):
        assert (host(t[:G]) == fill).all() and (host(t[-G:]) == fill).all()
    assert np.isnan(host(y[:G])).all() and np.isnan(host(y[-G:])).all()
    # the wire quantiser on the same slice, with the slice's scales
    w = torch.full((m + 2 * G,), 0x55555555, dtype=torch.int32, device=DEV)
    ops.quantize_i16_wire_blk(dev(x[0])[first * V:], kbd[first:], V, out=w[G:G + m])
    same(w[G:G + m], exp.wires[0][first * V:], "shard wire")
    assert (host(w[:G]) == 0x55555555).all() and (host(w[-G:]) == 0x55555555).all()


def test_grid_stride_with_the_default_cap_lowered():
    """set_tuning(max_blocks=2), then n = 65,536 + 5; the tuning is restored afterwards."""
    from ina_amd import ops
    n, V = 65_536 + 5, 32
    x = ranks_bucket(n, V, 932)
    exp = Expected(x, given_scales(x, V), V)
    ops.set_tuning(max_blocks=2)
    try:
        for off in (0, 1):
            run_case(exp, off, f"max_blocks=2 off={off}")
    finally:
        ops.set_tuning(max_blocks=16384)


def test_grid_stride_under_the_lab_build():
    """The grids of these kernels take the elementwise cap (tuning key 14, as their global-k
    siblings do), which only the lab build of the library lets a caller lower: the same case in a
    child process under libina_lab.so with a grid of two workgroups, so every thread strides."""
    from ina_amd import _lib
    lab = os.path.join(os.path.dirname(_lib.LIB_PATH), "libina_lab.so")
    assert os.path.exists(lab), f"{lab} is not built (make -C csrc lab; __graft_entry__.build() makes it)"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_shard_blk_ref.py")], cwd=REPO,
                       env=dict(os.environ, INA_LIBRARY="libina_lab.so"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "shard blk lab child ok" in r.stdout


# ---- the classes on one rank ------------------------------------------------------------------
def _bucket1(seed, n):
    rng = np.random.default_rng(seed)
    x = ref.bucket(rng, 1, n, 32)[0]
    x[7] = np.nan
    return x


@pytest.mark.parametrize("collective", ("rs_ag", "a2a", "allreduce"))
@pytest.mark.parametrize("wire", ("i16", "i32"))
def test_sharded_aggregator_block_scales_on_one_rank(wire, collective):
    from ina_amd.dist import ShardedAggregator
    n, V = 70_001, 32
    x = _bucket1(71, n)
    bits = 16 if wire == "i16" else 32
    kb = ref.kblk_ref([x], V, degree=1, bits=bits)
    if wire == "i16":
        want_int, want_f = ref.quantize_reduce_i16([x], kb, V)
        assert want_f.sum() == 1
    else:
        want_int = ref.quantize_reduce_i32([x], kb, V)
    want = ref.dequantize(want_int, kb, V)
    agg = ShardedAggregator(n, k="block", device=torch.device(DEV), wire=wire, V=V, collective=collective)
    assert agg.scale_bytes == 0 and agg.gather_bytes == 0
    xd = dev(x)
    ptrs = None
    for call in (1, 2):                                    # the second call reuses the buffers
        full = agg(xd)
        same(full, want, f"full, call {call}")
        same(agg.kblk, kb, f"kblk, call {call}")
        if wire == "i16":
            same(agg.overflow, want_f, f"overflow, call {call}")
        now = (full.data_ptr(), agg.kblk.data_ptr(), agg.q.data_ptr())
        assert ptrs in (None, now)
        ptrs = now
    same(agg.aggregate_int(xd)[:n], want_int, "aggregate_int")
    same(agg.kblk, kb, "kblk beside the integers")


@pytest.mark.parametrize("wire", ("i16", "i32"))
def test_range_aggregator_block_scales_on_one_rank(wire):
    from ina_amd.dist import RangeAggregator
    n, V, W = 70_001, 32, 3
    x = np.stack([_bucket1(80 + w, n) for w in range(W)])
    x[1:, 7] = 1.0                                         # one NaN in all
    bits = 16 if wire == "i16" else 32
    kb = ref.kblk_ref(x, V, degree=W, bits=bits)
    if wire == "i16":
        want_int, want_f = ref.quantize_reduce_i16(x, kb, V)
        assert want_f.sum() == 1
    else:
        want_int = ref.quantize_reduce_i32(x, kb, V)
    want = ref.dequantize(want_int, kb, V)
    agg = RangeAggregator(n, k="block", device=torch.device(DEV), wire=wire, V=V)
    assert agg.range == (0, n) and agg.gather_bytes == 0
    xs = [dev(r) for r in x]
    ptrs = None
    for call in (1, 2):
        full = agg(xs)
        same(full, want, f"full, call {call}")
        same(agg.kblk, kb, f"kblk, call {call}")
        if wire == "i16":
            same(agg.overflow, want_f, f"overflow, call {call}")
        now = (full.data_ptr(), agg.kblk.data_ptr())
        assert ptrs in (None, now)
        ptrs = now
    same(agg.aggregate_int(xs), want_int, "aggregate_int")


# ---- what it buys -----------------------------------------------------------------------------
def test_int16_wire_accuracy_under_block_scales():
    """test_gpu_blk.py's 96-block bucket (magnitudes 1e-9 .. 1e3), W = 4, int16 wire, through
    RangeAggregator.  k="block": every block within W * amax_s / (32767 / W - 1/2) of the float64
    sum -- each of the W roundings is <= 2^-k / 2, and k + 1 failing ina_scale_for's test gives
    2^-k < 2 * amax_s / lim -- and no flag.  At the scale_for_workers global k the oracle returns
    more than half of the blocks as all zeros."""
    from ina_amd import ops
    from ina_amd.dist import RangeAggregator
    W, V, nblk = 4, 32, 96
    n = nblk * V
    x = ref.bucket(np.random.default_rng(20260), W, n, V)
    xs = [dev(r) for r in x]
    agg = RangeAggregator(n, k="block", device=torch.device(DEV), wire="i16", V=V)
    y = host(agg(xs)).astype(np.float64)
    assert not host(agg.overflow).any()
    exact = x.astype(np.float64).sum(0)
    lim = 32767.0 / W - 0.5
    for s, sl in enumerate(ref.blocks(n, V)):
        amax = float(np.abs(x[:, sl]).max())
        err = float(np.abs(y[sl] - exact[sl]).max())
        assert err <= W * amax / lim, (s, err, W * amax / lim)
    k = ops.scale_for(float(np.abs(x).max()), W, bits=16)             # the host rule: scale_for_workers' k
    assert k == ops.scale_for_workers(xs, bits=16)
    g16, _ = ref.orc.quantize_reduce_i16_sat(list(x), k, V)           # the oracle's count
    zero = sum(1 for sl in ref.blocks(n, V) if not g16[sl].any())
    assert zero > nblk // 2, zero
    glob = RangeAggregator(n, k=k, device=torch.device(DEV), wire="i16", V=V)
    same(glob(xs), ref.orc.dequantize_i16(g16, k), "the global-k aggregate is the oracle's")


# ---- stream_store at the addresses that broke it ----------------------------------------------
GiB = 1 << 30
N_VIEW = 1 << 16


@pytest.fixture(scope="module")
def arena():
    """4 GiB + slack: some address in it has a low word of exactly 2^31."""
    slack = 4 << 20
    buf = torch.empty(4 * GiB + slack, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    b31 = (((base + (1 << 20) - (1 << 31) + (1 << 32) - 1) >> 32) << 32) + (1 << 31)
    assert base + (1 << 20) <= b31 and b31 + (1 << 20) < base + buf.numel()
    yield buf, base, b31
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", ("wire", "out16", "y"))
def test_stream_store_views_across_bit_31(arena, case):
    """wire, out16 and y written into views that straddle bit 31 of the low address word (+48: a
    wave's run of stores then always crosses it) equal the same call into an ordinary allocation,
    and the bytes around the view stay untouched."""
    from ina_amd import ops
    buf, base, b31 = arena
    V = 32
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(N_VIEW, device=DEV, generator=g) * 2.0
    kb = ops.block_scales([x], V, bits=16, degree=1)
    kb[::3] += 2                                                     # some blocks saturate
    wire = ops.quantize_i16_wire_blk(x, kb, V)
    dtype, fn = {"wire": (torch.int32, lambda o: ops.quantize_i16_wire_blk(x, kb, V, out=o)),
                 "out16": (torch.int16, lambda o: ops.i16_wire_finish_blk(wire, kb, V, out16=o, want_y=False)),
                 "y": (torch.float32, lambda o: ops.i16_wire_finish_blk(wire, kb, V, y=o, want_out16=False))}[case]
    ref_out = torch.empty(N_VIEW, dtype=dtype, device=DEV)
    fn(ref_out)
    esz = ref_out.element_size()
    nbytes = N_VIEW * esz
    addr = b31 - ((nbytes // 2) & ~1023) + 48
    assert (addr & 0xFFFFFFFF) < (1 << 31) <= ((addr + nbytes - 1) & 0xFFFFFFFF)
    off, GUARD = addr - base, 4096
    view = buf[off:off + nbytes].view(dtype)
    view.fill_(0x55 if dtype != torch.float32 else float("nan"))

    def guards():
        return torch.cat([buf[off - GUARD:off], buf[off + nbytes:off + nbytes + GUARD]]).clone()
    before = guards()
    fn(view)
    torch.cuda.synchronize()
    assert np.array_equal(host(view).view(np.uint8), host(ref_out).view(np.uint8)), case
    assert torch.equal(guards(), before), case
