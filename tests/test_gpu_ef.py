"""Error feedback for the quantiser on the device (include/ina_ef.h, ina_amd.ef).

Replay: every q, r', flag and scale is bit for bit the CPU oracle's quantiser applied to
v = (x - base) + r with the three numpy float32 operations of tests/_ef_ref.py around it.  Zero
residual: with r = 0 every q, flag, scale and packet row equals the non-EF sibling's.  Conservation:
on inputs where every fp32 operation is exact, what was sent plus the residual left is, in float64 and
with ==, what was meant to be sent -- where the plain quantiser sends nothing at all."""
import os
import socket
import sys
import tempfile
import threading

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import oracle as orc
from tests import _blk_ref as bref
from tests import _ef_ref as eref
from tests.conftest import PKG_ROOT, REPO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 5, 255, 256, 257, 511, 512, 513, 4099)
VS = (8, 32, 256, 12)                 # 12: no ballot layout, the scalar path
K32, K16 = 10, 6
SAT32, SAT16 = 5.0e6, 1000.0          # |v| * 2^k past the int32 / int16 range
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ops():
    from ina_amd import ef, ops
    return ef, ops


def dev(a, off=0):
    """a on the device; off = 1: as a view one element into its allocation (the unaligned path)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.to(DEV)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t)
    return buf[off:]


def out_like(n, dtype, off):
    return torch.empty(n + off, dtype=dtype, device=DEV)[off:]


def host(t):
    return t.cpu().numpy()


SPECIALS = lambda sat: np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -3e-42, sat, -2 * sat, 0.0], F32)  # noqa: E731


def bucket(seed, n, sat, scale=0.3):
    """(x, r, base): seeded values with NaN, +-inf, -0.0, subnormals and saturating values among x
    (as many as n holds; the seed moves them), a finite seeded residual and a base."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * scale).astype(F32)
    sp = rng.permutation(SPECIALS(sat))[: min(n, 9)]
    pos = rng.choice(n, size=sp.size, replace=False)
    x[pos] = sp
    r = (rng.standard_normal(n) * 2.0 ** -(K32 + 1)).astype(F32)
    r[rng.choice(n, size=min(n, 2), replace=False)] = F32(-0.0)
    base = (rng.standard_normal(n) * scale).astype(F32)
    return x, r, base, pos


def same_f32(got, want, what):
    assert np.array_equal(eref.bits(got), eref.bits(want)), what


def given_scales(seed, nblk, lo, hi):
    kb = np.random.default_rng(seed).integers(lo, hi, nblk).astype(np.int8)
    for i, v in zip(range(1, nblk, 3), (-128, 127, -127, -126)):      # the ABI's edges, where there is room
        kb[i] = v
    return kb


# ---- replay parity --------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("with_base", [False, True])
def test_replay_global_i32(off, with_base):
    ef, _ = _ops()
    for n in SIZES:
        x, r, base, _ = bucket(n, n, SAT32)
        b = base if with_base else None
        rt = dev(r, off)
        q = ef.quantize(dev(x, off), rt, K32, base=dev(b, off) if with_base else None, out=out_like(n, torch.int32, off))
        wq, wr = eref.quantize(x, r, K32, b)
        assert np.array_equal(host(q), wq), n
        same_f32(host(rt), wr, n)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("V", VS + (512, 1024))
def test_replay_global_i16(V, off):
    """512: one slot is both 256-value halves of a wave; 1024: no ballot layout, the scalar path with
    a block larger than a wave's 512 values.  At both the expected flags at n = 4099 hold 0s and 1s."""
    ef, _ = _ops()
    for n in SIZES:
        for with_base in (False, True):
            x, r, base, _ = bucket(100 + n, n, SAT16)
            b = base if with_base else None
            rt = dev(r, off)
            q, f = ef.quantize_i16(dev(x, off), rt, K16, V, base=dev(b, off) if with_base else None,
                                   out=out_like(n, torch.int16, off))
            wq, wf, wr = eref.quantize_i16(x, r, K16, V, b)
            assert np.array_equal(host(q), wq), (n, with_base)
            assert np.array_equal(host(f), wf), (n, with_base)
            same_f32(host(rt), wr, (n, with_base))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_replay_x16_every_bit_pattern(dt):
    """All 65,536 bfloat16 / float16 values as one bucket (NaNs, infinities, subnormals, both zeros),
    against the replay on the exactly widened values; aligned and one element in."""
    ef, _ = _ops()
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    xf = pat.float().numpy()                                  # exact widening
    bits16 = pat.view(torch.int16).numpy()
    rng = np.random.default_rng(7)
    r = (rng.standard_normal(65536) * 2.0 ** -5).astype(F32)
    base = (rng.standard_normal(65536) * 0.1).astype(F32)
    for off in (0, 1):
        for b in (None, base):
            bt = dev(b, off) if b is not None else None
            rt = dev(r, off)
            q = ef.quantize(dev(bits16, off).view(dt), rt, 4, base=bt)
            wq, wr = eref.quantize(xf, r, 4, b)
            assert np.array_equal(host(q), wq), (off, b is None)
            same_f32(host(rt), wr, (off, b is None))
            for V in (32, 12):
                rt = dev(r, off)
                q, f = ef.quantize_i16(dev(bits16, off).view(dt), rt, 4, V, base=bt)
                wq, wf, wr = eref.quantize_i16(xf, r, 4, V, b)
                assert np.array_equal(host(q), wq) and np.array_equal(host(f), wf), (off, V)
                same_f32(host(rt), wr, (off, V))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("V", VS)
def test_replay_block_scaled(V, off):
    """Given scales (the ABI's edge values among them) and scales computed in the launch, int32 and
    int16 out; n is no multiple of V except at 256 and 512, so the last block is short."""
    ef, _ = _ops()
    for n in SIZES:
        nblk = (n + V - 1) // V
        x, r, base, _ = bucket(200 + n, n, SAT32)
        bt = dev(base, off)
        # int32, given
        kb = given_scales(n, nblk, 4, 14)
        rt = dev(r, off)
        q, _ = ef.quantize_blk(dev(x, off), rt, V, kblk=dev(kb), base=bt, out=out_like(n, torch.int32, off))
        wq, wr = eref.quantize_blk(x, r, kb, V, base)
        assert np.array_equal(host(q), wq), n
        same_f32(host(rt), wr, n)
        # int32, computed from |v| for 3 summands
        rt = dev(r, off)
        q, kg = ef.quantize_blk(dev(x, off), rt, V, degree=3, out=out_like(n, torch.int32, off))
        wk = eref.block_scales([x], [r], V, 3, 32)
        wq, wr = eref.quantize_blk(x, r, wk, V)
        assert np.array_equal(host(kg), wk), n
        assert np.array_equal(host(q), wq), n
        same_f32(host(rt), wr, n)
        # int16, given
        x, r, base, _ = bucket(300 + n, n, SAT16)
        kb = given_scales(n + 1, nblk, 2, 9)
        rt = dev(r, off)
        q, f, _ = ef.quantize_i16_blk(dev(x, off), rt, V, kblk=dev(kb), out=out_like(n, torch.int16, off))
        wq, wf, wr = eref.quantize_i16_blk(x, r, kb, V)
        assert np.array_equal(host(q), wq) and np.array_equal(host(f), wf), n
        same_f32(host(rt), wr, n)
        # int16, computed, with a base
        rt = dev(r, off)
        q, f, kg = ef.quantize_i16_blk(dev(x, off), rt, V, degree=4, base=dev(base, off),
                                       out=out_like(n, torch.int16, off))
        wk = eref.block_scales([x], [r], V, 4, 16, base)
        wq, wf, wr = eref.quantize_i16_blk(x, r, wk, V, base)
        assert np.array_equal(host(kg), wk), n
        assert np.array_equal(host(q), wq) and np.array_equal(host(f), wf), n
        same_f32(host(rt), wr, n)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("W", [1, 3])
def test_replay_block_scales(W, off):
    ef, _ = _ops()
    for V in VS:
        for n in SIZES:
            bk = [bucket(400 + 10 * n + w, n, SAT32) for w in range(W)]
            xs, rs, base = [b[0] for b in bk], [b[1] for b in bk], bk[0][2]
            rts = [dev(r, off) for r in rs]
            for bits, b in ((32, None), (16, base)):
                got = ef.block_scales([dev(x, off) for x in xs], rts, V, bits=bits, degree=W + 1,
                                      base=dev(b, off) if b is not None else None)
                assert np.array_equal(host(got), eref.block_scales(xs, rs, V, W + 1, bits, b)), (V, n, bits)
            for rt, r in zip(rts, rs):                                   # nothing but the scales is written
                same_f32(host(rt), r, (V, n))


def test_nonfinite_leaves_zero_residual_and_a_finite_clip_is_carried():
    """The two rules by name: a NaN or +-inf v leaves +0 (and quantises as the sibling: 0, or saturated
    with the flag); a finite v that saturates leaves v - float(q) * 2^-k."""
    ef, ops = _ops()
    x = np.zeros(512, F32)
    r = np.full(512, 0.25, F32)
    x[[3, 40, 77]] = [np.nan, np.inf, -np.inf]
    x[[100, 300]] = [SAT32, -2 * SAT32]
    rt = dev(r)
    q = host(ef.quantize(dev(x), rt, K32))
    rn = host(rt)
    assert list(q[[3, 40, 77]]) == [0, 2**31 - 1, -2**31]
    assert np.array_equal(eref.bits(rn[[3, 40, 77]]), np.zeros(3, np.uint32))           # +0.0f, not -0 or NaN
    assert list(q[[100, 300]]) == [2**31 - 1, -2**31]
    want = (x[[100, 300]] + F32(0.25)) - np.array([2.0**31, -2.0**31], F32) * F32(2.0**-K32)
    same_f32(rn[[100, 300]], want.astype(F32), "carried clip")
    assert np.all(np.abs(rn[[100, 300]]) > 1e6)
    # int16: the slot flags of exactly those slots, and the same residual rules
    x[[100, 300]] = [SAT16, -2 * SAT16]
    rt = dev(r)
    q, f = ef.quantize_i16(dev(x), rt, K16, 32)
    q, f, rn = host(q), host(f), host(rt)
    assert sorted(np.flatnonzero(f)) == sorted({3 // 32, 40 // 32, 77 // 32, 100 // 32, 300 // 32})
    assert list(q[[3, 40, 77, 100, 300]]) == [0, 32767, -32768, 32767, -32768]
    assert np.array_equal(eref.bits(rn[[3, 40, 77]]), np.zeros(3, np.uint32))
    want = (x[[100, 300]] + F32(0.25)) - np.array([32767, -32768], F32) * F32(2.0**-K16)
    same_f32(rn[[100, 300]], want.astype(F32), "carried clip, int16")


# ---- zero residual equals today's call ------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 513, 4099])
def test_zero_residual_equals_the_sibling(n):
    ef, ops = _ops()
    x, _, base, _ = bucket(500 + n, n, SAT16)
    xt, bt = dev(x), dev(base)
    d = (xt - bt)                                                         # the fp32 subtraction
    zero = lambda: ef.new_residual(xt)                                    # noqa: E731
    r = zero()
    assert r.dtype == torch.float32 and r.shape == xt.shape and not r.any()
    assert torch.equal(ef.quantize(xt, r, K32, base=bt), ops.quantize(d, K32))
    same_f32(host(r), eref.quantize(x, np.zeros(n, F32), K32, base)[1], "residual left")
    for V in (32, 12):
        nblk = (n + V - 1) // V
        r = zero()
        q, f = ef.quantize_i16(xt, r, K16, V)
        sq, sf = ops.quantize_i16(xt, K16, V)
        assert torch.equal(q, sq) and torch.equal(f, sf)
        same_f32(host(r), eref.quantize_i16(x, np.zeros(n, F32), K16, V)[2], "residual left")
        assert torch.equal(ef.block_scales([xt, d], [zero(), zero()], V, bits=16, degree=5),
                           ops.block_scales([xt, d], V, bits=16, degree=5))
        kb = dev(given_scales(n, nblk, 2, 12))
        r = zero()
        assert torch.equal(ef.quantize_blk(xt, r, V, kblk=kb)[0], ops.quantize_blk(xt, kb, V))
        same_f32(host(r), eref.quantize_blk(x, np.zeros(n, F32), host(kb), V)[1], "residual left")
        q, f, _ = ef.quantize_i16_blk(xt, zero(), V, kblk=kb)
        sq, sf = ops.quantize_i16_blk(xt, kb, V)
        assert torch.equal(q, sq) and torch.equal(f, sf)
        # computed scales: the sibling's scales kernel, then its quantiser
        q, ka = ef.quantize_blk(d, zero(), V, degree=2)
        sk = ops.block_scales([d], V, bits=32, degree=2)
        assert torch.equal(ka, sk) and torch.equal(q, ops.quantize_blk(d, sk, V))
    for dt in (torch.bfloat16, torch.float16):
        h = xt.to(dt)
        assert torch.equal(ef.quantize(h, zero(), 4, base=bt), ops.quantize(h.float() - bt, 4))
        q, f = ef.quantize_i16(h, zero(), 4, 32)
        sq, sf = ops.quantize_i16(h, 4, 32)
        assert torch.equal(q, sq) and torch.equal(f, sf)


@pytest.mark.parametrize("V", [32, 256])
def test_zero_residual_packs_equal_the_sibling_rows(V):
    ef, ops = _ops()
    n, W = 4099, 3
    rng = np.random.default_rng(V)
    xs = [dev((rng.standard_normal(n) * 0.3).astype(F32)) for _ in range(W)]
    base = dev((rng.standard_normal(n) * 0.3).astype(F32))
    zeros = lambda: [ef.new_residual(x) for x in xs]                      # noqa: E731
    args = (V, [1, 2, 4], W, 1, 7)
    got = ef.quantize_pack_nga_multi_split(xs, zeros(), K32, *args, base=base, descs=True)
    want = ops.quantize_pack_nga_multi_split(xs, K32, *args, base=base, descs=True)
    for g, w in zip(got, want):
        assert all(torch.equal(a, b) for a, b in zip(g, w))
    npk = (n + V - 1) // V
    kb = dev(given_scales(V, npk, 4, 14))
    for k, kw in ((kb, dict(kblk=kb)), (None, dict(degree=5))):
        ef_kw = {} if k is not None else kw
        got = ef.quantize_pack_nga_multi_split(xs, zeros(), k, *args, base=base, descs=True, **ef_kw)
        want = ops.quantize_pack_nga_multi_split_blk(xs, *args, base=base, descs=True, **kw)
        for g, w in zip(got[:3], want[:3]):
            assert all(torch.equal(a, b) for a, b in zip(g, w))
        assert torch.equal(got[3], want[3])


# ---- pack parity ----------------------------------------------------------------------------------
def _pack_case(seed, W, n):
    rng = np.random.default_rng(seed)
    xs = [(rng.standard_normal(n) * 0.3).astype(F32) for _ in range(W)]
    for w, x in enumerate(xs):
        x[(17 * w + np.arange(9) * 31) % n] = SPECIALS(SAT32)
    rs = [(rng.standard_normal(n) * 2.0 ** -(K32 + 1)).astype(F32) for _ in range(W)]
    base = (rng.standard_normal(n) * 0.3).astype(F32)
    return xs, rs, base


def _rows_of(ops, q, V, w, W, desc=True):
    return ops.pack_nga_split(q, V, w + 1, W, 1, 7, desc=desc)


@pytest.mark.parametrize("V", [32, 256, 12])
@pytest.mark.parametrize("W", [1, 3, 8, 9])
def test_pack_parity(W, V):
    """The EF pack's rows are ops.pack_nga_split of each worker's ef.quantize result and the residuals
    are that call's, for a global k, given scales and scales computed from |v| (equal to
    ef.block_scales).  V = 12 and W = 9 compute their scales in a launch of their own first."""
    ef, ops = _ops()
    n = 4099
    xs, rs, base = _pack_case(1000 * W + V, W, n)
    xt, bt = [dev(x) for x in xs], dev(base)
    npk = (n + V - 1) // V
    bitmaps = list(range(1, W + 1))
    for mode in ("global", "given", "auto"):
        rt = [dev(r) for r in rs]
        if mode == "global":
            hdrs, pays, ds = ef.quantize_pack_nga_multi_split(xt, rt, K32, V, bitmaps, W, 1, 7, base=bt, descs=True)
        else:
            ra = [dev(r) for r in rs]
            want_k = ef.block_scales(xt, ra, V, bits=32, degree=W + 2, base=bt)
            k = dev(given_scales(W + V, npk, 4, 14)) if mode == "given" else None
            hdrs, pays, ds, kb = ef.quantize_pack_nga_multi_split(xt, rt, k, V, bitmaps, W, 1, 7, base=bt,
                                                                  degree=W + 2, descs=True)
            if mode == "auto":
                assert torch.equal(kb, want_k)
                assert np.array_equal(host(kb), eref.block_scales(xs, rs, V, W + 2, 32, base))
        for w in range(W):
            r1 = dev(rs[w])
            if mode == "global":
                q = ef.quantize(xt[w], r1, K32, base=bt)
            else:
                q, _ = ef.quantize_blk(xt[w], r1, V, kblk=kb, base=bt)
            h, p, d = _rows_of(ops, q, V, w, W)
            assert torch.equal(hdrs[w], h) and torch.equal(pays[w], p) and torch.equal(ds[w], d), (mode, w)
            same_f32(host(rt[w]), host(r1), (mode, w))


# ---- grid-stride ----------------------------------------------------------------------------------
def test_grid_stride_under_a_capped_grid():
    """tuning key 0 caps every EF launch at 2 workgroups: the grid-stride loops run many passes and
    give the uncapped results."""
    ef, ops = _ops()
    n, V, W = 3 * 1024 * 4 + 5, 32, 2
    xs, rs, base = _pack_case(9, W, n)
    xt, bt = [dev(x) for x in xs], dev(base)
    kb = dev(given_scales(9, (n + V - 1) // V, 4, 14))

    def run():
        out = []
        fresh = lambda: [dev(r) for r in rs]                              # noqa: E731
        for call in (lambda r: ef.quantize(xt[0], r[0], K32, base=bt),
                     lambda r: ef.quantize_i16(xt[0], r[0], K16, V),
                     lambda r: ef.quantize_i16(xt[0].bfloat16(), r[0], K16, V),
                     lambda r: ef.quantize(xt[0][1:], r[0][1:], K32),                    # scalar path
                     lambda r: ef.block_scales(xt, r, V, base=bt),
                     lambda r: ef.block_scales([x[1:] for x in xt], [q[1:] for q in r], 12),
                     lambda r: ef.quantize_blk(xt[0], r[0], V, kblk=kb),
                     lambda r: ef.quantize_blk(xt[0], r[0], V),
                     lambda r: ef.quantize_i16_blk(xt[0], r[0], V, kblk=kb),
                     lambda r: ef.quantize_i16_blk(xt[0], r[0], V),
                     lambda r: ef.quantize_i16_blk(xt[0], r[0], 12),                     # scalar path
                     lambda r: ef.quantize_pack_nga_multi_split(xt, r, K32, V, [1, 2], W, 1, 7, base=bt),
                     lambda r: ef.quantize_pack_nga_multi_split(xt, r, None, V, [1, 2], W, 1, 7, base=bt),
                     lambda r: ef.quantize_pack_nga_multi_split(xt, r, kb, V, [1, 2], W, 1, 7)):
            r = fresh()
            res = call(r)
            flat = []
            for t in (res if isinstance(res, tuple) else (res,)):
                flat += list(t) if isinstance(t, (list, tuple)) else [t]
            out.append([host(t).copy() for t in flat] + [eref.bits(host(t)).copy() for t in r])
        return out

    want = run()
    try:
        ops.set_tuning(max_blocks=2)
        got = run()
    finally:
        ops.set_tuning(max_blocks=16384)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), i


# ---- conservation, exact --------------------------------------------------------------------------
def _conservation_inputs(seed, T, n, k):
    """x_t = m * 2^-(k+8), integer m: |m| < 128 on the first half (each step alone rounds to zero),
    |m| < 2^15 on the second.  Every fp32 operation of the step is exact on these."""
    rng = np.random.default_rng(seed)
    m = np.concatenate([rng.integers(-127, 128, (T, n // 2)), rng.integers(-(2**15) + 1, 2**15, (T, n - n // 2))], axis=1)
    return (m * 2.0 ** -(k + 8)).astype(F32)


def test_conservation_is_exact():
    ef, ops = _ops()
    k, T, n = 10, 8, 4096
    xs = _conservation_inputs(0, T, n, k)
    assert np.array_equal(xs.astype(np.float64) * 2.0 ** (k + 8), np.rint(xs.astype(np.float64) * 2.0 ** (k + 8)))
    r = ef.new_residual(dev(xs[0]))
    sent = np.zeros(n, np.float64)
    for t in range(T):
        xt = dev(xs[t])
        q = host(ef.quantize(xt, r, k))
        sent += q.astype(np.float64) * 2.0 ** -k
        assert np.all(np.abs(host(r).astype(np.float64)) <= 2.0 ** -(k + 1)), t
        assert not host(ops.quantize(xt, k))[: n // 2].any(), t            # the plain quantiser: nothing, every step
    meant = xs.astype(np.float64).sum(axis=0)
    assert np.all(sent + host(r).astype(np.float64) == meant)
    assert np.any(meant[: n // 2] != 0) and np.any(sent[: n // 2] != 0)


def test_conservation_is_exact_through_four_workers_on_the_int16_wire():
    ef, ops = _ops()
    k, T, n, W, V = 10, 8, 4096, 4, 32
    xs = [_conservation_inputs(1 + w, T, n, k) for w in range(W)]
    rs = [ef.new_residual(dev(xs[0][0])) for _ in range(W)]
    sent = np.zeros(n, np.float64)
    for t in range(T):
        qs = []
        for w in range(W):
            q, f = ef.quantize_i16(dev(xs[w][t]), rs[w], k, V)
            assert not host(f).any()
            qs.append(q)
        s, f = ops.sum_reduce_i16(qs, V)
        assert not host(f).any(), t
        sent += host(ops.dequantize(s, k)).astype(np.float64)
    meant = sum(x.astype(np.float64).sum(axis=0) for x in xs)
    left = sum(host(r).astype(np.float64) for r in rs)
    assert np.all(sent + left == meant)


# ---- loopback -------------------------------------------------------------------------------------
LOOP_K, LOOP_V, LOOP_W, LOOP_EPOCHS = 8, 32, 2, 3


def make_small():
    return torch.nn.Linear(100, 1000)


def noise(idx, epoch, n):
    g = torch.Generator().manual_seed(1000 * idx + epoch)
    return (torch.randn(n, generator=g) * 1e-2).numpy().astype(F32)


def train_step(model, idx, epoch):
    with torch.no_grad():
        v = torch.nn.utils.parameters_to_vector(model.parameters())
        v += torch.from_numpy(noise(idx, epoch, v.numel())).to(v.device)
        torch.nn.utils.vector_to_parameters(v, model.parameters())


def _worker(idx, W, port, path):
    for p in (REPO, PKG_ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    from ina_amd.loopback import worker_serve
    worker_serve(idx, W, port, path, make_small, train_step, error_feedback=True)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", [LOOP_K, "block"])
def test_loopback_two_workers_with_error_feedback(k):
    """test_loopback_two_workers_bit_exact's flow with error_feedback=True: the PS's parameters after
    every epoch are the replay's -- each worker's residual carried from epoch to epoch, the scales of
    k = "block" taken over update + residual and agreed by MIN."""
    from ina_amd.loopback import ps_serve
    W, V = LOOP_W, LOOP_V
    torch.manual_seed(0)
    model = make_small().cuda()
    local = torch.nn.utils.parameters_to_vector(model.parameters()).detach().cpu().numpy()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    seen, out, listening = [], {}, threading.Event()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "switch.sock")
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_worker, args=(i, W, port, path)) for i in range(W)]
        th = threading.Thread(target=lambda: out.setdefault(
            "r", ps_serve(model, W, LOOP_EPOCHS, port, path, k=k, V=V, on_listen=listening.set,
                          on_epoch=lambda e, v, ta, tt: seen.append(v.cpu().numpy().copy()))))
        th.start()
        assert listening.wait(60)
        for p in procs:
            p.start()
        th.join(timeout=240)
        for p in procs:
            p.join(timeout=60)
        assert not th.is_alive()
        assert all(p.exitcode == 0 for p in procs)
    assert len(seen) == LOOP_EPOCHS
    n = local.size
    rs = [np.zeros(n, F32) for _ in range(W)]
    ws = F32(1.0 / (W + 1))
    for e in range(LOOP_EPOCHS):
        paras = [(local + noise(i, e, n)).astype(F32) for i in range(W)]
        if k == "block":
            kb = np.minimum.reduce([eref.block_scales([paras[i]], [rs[i]], V, W, 32, local) for i in range(W)])
            step = [eref.quantize_blk(paras[i], rs[i], kb, V, local) for i in range(W)]
            total = orc.sum_reduce_i32([q for q, _ in step])
            y = bref.dequantize(total, kb, V)
        else:
            step = [eref.quantize(paras[i], rs[i], k, local) for i in range(W)]
            total = orc.sum_reduce_i32([q for q, _ in step])
            y = orc.dequantize_i32(total, k)
        rs = [r for _, r in step]
        local = (local + y * ws).astype(F32)
        assert np.array_equal(seen[e].view(np.uint32), local.view(np.uint32)), e
    assert any(r.any() for r in rs)
