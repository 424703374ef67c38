"""Error feedback on the sharded int16 wire on the device (include/ina_shard_ef.h, ina_amd.ef) and
ShardedAggregator(error_feedback=True) on one rank.

Replay: the word is the CPU oracle's quantize_i16_wire on v = x + r (per block through
tests/_shard_blk_ref.wire_ref), and r' is tests/_ef_ref.carry with the q16 decoded from the word's low
22 bits, both bit for bit.  Zero residual: the word is the non-EF sibling's on x.  Conservation: on
inputs where every fp32 operation is exact, what the aggregator returned plus the residual it holds
is, in float64 and with ==, what was meant to be sent."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _blk_ref as bref
from tests import _ef_ref as eref
from tests import _shard_blk_ref as sref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
SIZES = (1, 5, 255, 256, 257, 4099)
VS = (8, 32, 256, 12)                 # 12: no vector layout, the value-by-value path
K = 9                                 # what ina_scale_for leaves a rank of a 64-rank int16 job
SAT = 32767.0 / 2 ** K                # |v| past this clips


def dev(a, off=0):
    """a on the device; off = 1: as a view one element into its allocation (the unaligned path)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.to(DEV)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    buf[off:].copy_(t)
    return buf[off:]


def out_like(n, off):
    return torch.empty(n + off, dtype=torch.int32, device=DEV)[off:]


def host(t):
    return t.cpu().numpy()


def same_f32(got, want, what):
    assert np.array_equal(eref.bits(got), eref.bits(want)), what


def q16_of(word):
    """One rank's q16 back out of its wire words: the low 22 bits, sign-extended."""
    w = np.asarray(word, np.int64) & 0x3FFFFF
    return np.where(w >= 1 << 21, w - (1 << 22), w).astype(np.int32)


def sat_of(word):
    """One rank's saturation bit: what is left above its q16 (1 where v clipped, was +-inf or NaN)."""
    return (np.asarray(word, np.int64) + (1 << 21)) >> 22


def carry_blk(v, q16, kb, V):
    return np.concatenate([eref.carry(v[sl], q16[sl], bref.keff(kb[s])) for s, sl in enumerate(bref.blocks(v.size, V))])


def global_case(n, seed=0):
    """(x, r): some |x + r| past the int16 range at K, a seeded non-zero residual with two -0.0, and
    one NaN and one +inf planted where the bucket has room."""
    rng = np.random.default_rng(1000 * seed + n)
    x = (rng.standard_normal(n) * 0.4 * SAT).astype(F32)
    r = (rng.standard_normal(n) * 2.0 ** -(K + 1)).astype(F32)
    r[rng.choice(n, size=min(n, 2), replace=False)] = F32(-0.0)
    if n >= 8:
        x[1], x[n - 2] = np.nan, np.inf
    return x, r


def blk_case(n, V, seed=0):
    """(x, r, kblk): tests/_blk_ref.bucket data (neighbouring blocks carry different k), a residual
    of a few per cent of each value, the NaN and +inf as above, and _shard_blk_ref.given_scales-style
    scales of v -- 3 added on every third block, so that elements there clip."""
    rng = np.random.default_rng(2000 * seed + 13 * V + n)
    x = bref.bucket(rng, 1, n, V)[0]
    r = (x * rng.standard_normal(n).astype(F32) * F32(2.0 ** -5)).astype(F32)
    r[rng.choice(n, size=min(n, 2), replace=False)] = F32(-0.0)
    if n >= 8:
        x[1], x[n - 2] = np.nan, np.inf
    return x, r, sref.given_scales(eref.v_of(x, r)[None, :], V)


# ---- replay parity --------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
def test_replay_global(off):
    from ina_amd import ef
    clipped = 0
    for n in SIZES:
        x, r = global_case(n)
        rt = dev(r, off)
        word = host(ef.quantize_i16_wire(dev(x, off), rt, K, out=out_like(n, off)))
        v = eref.v_of(x, r)
        want = orc.quantize_i16_wire(v, K)
        assert word.dtype == np.int32 and np.array_equal(word, want), n
        same_f32(host(rt), eref.carry(v, q16_of(want), K), n)
        clipped += int(np.count_nonzero(sat_of(want)))
    assert clipped > 10                                               # NaN, inf and finite clips among them


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("V", VS)
def test_replay_block_scaled(V, off):
    from ina_amd import ef
    clipped = 0
    for n in SIZES:
        x, r, kb = blk_case(n, V)
        rt = dev(r, off)
        word = host(ef.quantize_i16_wire_blk(dev(x, off), rt, dev(kb), V, out=out_like(n, off)))
        v = eref.v_of(x, r)
        want = sref.wire_ref(v, kb, V)
        assert word.dtype == np.int32 and np.array_equal(word, want), (V, n)
        same_f32(host(rt), carry_blk(v, q16_of(want), kb, V), (V, n))
        clipped += int(np.count_nonzero(sat_of(want)))
    assert clipped > 10


def test_a_given_minus_128_is_read_as_minus_126_and_k_127_carries_the_subnormal():
    from ina_amd import ef
    V, n = 32, 5 * 32 + 3
    rng = np.random.default_rng(128)
    x = (rng.standard_normal(n) * 1e38).astype(F32)                    # a few units at 2^-126
    r = (rng.standard_normal(n) * 1e37).astype(F32)
    v = eref.v_of(x, r)
    for low in (-128, -127, -126):
        kb = np.full(6, low, np.int8)
        rt = dev(r)
        word = host(ef.quantize_i16_wire_blk(dev(x), rt, dev(kb), V))
        want = orc.quantize_i16_wire(v, -126)
        assert np.abs(q16_of(want)).max() > 0 and np.array_equal(word, want), low
        same_f32(host(rt), eref.carry(v, q16_of(want), -126), low)
    tiny = (rng.standard_normal(n) * 2.0 ** -120).astype(F32)          # k = 127: 2^-k is the subnormal 2^-127
    rt = dev(tiny * F32(0.25))
    v = eref.v_of(tiny, tiny * F32(0.25))
    word = host(ef.quantize_i16_wire(dev(tiny), rt, 127))
    want = orc.quantize_i16_wire(v, 127)
    assert np.abs(q16_of(want)).max() > 0 and np.array_equal(word, want)
    same_f32(host(rt), eref.carry(v, q16_of(want), 127), "k = 127")


# ---- the same step as the int16 EF call -----------------------------------------------------------
@pytest.mark.parametrize("n", [5, 257, 4099])
def test_agrees_with_the_int16_ef_call(n):
    """ef.quantize_i16 / ef.quantize_i16_blk on the same inputs: their q is the word's low part, their
    r' this call's, and their slot flag is set exactly where a word of the slot has its sat bit."""
    from ina_amd import ef
    V = 32
    x, r = global_case(n, seed=3)
    ra, rb = dev(r), dev(r)
    word = host(ef.quantize_i16_wire(dev(x), ra, K))
    q, f = ef.quantize_i16(dev(x), rb, K, V)
    assert np.array_equal(q16_of(word), host(q).astype(np.int32))
    same_f32(host(ra), host(rb), "global r'")
    assert np.array_equal(host(f), np.array([sat_of(word[sl]).any() for sl in bref.blocks(n, V)], np.uint8))
    x, r, kb = blk_case(n, V, seed=3)
    ra, rb = dev(r), dev(r)
    word = host(ef.quantize_i16_wire_blk(dev(x), ra, dev(kb), V))
    q, f, _ = ef.quantize_i16_blk(dev(x), rb, V, kblk=dev(kb))
    assert np.array_equal(q16_of(word), host(q).astype(np.int32))
    same_f32(host(ra), host(rb), "block r'")
    assert np.array_equal(host(f), np.array([sat_of(word[sl]).any() for sl in bref.blocks(n, V)], np.uint8))


# ---- zero residual equals today's call ------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [5, 257, 4099])
def test_zero_residual_equals_the_sibling(n, off):
    from ina_amd import ef, ops
    x, _ = global_case(n, seed=5)
    xt = dev(x, off)
    r = torch.zeros(n + off, dtype=torch.float32, device=DEV)[off:]
    assert torch.equal(ef.quantize_i16_wire(xt, r, K), ops.quantize_i16_wire(xt, K))
    v = eref.v_of(x, np.zeros(n, F32))                                  # x up to the sign of zero
    same_f32(host(r), eref.carry(v, q16_of(orc.quantize_i16_wire(v, K)), K), "residual left")
    for V in (32, 12):
        x, _, kb = blk_case(n, V, seed=5)
        xt, kbt = dev(x, off), dev(kb)
        r = torch.zeros(n + off, dtype=torch.float32, device=DEV)[off:]
        assert torch.equal(ef.quantize_i16_wire_blk(xt, r, kbt, V), ops.quantize_i16_wire_blk(xt, kbt, V))
        v = eref.v_of(x, np.zeros(n, F32))
        same_f32(host(r), carry_blk(v, q16_of(sref.wire_ref(v, kb, V)), kb, V), "residual left")


def test_residual_right_beside_x_and_the_bytes_around_the_outputs():
    """x, resid and the words adjacent in one allocation (no byte shared: not an overlap); the words
    and r' land inside their own ranges."""
    from ina_amd import ef
    n, G = 1028, 64
    x, r = global_case(n, seed=7)
    buf = torch.full((3 * n + 2 * G,), float("nan"), dtype=torch.float32, device=DEV)
    xt, rt, wt = buf[G:G + n], buf[G + n:G + 2 * n], buf[G + 2 * n:G + 3 * n].view(torch.int32)
    xt.copy_(dev(x))
    rt.copy_(dev(r))
    ef.quantize_i16_wire(xt, rt, K, out=wt)
    v = eref.v_of(x, r)
    want = orc.quantize_i16_wire(v, K)
    assert np.array_equal(host(wt), want)
    same_f32(host(rt), eref.carry(v, q16_of(want), K), "r'")
    same_f32(host(xt), x, "x is only read")
    assert np.isnan(host(buf[:G])).all() and np.isnan(host(buf[-G:])).all()


# ---- the two rules by name ------------------------------------------------------------------------
def test_nonfinite_leaves_zero_residual_and_a_finite_clip_is_carried():
    from ina_amd import ef
    n, V = 512, 32
    x = np.zeros(n, F32)
    r = np.full(n, 0.25, F32)
    x[[3, 40, 77]] = [np.nan, np.inf, -np.inf]
    x[[100, 300]] = [3 * SAT, -5 * SAT]
    kb = np.full(n // V, K, np.int8)
    for call in (lambda xt, rt: ef.quantize_i16_wire(xt, rt, K),
                 lambda xt, rt: ef.quantize_i16_wire_blk(xt, rt, dev(kb), V)):
        rt = dev(r)
        word = host(call(dev(x), rt))
        rn = host(rt)
        sat = 1 << 22
        assert list(word[[3, 40, 77]]) == [sat, sat + 32767, sat - 32768]       # the sat bit, NaN -> 0
        assert np.array_equal(eref.bits(rn[[3, 40, 77]]), np.zeros(3, np.uint32))   # +0.0f, not -0 or NaN
        assert list(word[[100, 300]]) == [sat + 32767, sat - 32768]
        want = (x[[100, 300]] + F32(0.25)) - np.array([32767, -32768], F32) * F32(2.0 ** -K)
        same_f32(rn[[100, 300]], want.astype(F32), "carried clip")
        assert np.all(np.abs(rn[[100, 300]]) > SAT)
        rest = np.setdiff1d(np.arange(n), [3, 40, 77, 100, 300])
        assert np.all(word[rest] == 128) and not rn[rest].any()               # 0.25 * 2^9, nothing dropped


# ---- grid-stride ----------------------------------------------------------------------------------
def test_grid_stride_under_a_capped_grid():
    """Tuning key 0 caps both launches, and the value-by-value path, at 2 workgroups: the grid-stride
    loops run many passes and give the uncapped results, every output byte and residual bit."""
    from ina_amd import ef, ops
    n, V = 3 * 1024 * 4 + 5, 32
    x, r, kb = blk_case(n, V, seed=9)
    xg, rg = global_case(n, seed=9)
    kbt, kb12 = dev(kb), dev(sref.given_scales(eref.v_of(x, r)[None, :], 12))

    def run():
        out = []
        for call in (lambda xt, rt: ef.quantize_i16_wire(xt, rt, K),
                     lambda xt, rt: ef.quantize_i16_wire_blk(xt, rt, kbt, V),
                     lambda xt, rt: ef.quantize_i16_wire(xt[1:], rt[1:], K),               # one element in
                     lambda xt, rt: ef.quantize_i16_wire_blk(xt[1:], rt[1:], kbt, V),
                     lambda xt, rt: ef.quantize_i16_wire_blk(xt, rt, kb12, 12)):                # no vector layout
            for xs, rs in ((xg, rg), (x, r)):
                rt = dev(rs)
                out.append((host(call(dev(xs), rt)).copy(), eref.bits(host(rt)).copy()))
        return out

    want = run()
    try:
        ops.set_tuning(max_blocks=2)
        got = run()
    finally:
        ops.set_tuning(max_blocks=16384)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0].view(np.uint8), w[0].view(np.uint8)), i
        assert np.array_equal(g[1], w[1]), i
    # and the uncapped run is the replay (the larger n of this file)
    v = eref.v_of(x, r)
    assert np.array_equal(want[3][0], sref.wire_ref(v, kb, V))
    same_f32(want[3][1].view(F32), carry_blk(v, q16_of(want[3][0]), kb, V), "block r' at n = 12293")


# ---- the aggregator on one rank -------------------------------------------------------------------
def _conservation_inputs(seed, T, n, k):
    """x_t = m * 2^-(k+8), integer m: |m| < 128 on the first half (each step alone rounds to zero),
    |m| < 2^15 on the second.  Every fp32 operation of the step is exact on these."""
    rng = np.random.default_rng(seed)
    m = np.concatenate([rng.integers(-127, 128, (T, n // 2)), rng.integers(-(2**15) + 1, 2**15, (T, n - n // 2))], axis=1)
    return (m * 2.0 ** -(k + 8)).astype(F32)


@pytest.mark.parametrize("wire", ["i16", "i32"])
def test_world_1_aggregator_conserves_exactly(wire):
    from ina_amd.dist import ShardedAggregator
    k, T, n, V = 10, 8, 4096, 32
    xs = _conservation_inputs(40, T, n, k)
    grid = xs.astype(np.float64) * 2.0 ** (k + 8)
    assert np.array_equal(grid, np.rint(grid))                                # on the 2^-(k+8) grid
    make = lambda **kw: ShardedAggregator(n=n, k=k, wire=wire, V=V, device=torch.device(DEV), **kw)   # noqa: E731
    agg, plain = make(error_feedback=True), make()
    assert plain.residual is None
    res = agg.residual
    assert res.dtype == torch.float32 and res.shape == (n,) and res.is_cuda and not res.any()
    sent = np.zeros(n, np.float64)
    first = None
    for t in range(T):
        full = host(agg(dev(xs[t])))
        assert full.shape == (n,) and agg.residual is res                     # updated in place
        if first is None:
            first = (full.copy(), eref.bits(host(res)).copy())
        sent += full.astype(np.float64)
        assert np.all(np.abs(host(res).astype(np.float64)) <= 2.0 ** -(k + 1)), t
        assert not host(plain(dev(xs[t])))[: n // 2].any(), t                 # without: nothing, every step
        if wire == "i16":
            assert not host(agg.overflow).any(), t
    meant = xs.astype(np.float64).sum(axis=0)
    assert np.all(sent + host(res).astype(np.float64) == meant)
    assert np.any(meant[: n // 2] != 0) and np.any(sent[: n // 2] != 0)
    # reset_residual(), then one step: a fresh aggregator's first step
    agg.reset_residual()
    assert agg.residual is res and not res.any()
    again = host(agg(dev(xs[0])))
    assert np.array_equal(eref.bits(again), eref.bits(first[0])) and np.array_equal(eref.bits(host(res)), first[1])
    # aggregate_int is a step too: it advances the residual
    before = eref.bits(host(res)).copy()
    agg.aggregate_int(dev(xs[1]))
    assert not np.array_equal(eref.bits(host(res)), before)


@pytest.mark.parametrize("wire", ["i16", "i32"])
def test_world_1_aggregator_block_scales_replay(wire):
    """T = 3 steps on _blk_ref.bucket data; after each step full, kblk, overflow and residual are the
    numpy replay's: _ef_ref.block_scales of v, the wire (wire_ref / the per-block quantiser), the
    finish, ref.dequantize, and the carry of this rank's own q."""
    from ina_amd.dist import ShardedAggregator
    n, V, T = 5000, 32, 3
    bits = 16 if wire == "i16" else 32
    agg = ShardedAggregator(n=n, k="block", wire=wire, V=V, device=torch.device(DEV), error_feedback=True)
    r = np.zeros(n, F32)
    rng = np.random.default_rng(77)
    for t in range(T):
        x = bref.bucket(rng, 1, n, V)[0]
        if t == 1:
            x[7], x[n - 3] = np.nan, -np.inf
        full = agg(dev(x))
        v = eref.v_of(x, r)
        kb = eref.block_scales([x], [r], V, 1, bits)
        if wire == "i16":
            word = sref.wire_ref(v, kb, V)
            o16, _, flags = sref.finish_ref(word, kb, V)
            want, q = bref.dequantize(o16, kb, V), q16_of(word)
            sref.same(agg.overflow, flags, f"overflow, step {t}")
            assert flags.sum() == (2 if t == 1 else 0)
        else:
            q = bref.quantize_i32(v, kb, V)
            want = bref.dequantize(q, kb, V)
        r = carry_blk(v, q, kb, V)
        sref.same(full, want, f"full, step {t}")
        sref.same(agg.kblk, kb, f"kblk, step {t}")
        same_f32(host(agg.residual), r, f"residual, step {t}")
        assert r.any()
