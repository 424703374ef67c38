"""Stochastic rounding on the packet path (include/ina_pkt_sr.h) on the GPU against the numpy replay of
tests/_sr_pkt_ref.py, bit for bit.  The yardstick is never the code under test: payload words are the
replay's (Philox, the rounding step, the oracle's clamp), rows the oracle's NGA pack of them.  Every
output row array sits between guard bytes that must come back untouched."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _sr_pkt_ref as P
from tests import _sr_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT, GUARD = 0xA5, 64
SEED, STEP, SUB = 0x9E3779B97F4A7C15, 7, 0xFFFFFFFE        # sub + w wraps at w = 2
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
VS = [8, 12, 32, 256]                                       # 12: no power of two; 256: a wave per packet
KW = dict(seed=SEED, step=STEP, sub=SUB)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ina_amd import sr  # noqa: F401


def mods():
    from ina_amd import ops, sr
    return ops, sr


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ns_of(V):
    return sorted({1, 5, V - 1, V, 3 * V + 1, 4099})


def bucket(seed, n, dt, W=1, special=True):
    """W buckets of dtype dt and an fp32 base: values around 2^-9 quanta with fractions of every size, and
    NaN / +-inf / subnormals where special.  Returns (device tensors, their exact fp32 values, base)."""
    rng = np.random.default_rng(seed)
    xs, vals = [], []
    for _ in range(W):
        x = (rng.standard_normal(n) * np.float32(10.0) ** rng.integers(-4, 1, n)).astype(np.float32)
        if special and n >= 5:
            for i, v in zip(rng.choice(n, 5, replace=False), (np.nan, np.inf, -np.inf, 1e-40, -3e-39)):
                x[i] = v
        t = torch.from_numpy(x).to(DTYPES[dt]).to(DEV)
        xs.append(t)
        vals.append(t.float().cpu().numpy())
    base = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    return xs, vals, base


class Guarded:
    """A uint8 [rows, width] view with GUARD sentinel bytes before and after it."""

    def __init__(self, rows, width):
        self.flat = torch.full((2 * GUARD + rows * width,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.flat[GUARD:GUARD + rows * width].view(rows, width)

    def check(self):
        f = host(self.flat)
        assert (f[:GUARD] == SENT).all() and (f[-GUARD:] == SENT).all()
        return f[GUARD:-GUARD].reshape(self.t.shape)


class GuardedDesc:
    def __init__(self, npk):
        self.flat = torch.full((npk + 16,), -1, dtype=torch.int64, device=DEV)
        self.t = self.flat[8:8 + npk]

    def check(self):
        f = host(self.flat)
        assert (f[:8] == -1).all() and (f[-8:] == -1).all()
        return f[8:-8]


def packed(x, val, k, V, n, base, e0=0, seq0=5, stride=None, desc=True, sub=SUB):
    """One single-worker SR pack into guarded rows, checked against the replay's rows."""
    _, sr = mods()
    stride = stride or (15 + 4 * V + 15) // 16 * 16
    npk = (n + V - 1) // V
    out, d = Guarded(npk, stride), GuardedDesc(npk) if desc else None
    kk = dev(k) if isinstance(k, np.ndarray) else k
    sr.quantize_pack_nga(x, kk, V, 3, 2, 1, seq0, SEED, step=STEP, sub=sub, e0=e0,
                         base=None if base is None else dev(base), stride=stride, out=out.t,
                         desc=d.t if desc else None)
    want = P.rows(P.quantize(val, k, V, SEED, STEP, sub, e0, base), V, 3, 2, seq0, stride=stride)
    assert np.array_equal(out.check(), want), (V, n, k if np.ndim(k) == 0 else "blk", stride, e0)
    if desc:
        assert np.array_equal(d.check(), P.desc_of(want))


def split(xs, vals, k, V, n, base, e0=0, seq0=9, desc=True, sub=SUB, degree=None, want_k=None):
    """One multi-worker SR split pack into guarded rows, checked worker by worker.  k None: AUTO, the
    scales written must be want_k."""
    _, sr = mods()
    W, npk = len(xs), (n + V - 1) // V
    hs, ps = [Guarded(npk, 16) for _ in xs], [Guarded(npk, 4 * V) for _ in xs]
    ds = [GuardedDesc(npk) for _ in xs] if desc else None
    kk = dev(k) if isinstance(k, np.ndarray) else k
    kout = torch.full((npk + 16,), 77, dtype=torch.int8, device=DEV)
    res = sr.quantize_pack_nga_multi_split(xs, kk, V, [1 << (w % 32) for w in range(W)], W, 1, seq0, SEED, step=STEP,
                                           sub=sub, e0=e0, base=None if base is None else dev(base), degree=degree,
                                           kblk_out=kout[:npk] if k is None else None, hdrs=[h.t for h in hs],
                                           pays=[p.t for p in ps], descs=[d.t for d in ds] if desc else None)
    if k is None:
        got_k = host(kout)
        assert np.array_equal(got_k[:npk], want_k) and (got_k[npk:] == 77).all() and res[-1].data_ptr() == kout.data_ptr()
        k = want_k
    qs = P.workers(vals, k, V, SEED, STEP, sub, e0, base)
    for w in range(W):
        want = P.rows(qs[w], V, 1 << (w % 32), W, seq0)
        wh, wp = P.split_of(want, V)
        assert np.array_equal(hs[w].check(), wh), (V, n, w)
        assert np.array_equal(ps[w].check(), wp), (V, n, w)
        if desc:
            assert np.array_equal(ds[w].check(), P.desc_of(want))
    return [h.check() for h in hs], [p.check() for p in ps]


# ---- composition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_packed_rows_are_the_plain_pack_of_the_sr_quantiser(dt, V):
    """The flat kernel, the wave-per-packet kernel at V = 256 and, at the tight stride 15 + 4V, the byte path."""
    for i, n in enumerate(ns_of(V)):
        (x,), (val,), base = bucket(100 * V + i, n, dt)
        for b in (None, base):
            for k in (9, 40):                              # 40: values past 2^-9 clip at the int32 limits
                packed(x, val, k, V, n, b, desc=(k == 9))
        packed(x, val, 9, V, n, base, stride=15 + 4 * V, desc=True)
        packed(x, val, 9, V, n, None, stride=15 + 4 * V + 3, desc=False)
        packed(x, val, 9, V, n, base, e0=4 * 12345678901, seq0=0xFFFFFFF0)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_split_rows_are_the_plain_pack_of_the_sr_quantiser(dt, V):
    for i, n in enumerate(ns_of(V)):
        xs, vals, base = bucket(200 * V + i, n, dt, W=2)
        for b in (None, base):
            for k in (9, 40):
                split(xs, vals, k, V, n, b, desc=(k == 9))
        split(xs, vals, 9, V, n, base, e0=4 * 12345678901, seq0=0xFFFFFFF0)


def test_the_composition_on_the_device_is_the_same_bytes():
    """sr.quantize with sub + w, then the plain packs: the launches the fused pack replaces."""
    ops, sr = mods()
    V, n, W = 32, 4099, 3
    xs, vals, base = bucket(31, n, "f32", W=W)
    b = dev(base)
    hs, ps = sr.quantize_pack_nga_multi_split(xs, 9, V, [1, 2, 4], W, 1, 9, SEED, step=STEP, sub=5, base=b)
    for w in range(W):
        q = sr.quantize(xs[w], 9, SEED, step=STEP, sub=5 + w, base=b)
        h, p = ops.pack_nga_split(q, V, 1 << w, W, 1, 9)
        assert torch.equal(h, hs[w]) and torch.equal(p, ps[w])
        pk = sr.quantize_pack_nga(xs[w], 9, V, 1 << w, W, 1, 9, SEED, step=STEP, sub=5 + w, base=b)
        assert torch.equal(pk, ops.pack_nga(q, V, 1 << w, W, 1, 9))


def test_grid_stride_loops():
    """ops.set_tuning(max_blocks=2): 512 threads, so every SR launch strides -- 1025 chunks in 3 passes, 17
    NGA-256 packets at 8 waves a pass, the byte path, the block-scaled kernels GIVEN and AUTO."""
    ops, _ = mods()
    ops.set_tuning(max_blocks=2)
    try:
        n = 4099
        for dt in DTYPES:
            for V in (32, 256):
                xs, vals, base = bucket(7 * V, n, dt, W=3)
                packed(xs[0], vals[0], 9, V, n, base)
                packed(xs[0], vals[0], 9, V, n, base, stride=15 + 4 * V)
                split(xs, vals, 9, V, n, base)
        for V in (32, 256):
            xs, vals, base = bucket(9 * V, n, "f32", W=3)
            k = P.block_scales(vals, V, 3, base=base)
            packed(xs[0], vals[0], k, V, n, base)
            split(xs, vals, k, V, n, base)
            split(xs, vals, None, V, n, base, want_k=k)
    finally:
        ops.set_tuning(max_blocks=16384)


# ---- workers, integers, slices ------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3, 8, 9])
def test_one_call_for_w_workers_equals_w_single_calls(W):
    """W = 9 crosses a pack group: worker 8 is the second group's first and still draws from sub + 8."""
    _, sr = mods()
    for dt, V, n in (("f32", 32, 1030), ("bf16", 256, 700), ("f16", 12, 131)):
        xs, vals, base = bucket(W * V, n, dt, W=W)
        hs, ps = split(xs, vals, 9, V, n, base)
        b = dev(base)
        for w in range(W):
            h, p, d = sr.quantize_pack_nga_multi_split([xs[w]], 9, V, [1 << w], W, 1, 9, SEED, step=STEP,
                                                       sub=(SUB + w) & 0xFFFFFFFF, base=b, descs=True)
            assert np.array_equal(host(h[0]), hs[w]) and np.array_equal(host(p[0]), ps[w])
    xs, vals, base = bucket(5 * W, 1030, "f32", W=W)           # block scales given, and AUTO
    k = P.block_scales(vals, 32, W, base=base)
    split(xs, vals, k, 32, 1030, base)
    split(xs, vals, None, 32, 1030, base, want_k=k)


def test_integers_round_as_the_nearest_sibling_for_every_seed():
    ops, sr = mods()
    rng = np.random.default_rng(3)
    V, n, k = 32, 1030, 9
    q = rng.integers(-2 ** 20, 2 ** 20, (2, n))
    for dt in DTYPES:
        xs = [torch.from_numpy((v * 2.0 ** -k).astype(np.float32)).to(DTYPES[dt]).to(DEV) for v in q]
        if dt != "f32":                                    # 16-bit: integers that the type holds
            xs = [torch.from_numpy((v % 256 - 128).astype(np.float32) * 2.0 ** -k).to(DTYPES[dt]).to(DEV) for v in q]
        want = ops.quantize_pack_nga_multi_split(xs, k, V, [1, 2], 2, 1, 9)
        one = ops.quantize_pack_nga(xs[0], k, V, 1, 2, 1, 9)
        for seed in (0, 1, SEED):
            got = sr.quantize_pack_nga_multi_split(xs, k, V, [1, 2], 2, 1, 9, seed, step=seed & 3)
            for a, b in zip(want[0] + want[1], got[0] + got[1]):
                assert torch.equal(a, b), (dt, seed)
            assert torch.equal(one, sr.quantize_pack_nga(xs[0], k, V, 1, 2, 1, 9, seed))
    xs = [torch.from_numpy((v * 2.0 ** -k).astype(np.float32)).to(DEV) for v in q]
    kb = torch.full(((n + V - 1) // V,), k, dtype=torch.int8, device=DEV)
    want = ops.quantize_pack_nga_multi_split_blk(xs, V, [1, 2], 2, 1, 9, kblk=kb)
    got = sr.quantize_pack_nga_multi_split(xs, kb, V, [1, 2], 2, 1, 9, 5)
    assert all(torch.equal(a, b) for a, b in zip(want[0] + want[1], got[0] + got[1]))


def test_slices_at_packet_boundaries():
    _, sr = mods()
    for dt, V in (("f32", 32), ("bf16", 256), ("f32", 12)):
        n = 11 * V + 3
        xs, vals, base = bucket(V, n, dt, W=2)
        b = dev(base)
        hs, ps = sr.quantize_pack_nga_multi_split(xs, 9, V, [1, 2], 2, 1, 100, SEED, step=STEP, sub=1, base=b)
        pk = sr.quantize_pack_nga(xs[0], 9, V, 1, 2, 1, 100, SEED, step=STEP, sub=1, base=b)
        for lo, hi in ((0, 4 * V), (4 * V, 5 * V), (5 * V, n)):
            p0, p1 = lo // V, -(-hi // V)
            h2, p2 = sr.quantize_pack_nga_multi_split([x[lo:hi] for x in xs], 9, V, [1, 2], 2, 1, 100 + p0, SEED,
                                                      step=STEP, sub=1, e0=lo, base=b[lo:hi])
            for w in range(2):
                assert torch.equal(h2[w], hs[w][p0:p1]) and torch.equal(p2[w], ps[w][p0:p1]), (dt, V, lo)
            one = sr.quantize_pack_nga(xs[0][lo:hi], 9, V, 1, 2, 1, 100 + p0, SEED, step=STEP, sub=1, e0=lo, base=b[lo:hi])
            assert torch.equal(one, pk[p0:p1])


# ---- block scales -------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VS)
def test_given_scales_against_the_replay(V):
    """Neighbouring packets with very different scales, -127 / -128 among them, and a short last block."""
    for i, n in enumerate((3 * V + 1, 4099, V - 1)):
        xs, vals, base = bucket(300 * V + i, n, "f32", W=2)
        k = P.block_scales(vals, V, 2, base=base)
        for j, v in enumerate((127, -128, -127, -126)):
            if j < k.size - 1:
                k[j] = v
        for b in (None, base):
            packed(xs[0], vals[0], k, V, n, b)
            split(xs, vals, k, V, n, b)
        packed(xs[0], vals[0], k, V, n, base, stride=15 + 4 * V, e0=8 * V)


@pytest.mark.parametrize("V,W", [(8, 2), (32, 3), (256, 8), (12, 2), (32, 9)])
def test_auto_scales_are_block_scales_and_the_rows_the_given_calls(V, W):
    """V = 12 and W = 9 take the scales kernel first and then the GIVEN kernels: identical output."""
    _, sr = mods()
    for n in (3 * V + 1, 2050):
        xs, vals, base = bucket(V * W + n, n, "f32", W=W)
        for b, deg in ((base, None), (None, 64)):
            want = P.block_scales(vals, V, deg or W, base=b)
            got = sr.block_scales(xs, V, degree=deg, base=None if b is None else dev(b))
            assert np.array_equal(host(got), want)
            split(xs, vals, None, V, n, b, degree=deg, want_k=want)


def test_block_scales_at_the_boundaries_of_lim():
    """amax at, just under and just over a power-of-two boundary of lim = (2^31 - 1) / degree - 1, and of the
    16-bit lim: the device comparison equals the rule in exact rationals."""
    _, sr = mods()
    V = 8
    for bits, deg in ((32, 1), (32, 3), (32, 64), (16, 1), (16, 5)):
        lim = np.float64((2 ** (bits - 1) - 1) / deg - 1)
        edges = []
        for e in (-96, -30, 0, 1, 20, 100, 126, 127, 140):   # amax = lim * 2^-e stays a finite fp32
            a = np.float32(lim * 2.0 ** -e)
            edges += [np.nextafter(a, np.float32(0)), a, np.nextafter(a, np.float32(np.inf))]
        x = np.zeros((len(edges), V), np.float32)
        x[:, 3] = np.array(edges, np.float32) * np.where(np.arange(len(edges)) % 2, -1, 1)
        x[:, 5] = np.nan
        want = np.array([S.scale_for_sr(a, deg, bits) for a in edges], np.int8)
        got = host(sr.block_scales([dev(x.ravel())], V, bits=bits, degree=deg))
        assert np.array_equal(got, want), (bits, deg)
        assert np.array_equal(P.block_scales([x.ravel()], V, deg, bits), want)
    from ina_amd import ops
    # 32766.5 at 16 bits sits on the nearest lim (32767 - 1/2) and over this one (32767 - 1): k = 0 to nearest,
    # -1 with a whole quantum.  (At 32 bits no fp32 lies between the two lims, half a quantum apart.)
    x = dev(np.full(V, np.float32(32766.5), np.float32))
    assert S.scale_for_sr(32766.5, 1, 16) == -1
    assert int(host(ops.block_scales([x], V, bits=16))[0]) == 0 and int(host(sr.block_scales([x], V, bits=16))[0]) == -1


# ---- the streams, and the point of the feature --------------------------------------------------------
def test_streams_differ_with_seed_step_and_sub():
    _, sr = mods()
    n, V = 4096, 32
    x = dev(np.full(n, np.float32(0.5) * np.float32(2.0 ** -9), np.float32))          # a coin flip each

    def vals(**kw):
        args = dict(seed=1, step=0, sub=0)
        args.update(kw)
        ops, _ = mods()
        h, p = sr.quantize_pack_nga_multi_split([x], 9, V, [1], 1, 1, 1, **args)
        return host(ops.unpack_nga_split(h[0], p[0], V)[1]).ravel()[:n]
    ref = vals()
    assert set(np.unique(ref)) == {0, 1}
    for what, kw in (("seed", dict(seed=2)), ("step", dict(step=1)), ("sub", dict(sub=1))):
        share = float((vals(**kw) != ref).mean())
        print(f"{what}: {share:.4f} of 4,096 roundings change")
        assert 0.4 <= share <= 0.6, what
    assert np.array_equal(vals(), ref)


def test_bias_end_to_end():
    """W = 4 workers, 65,536 values 0.3f * 2^-9 each, k = 9: to nearest the sum is 0 everywhere; with
    stochastic rounding its mean is within 5 sigma = 0.018 of 1.2, and equals the replay's."""
    ops, sr = mods()
    W, n, V, k = 4, 65536, 256, 9
    xs = [dev(np.full(n, np.float32(0.3) * np.float32(2.0 ** -9), np.float32)) for _ in range(W)]

    def total(hs, ps):
        return sum(host(ops.unpack_nga_split(h, p, V)[1]).ravel()[:n].astype(np.int64) for h, p in zip(hs, ps))
    near = total(*ops.quantize_pack_nga_multi_split(xs, k, V, [1, 2, 4, 8], W, 1, 1))
    assert not near.any()
    sigma = (4 * 0.21 / 65536) ** 0.5
    for seed in (2024, 7):
        got = total(*sr.quantize_pack_nga_multi_split(xs, k, V, [1, 2, 4, 8], W, 1, 1, seed, step=0, sub=0))
        print(f"seed {seed}: mean of the sums {got.mean():.5f} ({abs(got.mean() - 1.2) / sigma:.1f} sigma)")
        assert abs(got.mean() - 1.2) <= 5 * sigma
        assert np.array_equal(got, P.bias_case(seed))
