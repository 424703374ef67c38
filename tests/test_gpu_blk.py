"""GPU parity of the per-block-scale entry points (include/ina_blk.h) against the existing CPU
oracle called once per block (tests/_blk_ref.py): the scales equal ina_scale_for bit for bit, and
every block's values, saturation and flag are the global-k sibling's on that block alone."""
import numpy as np
import pytest
import torch

from tests import _blk_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VEC_V, SCALAR_V = (8, 32, 256), (1, 12, 1000)
WS = (1, 2, 5, 8, 16)
WSTEP = 0.125 * 0.3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def same(got, want, what):
    got = host(got) if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got.view(f"u{got.itemsize}") != want.view(f"u{want.itemsize}"))      # bit for bit
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def sizes(V):
    ns = sorted({n for n in (1, V - 1, V, V + 1, 64 * V, 64 * V + 3, 96 * V - 5) if n >= 1})
    return ns + ([99_989] if V >= 8 else [])


# ---- scales ---------------------------------------------------------------------------------
def _special_amax(degree, bits):
    """amax values around everything ina_scale_for distinguishes."""
    lim = ((1 << (bits - 1)) - 1) / degree - 0.5
    vals = [0.0, np.nan, np.inf, -np.inf, 1e-40, 1e-38, 3e38, 2.0 ** -20, 1.0, 2.0 ** 10, 2.0 ** -126, 2.0 ** -149]
    for k in (-20, -3, 0, 7, 20, 60, 126):
        t = np.float32(lim / 2.0 ** k)                       # float64 quotient, rounded once
        if np.isfinite(t) and t > 0:
            vals += [t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf))]
    return [np.float32(v) for v in vals]


def _special_bucket(rng, W, V, degree, bits):
    """[W, n]: block s has amax exactly special[s] (NaN: the whole block), the last block short."""
    amax = _special_amax(degree, bits)
    n = len(amax) * V - (V // 3)
    x = np.zeros((W, len(amax) * V), np.float32)
    for s, a in enumerate(amax):
        blk = x[:, s * V:(s + 1) * V]
        if np.isnan(a):
            blk[:] = np.nan
            continue
        if np.isfinite(a):
            blk[:] = (rng.uniform(-1, 1, blk.shape) * 0.5).astype(np.float32) * a
            blk[rng.integers(W), rng.integers(V)] = np.nan       # ignored
        blk[rng.integers(W), 0] = a if s % 2 else -a             # position 0 survives the short tail
    return x[:, :n].copy()


@pytest.mark.parametrize("V", VEC_V + SCALAR_V)
def test_scales_equal_the_host_function(V):
    from ina_amd import ops
    rng = np.random.default_rng(100 + V)
    for bits in (16, 32):
        for W, degree in ((2, 16), (2, None), (5, None), (8, 8)):
            deg = degree or W
            x = _special_bucket(rng, W, V, deg, bits)
            n = x.shape[1]
            want = ref.kblk_ref(x, V, deg, bits)
            assert want.min() == -126 and want.max() == 127
            xs = [dev(r) for r in x]
            same(ops.block_scales(xs, V, bits=bits, degree=degree), want, f"block_scales V={V} bits={bits} W={W}")
            if bits == 32:
                _, kb = ops.quantize_reduce_blk(xs, V, degree=degree)
                same(kb, want, f"AUTO i32 scales V={V} W={W}")
                if degree is None:       # the PS combine: degree = W, deltas against local
                    kb = torch.full((want.size,), 5, dtype=torch.int8, device=DEV)
                    ops.ps_combine_ina_blk(torch.zeros(n, device=DEV), xs, V, WSTEP, kblk_out=kb)
                    same(kb, want, f"PS combine scales V={V} W={W}")
            else:
                _, _, kb = ops.quantize_reduce_i16_blk(xs, V, degree=degree)
                same(kb, want, f"AUTO i16 scales V={V} W={W}")
            # with a base: the fp32 subtraction decides
            base = (rng.standard_normal(n) * 1e-3).astype(np.float32)
            want_b = ref.kblk_ref(x, V, deg, bits, base=base)
            same(ops.block_scales(xs, V, bits=bits, degree=degree, base=dev(base)), want_b, f"base V={V}")
            if bits == 32 and degree is None:
                kb = torch.empty(want.size, dtype=torch.int8, device=DEV)
                ops.ps_combine_ina_blk(dev(base), xs, V, WSTEP, kblk_out=kb)
                same(kb, want_b, f"PS combine scales against local V={V} W={W}")


# ---- parity ---------------------------------------------------------------------------------
def _check_given(x, kb, V, tag):
    """All GIVEN entry points on the bucket x [W, n] with scales kb, against the per-block oracle."""
    from ina_amd import ops
    W, n = x.shape
    xs, kbd = [dev(r) for r in x], dev(kb)
    nblk = kb.size
    q = ref.quantize_i32(x[0], kb, V)
    same(ops.quantize_blk(xs[0], kbd, V), q, f"quantize_blk {tag}")
    q16, f16 = ref.quantize_i16(x[0], kb, V)
    got, flags = ops.quantize_i16_blk(xs[0], kbd, V, overflow=torch.full((nblk,), 0xFF, dtype=torch.uint8, device=DEV))
    same(got, q16, f"quantize_i16_blk {tag}")
    same(flags, f16, f"quantize_i16_blk flags {tag}")
    s32 = ref.quantize_reduce_i32(x, kb, V)
    got, kb_back = ops.quantize_reduce_blk(xs, V, kblk=kbd)
    same(got, s32, f"quantize_reduce_blk {tag}")
    same(kb_back, kb, f"given scales untouched {tag}")
    s16, f16 = ref.quantize_reduce_i16(x, kb, V)
    got, flags, _ = ops.quantize_reduce_i16_blk(xs, V, kblk=kbd,
                                                overflow=torch.full((nblk,), 0xFF, dtype=torch.uint8, device=DEV))
    same(got, s16, f"quantize_reduce_i16_blk {tag}")
    same(flags, f16, f"quantize_reduce_i16_blk flags {tag}")
    same(ops.dequantize_blk(dev(s32), kbd, V), ref.dequantize(s32, kb, V), f"dequantize_blk i32 {tag}")
    same(ops.dequantize_blk(dev(s16), kbd, V), ref.dequantize(s16, kb, V), f"dequantize_blk i16 {tag}")
    local = x[-1] * np.float32(0.5)
    same(ops.ps_apply_blk(dev(local), dev(s32), kbd, V, WSTEP), ref.ps_apply(local, s32, kb, V, WSTEP),
         f"ps_apply_blk {tag}")
    return s32, s16, f16


def _check_auto(x, V, tag):
    from ina_amd import ops
    W, n = x.shape
    xs = [dev(r) for r in x]
    kb32, kb16 = ref.kblk_ref(x, V, W, 32), ref.kblk_ref(x, V, W, 16)
    got, kb = ops.quantize_reduce_blk(xs, V)
    same(kb, kb32, f"AUTO i32 scales {tag}")
    same(got, ref.quantize_reduce_i32(x, kb32, V), f"AUTO quantize_reduce_blk {tag}")
    s16, f16 = ref.quantize_reduce_i16(x, kb16, V)
    got, flags, kb = ops.quantize_reduce_i16_blk(
        xs, V, overflow=torch.full((kb16.size,), 0xFF, dtype=torch.uint8, device=DEV))
    same(kb, kb16, f"AUTO i16 scales {tag}")
    same(got, s16, f"AUTO quantize_reduce_i16_blk {tag}")
    same(flags, f16, f"AUTO flags {tag}")
    local = (x[0] * np.float32(0.75)).astype(np.float32)
    kbl = ref.kblk_ref(x, V, W, 32, base=local)
    same(ops.ps_combine_ina_blk(dev(local), xs, V, WSTEP), ref.ps_combine_ina(local, x, kbl, V, WSTEP),
         f"ps_combine_ina_blk {tag}")


@pytest.mark.parametrize("V", VEC_V + SCALAR_V)
def test_parity_per_block_given_and_auto(V):
    rng = np.random.default_rng(V)
    for idx, n in enumerate(sizes(V)):
        for W in (WS if n == 64 * V + 3 else (WS[idx % len(WS)],)):
            x = ref.bucket(rng, W, n, V)
            tag = f"V={V} n={n} W={W}"
            kb = ref.kblk_ref(x, V, W, 16 if idx % 2 else 32)
            _check_given(x, kb, V, tag)
            _check_auto(x, V, tag)


@pytest.mark.parametrize("V", (8, 32, 256, 12))
def test_adversarial_given_scales(V):
    rng = np.random.default_rng(7 * V)
    n, W = 64 * V + 3, 4
    nblk = (n + V - 1) // V
    x = ref.bucket(rng, W, n, V, lo=-6, hi=2)
    full = rng.integers(-128, 128, nblk).astype(np.int8)
    full[:4] = (-128, -127, -126, 127)
    _check_given(x, full, V, f"full int8 range V={V}")
    alt = np.where(np.arange(nblk) % 2 == 0, 127, -126).astype(np.int8)
    _check_given(x, alt, V, f"127 / -126 alternating V={V}")
    # saturating blocks next to clean ones: every third block's scale 6 too large for int16
    kb = ref.kblk_ref(x, V, W, 16)
    hot = np.arange(nblk) % 3 == 1
    kb[hot] = np.minimum(kb[hot].astype(int) + 6, 127).astype(np.int8)
    _, _, flags = _check_given(x, kb, V, f"saturating next to clean V={V}")
    assert flags[hot].all() and not flags[~hot].any()


def test_dequantize_at_k_127_is_a_subnormal_not_zero():
    from ina_amd import ops
    for V in (32, 12):
        kb = torch.full((4,), 127, dtype=torch.int8, device=DEV)
        for dt in (torch.int32, torch.int16):
            y = ops.dequantize_blk(torch.ones(4 * V - 1, dtype=dt, device=DEV), kb, V)
            assert (host(y) == np.float32(2.0 ** -127)).all() and 2.0 ** -127 > 0


@pytest.mark.parametrize("off", (1, 2, 3))
def test_unaligned_views_give_the_aligned_results(off):
    from ina_amd import ops
    rng = np.random.default_rng(off)
    V, W, n = 32, 4, 64 * 32 + 3
    x = ref.bucket(rng, W, n, V)
    xs = [dev(r) for r in x]
    shifted = [dev(np.concatenate([np.zeros(off, np.float32), r]))[off:] for r in x]
    assert all(t.data_ptr() % 16 for t in shifted)
    a, kb = ops.quantize_reduce_blk(xs, V)
    b, kb2 = ops.quantize_reduce_blk(shifted, V)
    assert torch.equal(a, b) and torch.equal(kb, kb2)
    a16, fa, ka = ops.quantize_reduce_i16_blk(xs, V)
    out = torch.empty(n + off, dtype=torch.int16, device=DEV)[off:]
    b16, fb, kb3 = ops.quantize_reduce_i16_blk(shifted, V, out=out)
    assert torch.equal(a16, b16) and torch.equal(fa, fb) and torch.equal(ka, kb3)
    assert torch.equal(ops.block_scales(xs, V), ops.block_scales(shifted, V))
    ya = ops.dequantize_blk(a, kb, V)
    yb = ops.dequantize_blk(dev(np.concatenate([np.zeros(off, np.int32), host(a)]))[off:], kb, V)
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    pa = ops.ps_combine_ina_blk(xs[0], xs, V, WSTEP)
    pb = ops.ps_combine_ina_blk(shifted[0], shifted, V, WSTEP)
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
    # ... and equal to the oracle, so both paths are right
    same(a, ref.quantize_reduce_i32(x, ref.kblk_ref(x, V, W, 32), V), "aligned result")


@pytest.mark.parametrize("V", (32, 12))
def test_in_place(V):
    from ina_amd import ops
    rng = np.random.default_rng(V)
    W, n = 5, 64 * V + 3
    x = ref.bucket(rng, W, n, V)
    for Wn in (4, 5):                      # register-held and re-read
        xs = [dev(r) for r in x[:Wn]]
        want = ref.quantize_reduce_i32(x[:Wn], ref.kblk_ref(x[:Wn], V, Wn, 32), V)
        got, _ = ops.quantize_reduce_blk(xs, V, out=xs[0].view(torch.int32))     # out aliases bufs[0]
        same(got, want, f"in place reduce V={V} W={Wn}")
        local = (x[0] * np.float32(0.75)).astype(np.float32)
        xs, ld = [dev(r) for r in x[:Wn]], dev(local)
        kbl = ref.kblk_ref(x[:Wn], V, Wn, 32, base=local)
        ops.ps_combine_ina_blk(ld, xs, V, WSTEP, out=ld)                          # out aliases local
        same(ld, ref.ps_combine_ina(local, x[:Wn], kbl, V, WSTEP), f"in place PS combine V={V} W={Wn}")
        s32 = ref.quantize_reduce_i32(x[:Wn], kbl, V)
        ld = dev(local)
        ops.ps_apply_blk(ld, dev(s32), dev(kbl), V, WSTEP, out=ld)
        same(ld, ref.ps_apply(local, s32, kbl, V, WSTEP), f"in place PS apply V={V}")


# ---- what the feature buys --------------------------------------------------------------------
@pytest.mark.parametrize("W,V", ((16, 256), (8, 32), (16, 8)))
def test_int16_accuracy_under_block_scales(W, V):
    """Per block |dequantise(AUTO int16 sum) - float64 sum| <= W * amax_s / (32767 / W - 1/2) with
    no flag set: each of the W roundings is <= 2^-k / 2, and k + 1 failing ina_scale_for's test
    gives 2^-k < 2 * amax_s / lim.  The global k leaves at least half of the blocks all zero."""
    from ina_amd import ops
    rng = np.random.default_rng(20260)
    nblk = 96
    n = nblk * V
    x = ref.bucket(rng, W, n, V)
    xs = [dev(r) for r in x]
    out, flags, kb = ops.quantize_reduce_i16_blk(xs, V)
    y = host(ops.dequantize_blk(out, kb, V)).astype(np.float64)
    assert not host(flags).any()
    exact = x.astype(np.float64).sum(0)
    lim = 32767.0 / W - 0.5
    for s, sl in enumerate(ref.blocks(n, V)):
        amax = float(np.abs(x[:, sl]).max())
        err = float(np.abs(y[sl] - exact[sl]).max())
        assert err <= W * amax / lim, (s, err, W * amax / lim)
    k = ops.scale_for_workers(xs, bits=16)
    g, _ = ops.quantize_reduce_i16(xs, k, V)
    zero = sum(1 for sl in ref.blocks(n, V) if not host(g)[sl].any())
    assert zero >= nblk // 2, zero


# ---- the PS surface ---------------------------------------------------------------------------
class _Worker:
    def __init__(self, paras):
        self.updated_paras = paras


def test_ps_block_scales_and_the_existing_k_values():
    from ina_amd import ops, ps
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.ReLU(), torch.nn.Linear(53, 11)).to(DEV)
    local = torch.nn.utils.parameters_to_vector(model.parameters()).detach().clone()
    n, W, V = local.numel(), 3, 256
    assert n % 256
    rng = np.random.default_rng(5)
    paras = [local + dev(ref.bucket(rng, 1, n, V, lo=-7, hi=0)[0]) for _ in range(W)]
    lh, ph = host(local), [host(p) for p in paras]
    kbl = ref.kblk_ref(ph, V, W, 32, base=lh)
    same(ps.combine_ina(local, paras, "block", 0.1), ref.ps_combine_ina(lh, ph, kbl, V, 0.1), "combine_ina block")
    kb64 = ref.kblk_ref(ph, 64, W, 32, base=lh)
    same(ps.combine_ina(local, paras, "block", 0.1, block=64), ref.ps_combine_ina(lh, ph, kb64, 64, 0.1),
         "combine_ina block=64")
    from oracle import oracle as orc
    same(ps.combine_ina(local, paras, 16, 0.1), orc.ps_combine_ina_f32(lh, ph, 16, 0.1), "k=16 as before")
    ka = ops.scale_for_workers(paras, base=local)
    same(ps.combine_ina(local, paras, "auto", 0.1), orc.ps_combine_ina_f32(lh, ph, ka, 0.1), "k=auto as before")
    ws = 1.0 / (W + 1) * 0.5
    workers = [_Worker(p.clone()) for p in paras]
    out = ps.aggregate(model, workers, 0.5, mode="ina", k="block")
    same(out, ref.ps_combine_ina(lh, ph, kbl, V, ws), "aggregate k=block")
    same(torch.nn.utils.parameters_to_vector(model.parameters()).detach(), ref.ps_combine_ina(lh, ph, kbl, V, ws),
         "aggregate wrote the model")
