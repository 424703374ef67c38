"""GPU parity of the block-scaled entry points for bf16 / fp16 buckets (include/ina_x16_blk.h, ina_amd.blk).

Widening a 16-bit float to fp32 is exact, so every expectation is the existing per-block CPU oracle
(tests/_blk_ref.py) on the CPU-widened input (`t.float().numpy()`) -- never the fp32 kernels of this
library.  Scales, values, flags, packet rows and descriptors are compared bit for bit; a decode into a
16-bit buffer is the oracle's fp32 result converted once on the CPU, compared as raw bit patterns."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _blk_ref as ref
from tests import _blk_x16_lab as lab

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
VS = (8, 32, 256)
WS = (1, 2, 3, 4, 8, 16, 17)          # held instances, the runtime instance (3, 17), the int16 re-read at 16
NUM_SLOTS = 16384
SENT = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ina_amd import blk  # noqa: F401


def blk():
    from ina_amd import blk as b
    return b


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(t):
    torch.cuda.synchronize()
    return t.detach().cpu().view(torch.int16).numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what):
    got = host(got) if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got.view(f"u{got.itemsize}") != want.view(f"u{want.itemsize}"))      # bit for bit
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def flags_ff(nblk):
    return torch.full((nblk,), 0xFF, dtype=torch.uint8, device=DEV)


# ---- 1. every bit pattern -----------------------------------------------------------------------
def all_patterns(dtype):
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_bit_pattern(dtype, V):
    b = blk()
    x = all_patterns(dtype)
    w, xd, nblk = x.float().numpy(), x.to(DEV), 65536 // V
    # the oracle sees every NaN as the quiet one: numpy's fmax, which _blk_ref takes a block's max with, returns
    # NaN for a signalling NaN instead of ignoring it.  A NaN's payload means nothing to the contract.
    w = np.where(np.isnan(w), np.float32(np.nan), w)
    with np.errstate(invalid="ignore", over="ignore"):
        scales = {}
        for nbits in (16, 32):
            want = ref.kblk_ref([w], V, 1, nbits)
            assert (want == -126).any() and (want == 127).any()          # inf blocks; all-NaN, zero and tiny ones
            same(b.block_scales([xd], V, bits=nbits), want, f"block_scales bits={nbits}")
            scales[nbits] = want
        # the blocks' own scales through the per-block oracle; one hand-set scale for the whole bucket is the
        # oracle's global-k call the per-block one makes, on every block at once
        for name, kb in (("own", scales[32]), ("own16", scales[16])):
            same(b.quantize(xd, dev(kb), V), ref.quantize_i32(w, kb, V), f"quantize {name}")
            q16, f16 = ref.quantize_i16(w, kb, V)
            got, fl = b.quantize_i16(xd, dev(kb), V, overflow=flags_ff(nblk))
            same(got, q16, f"quantize_i16 {name}")
            same(fl, f16, f"quantize_i16 flags {name}")
        for k in (-128, -127, -126, 0, 127):
            kbd = torch.full((nblk,), k, dtype=torch.int8, device=DEV)
            same(b.quantize(xd, kbd, V), orc.quantize_i32(w, ref.keff(k)), f"quantize k={k}")
            q16, f16 = orc.quantize_reduce_i16_sat([w], ref.keff(k), V)
            got, fl = b.quantize_i16(xd, kbd, V, overflow=flags_ff(nblk))
            same(got, q16, f"quantize_i16 k={k}")
            same(fl, f16, f"quantize_i16 flags k={k}")


# ---- 2. reduces ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bucket(dtype, V, n, W=17, seed=0):
    """W worker buckets with block magnitudes 1e-7 .. 1e3 in `dtype`: (device tensors, widened fp32 [W, n])."""
    rng = np.random.default_rng(1000 * V + n + seed)
    t = torch.from_numpy(ref.bucket(rng, W, n, V, lo=-7.0, hi=3.0)).to(dtype)
    return [r.to(DEV) for r in t], t.float().numpy()


def check_reduces(b, xs, w, V, tag, degree=None):
    """AUTO and GIVEN, int32 and int16, on the buckets xs (widened: w [W, n])."""
    W, n = w.shape
    nblk = (n + V - 1) // V
    deg = degree or W
    kb32, kb16 = ref.kblk_ref(w, V, deg, 32), ref.kblk_ref(w, V, deg, 16)
    s32 = ref.quantize_reduce_i32(w, kb32, V)
    s16, f16 = ref.quantize_reduce_i16(w, kb16, V)
    got, kb = b.quantize_reduce(xs, V, degree=degree)
    same(kb, kb32, f"AUTO i32 scales {tag}")
    same(got, s32, f"AUTO i32 {tag}")
    got, kb = b.quantize_reduce(xs, V, kblk=dev(kb32))
    same(got, s32, f"GIVEN i32 {tag}")
    same(kb, kb32, f"given scales untouched {tag}")
    got, fl, kb = b.quantize_reduce_i16(xs, V, degree=degree, overflow=flags_ff(nblk))
    same(kb, kb16, f"AUTO i16 scales {tag}")
    same(got, s16, f"AUTO i16 {tag}")
    same(fl, f16, f"AUTO i16 flags {tag}")
    # GIVEN with the int32 scales: 16 bits too large for int16, so blocks saturate and their flags say so
    hot = kb16.copy()
    hot[::3] = np.minimum(hot[::3].astype(int) + 6, 127).astype(np.int8)
    s16h, f16h = ref.quantize_reduce_i16(w, hot, V)
    got, fl, _ = b.quantize_reduce_i16(xs, V, kblk=dev(hot), overflow=flags_ff(nblk))
    same(got, s16h, f"GIVEN i16 {tag}")
    same(fl, f16h, f"GIVEN i16 flags {tag}")
    same(b.block_scales(xs, V, bits=16, degree=degree), kb16, f"block_scales {tag}")


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduces(dtype, V):
    b = blk()
    for n in (1, 4 * V + 3, 5123):
        xs, w = bucket(dtype, V, n)
        for W in WS:
            check_reduces(b, xs[:W], w[:W], V, f"{dtype} V={V} n={n} W={W}")
    xs, w = bucket(dtype, V, 4 * V + 3)
    check_reduces(b, xs[:4], w[:4], V, f"{dtype} V={V} degree 16 over W=4", degree=16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_stride_under_the_default_cap(dtype):
    """The kernels under tuning key 0 at a grid of two workgroups: the int16 reduce (11 regions over 8 waves), the
    scalar kernel (V = 12: 427 blocks over 8 waves) and the pack (832 chunks over 512 threads)."""
    from ina_amd import ops
    b = blk()
    ops.set_tuning(max_blocks=2)
    try:
        for V, W in ((32, 4), (32, 16), (32, 3), (12, 3)):
            xs, w = bucket(dtype, V, 5123)
            check_reduces(b, xs[:W], w[:W], V, f"max_blocks=2 {dtype} V={V} W={W}")
        check_pack(b, dtype, V=256, W=2, with_base=True, auto=True)
        check_pack(b, dtype, V=256, W=2, with_base=True, auto=False)
    finally:
        ops.set_tuning(max_blocks=16384)


@pytest.fixture(scope="module")
def lab_records(tmp_path_factory):
    """tests/_blk_x16_lab.py once, in a fresh process on libina_lab.so (the caps of the scales, the int32 reduce
    and the decode are lab keys): its records by name."""
    from ina_amd import _lib
    from tests.conftest import REPO
    so = os.path.join(os.path.dirname(_lib.LIB_PATH), "libina_lab.so")
    assert os.path.exists(so), f"{so} is not built (make -C csrc lab; __graft_entry__.build() makes it)"
    out = str(tmp_path_factory.mktemp("blk_x16") / "lab.jsonl")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_blk_x16_lab.py"), out], cwd=REPO,
                       env=dict(os.environ, INA_LIBRARY="libina_lab.so"), capture_output=True, text=True, timeout=300)
    recs = {}
    if os.path.exists(out):
        with open(out) as fh:
            recs = {rec["name"]: rec for rec in map(json.loads, fh)}
    return r, recs


@pytest.mark.parametrize("name", lab.IDS)
def test_grid_stride_under_the_lab_caps(lab_records, name):
    r, recs = lab_records
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert name in recs, f"the child stopped before {name}: {r.stderr[-1500:]}"
    assert recs[name]["ok"] and recs[name]["checks"] > 0, recs[name]


# ---- 3. scalar path -----------------------------------------------------------------------------
def shifted(t, off):
    """A copy of t that starts `off` elements into its allocation."""
    s = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)[off:]
    s.copy_(t)
    return s


@pytest.mark.parametrize("case", ["off1", "off4", "V12", "V512"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_scalar_path(dtype, case):
    b = blk()
    V = {"V12": 12, "V512": 512}.get(case, 32)
    off = {"off1": 1, "off4": 4}.get(case, 0)
    n = 4 * V + 3 if V == 512 else 5123
    xs, w = bucket(dtype, V, n)
    for W in (1, 4, 5):
        xw = [shifted(x, off) for x in xs[:W]]
        if off:
            assert all(t.data_ptr() % 16 == 2 * off for t in xw)          # 2 bytes: scalar; 8: the 16-bit side's vector rule
        check_reduces(b, xw, w[:W], V, f"{dtype} {case} W={W}")
    if not off:
        return
    # the 32-bit and int16 sides `off` elements off: 4 / 16 and 2 / 8 bytes
    W, nblk = 4, (n + V - 1) // V
    kb32, kb16 = ref.kblk_ref(w[:W], V, W, 32), ref.kblk_ref(w[:W], V, W, 16)
    out32 = shifted(torch.zeros(n, dtype=torch.int32, device=DEV), off)
    got, _ = b.quantize_reduce(xs[:W], V, out=out32)
    s32 = ref.quantize_reduce_i32(w[:W], kb32, V)
    same(got, s32, f"int32 out off {off}")
    out16 = shifted(torch.zeros(n, dtype=torch.int16, device=DEV), off)
    got, fl, _ = b.quantize_reduce_i16(xs[:W], V, out=out16, overflow=flags_ff(nblk))
    s16, f16 = ref.quantize_reduce_i16(w[:W], kb16, V)
    same(got, s16, f"int16 out off {off}")
    same(fl, f16, f"int16 out off {off} flags")
    for s, kb in ((s32, kb32), (s16, kb16)):
        want = torch.from_numpy(ref.dequantize(s, kb, V)).to(dtype).view(torch.int16).numpy()
        y = shifted(torch.zeros(n, dtype=dtype, device=DEV), off)
        assert np.array_equal(bits(b.dequantize(shifted(dev(s), off), dev(kb), V, out=y)), want), (s.dtype, off)


@pytest.mark.parametrize("off", (1, 2))
@pytest.mark.parametrize("dtype", DTYPES)
def test_32bit_side_off_its_alignment_beside_aligned_buckets(dtype, off):
    """The 16-bit buckets are vector-eligible (16-byte aligned); an int32 `out`, an fp32 `base` or an int32 source
    4 or 8 bytes off 16-byte alignment sends the call to the scalar kernel, with the same results."""
    b = blk()
    V, W, n = 32, 4, 5123
    xs, w = bucket(dtype, V, n)
    xs, w = xs[:W], w[:W]
    assert all(x.data_ptr() % 16 == 0 for x in xs)
    kb32 = ref.kblk_ref(w, V, W, 32)
    s32 = ref.quantize_reduce_i32(w, kb32, V)
    out32 = shifted(torch.zeros(n, dtype=torch.int32, device=DEV), off)
    assert out32.data_ptr() % 16 == 4 * off
    for kblk in (None, kb32):
        got, kb = b.quantize_reduce(xs, V, kblk=None if kblk is None else dev(kblk), out=out32)
        same(got, s32, f"int32 out {4 * off} bytes off")
        same(kb, kb32, f"scales, int32 out {4 * off} bytes off")
    same(b.quantize(xs[0], dev(kb32), V, out=out32), ref.quantize_i32(w[0], kb32, V), f"quantize, out {4 * off} bytes off")
    base = (np.random.default_rng(off).standard_normal(n) * 1e-3).astype(np.float32)
    bd = shifted(dev(base), off)
    assert bd.data_ptr() % 16 == 4 * off
    for nbits in (16, 32):
        same(b.block_scales(xs, V, bits=nbits, base=bd), ref.kblk_ref(w, V, W, nbits, base=base),
             f"block_scales bits={nbits}, base {4 * off} bytes off")
    want = torch.from_numpy(ref.dequantize(s32, kb32, V)).to(dtype).view(torch.int16).numpy()
    assert np.array_equal(bits(b.dequantize(shifted(dev(s32), off), dev(kb32), V, dtype=dtype)), want)


@pytest.mark.parametrize("V", (32, 12))
@pytest.mark.parametrize("W", (4, 3, 16))                # held, and the re-read instances (runtime W; W = 16)
@pytest.mark.parametrize("dtype", DTYPES)
def test_int16_out_may_alias_the_first_bucket(dtype, W, V):
    b = blk()
    n = 5123
    _, w = bucket(dtype, V, n)
    w = w[:W]
    kb16 = ref.kblk_ref(w, V, W, 16)
    s16, f16 = ref.quantize_reduce_i16(w, kb16, V)
    for kblk in (None, kb16):
        xs = [torch.from_numpy(r).to(dtype).to(DEV) for r in w]               # fresh: the call overwrites xs[0]
        sep, fsep, _ = b.quantize_reduce_i16([x.clone() for x in xs], V, kblk=None if kblk is None else dev(kblk))
        got, fl, kb = b.quantize_reduce_i16(xs, V, kblk=None if kblk is None else dev(kblk),
                                            out=xs[0].view(torch.int16), overflow=flags_ff(kb16.size))
        assert got.data_ptr() == xs[0].data_ptr()
        assert torch.equal(got, sep) and torch.equal(fl, fsep)
        same(got, s16, f"aliased out V={V} {'AUTO' if kblk is None else 'GIVEN'}")
        same(fl, f16, "aliased out flags")
        same(kb, kb16, "aliased out scales")


# ---- 4. decode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (32, 256, 12))
@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_into_16bit(dtype, V):
    b = blk()
    rng = np.random.default_rng(V)
    n = 40 * V + 3                                             # ragged; several waves at V = 256
    nblk = (n + V - 1) // V
    kb = rng.integers(-126, 128, nblk).astype(np.int8)
    kb[:6] = (-126, 127, 0, -15, -16, -128)                    # fp16: 2^15 * 3 overflows to inf; -128 reads as -126
    s32 = (rng.integers(-2**31, 2**31, n, dtype=np.int64) >> rng.integers(0, 31, n)).astype(np.int32)
    s32[2 * V:2 * V + 4] = (257, 259, 65519, 65520)            # ties to even; fp16: 65504 and inf at k = 0
    s16 = rng.integers(-2**15, 2**15, n, dtype=np.int64).astype(np.int16)
    for s in (s32, s16):
        f32 = ref.dequantize(s, kb, V)
        want = torch.from_numpy(f32).to(dtype).view(torch.int16).numpy()
        if dtype == torch.float16:
            assert (np.isinf(torch.from_numpy(f32).to(dtype).float().numpy()) & np.isfinite(f32)).any()    # fp16 overflow
        sd, kd = dev(s), dev(kb)
        assert np.array_equal(bits(b.dequantize(sd, kd, V, dtype=dtype)), want), (s.dtype, V)
        out = torch.full((n + 5,), 1.0, dtype=dtype, device=DEV)
        assert b.dequantize(sd, kd, V, out=out) is out         # the dtype of `out` decides
        assert np.array_equal(bits(out)[:n], want) and (host(out[n:].float()) == 1.0).all()
        same(b.dequantize(sd, kd, V), f32, "fp32 decode goes to ops")


# ---- 5. worker pack -----------------------------------------------------------------------------
def sentinel(shape, dtype=torch.uint8):
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((int(np.prod(shape)) * size,), SENT, dtype=torch.uint8, device=DEV).view(dtype).reshape(shape)


def check_pack(b, dtype, V, W, with_base, auto):
    """Header rows, payload rows, descriptors and scales against oracle.pack_nga of the per-block oracle's
    values of the widened deltas (the construction of tests/test_gpu_blk_packets.py)."""
    n, seq0 = 4 * V * 3 + 5, 0xFFFFFFFE                        # the sequence numbers wrap inside the bucket
    xs, w = bucket(dtype, V, n, seed=W)
    xs, w = xs[:W], w[:W].copy()
    base = (np.random.default_rng(V + W).standard_normal(n) * 1e-3).astype(np.float32) if with_base else None
    if with_base:                                              # packet 0: all-zero deltas -> 127
        base[:V] = w[0, :V]
        xs = [x.clone() for x in xs]
        for x in xs:
            x[:V] = xs[0][:V]
        w[:, :V] = w[0, :V]
    want_k = ref.kblk_ref(w, V, W, 32, base=base)
    if not auto:
        want_k[1:4] = (127, -128, -126)
    npk = want_k.size
    hdrs = [sentinel((npk + 2, 16)) for _ in range(W)]
    pays = [sentinel((npk + 2, 4 * V)) for _ in range(W)]
    descs = [sentinel((npk + 3,), torch.int64) for _ in range(W)]
    kout = sentinel((npk + 3,), torch.int8)
    kw = dict(kblk_out=kout) if auto else dict(kblk=dev(want_k))
    h, p, d, k = b.quantize_pack_nga_multi_split(xs, V, list(range(1, W + 1)), W, 1, seq0,
                                                 base=None if base is None else dev(base), num_slots=NUM_SLOTS,
                                                 hdrs=hdrs, pays=pays, descs=descs, **kw)
    k = host(k)
    assert np.array_equal(k[:npk], want_k), (k[:npk], want_k)
    if auto:
        assert (k[npk:].view(np.uint8) == SENT).all()
    for i in range(W):
        delta = (w[i] - base).astype(np.float32) if base is not None else w[i]
        rows = orc.pack_nga(ref.quantize_i32(delta, want_k, V), V, i + 1, W, 1, seq0, num_slots=NUM_SLOTS)
        wh = np.zeros((npk, 16), np.uint8)
        wh[:, :15] = rows[:, :15]
        gh, gp, gd = host(h[i]), host(p[i]), host(d[i])
        assert np.array_equal(gh[:npk], wh) and (gh[npk:] == SENT).all(), i
        assert np.array_equal(gp[:npk], rows[:, 15:15 + 4 * V]) and (gp[npk:] == SENT).all(), i
        assert np.array_equal(gd[:npk], np.ascontiguousarray(rows[:, 4:12]).view(np.int64).ravel()), i
        assert (gd[npk:].view(np.uint8) == SENT).all(), i


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("W", [2, 8, 9])                 # 9 crosses a pack group: AUTO runs the scales first
@pytest.mark.parametrize("V", [32, 256, 12])             # 12: AUTO runs the scales first
@pytest.mark.parametrize("dtype", DTYPES)
def test_worker_pack(dtype, V, W, with_base):
    for auto in (True, False):
        check_pack(blk(), dtype, V, W, with_base, auto)


# ---- 6. what it buys ----------------------------------------------------------------------------
SEED = 20260            # tests/test_gpu_blk.py's: the bucket rounded to bf16 still loses more than half its blocks


def test_int16_accuracy_of_a_bf16_bucket():
    """The 96-block bucket of test_int16_accuracy_under_block_scales rounded to bf16, W = 16, V = 32: per block
    |decode(AUTO int16 sum) - float64 sum of the widened values| <= W * amax_s / (32767 / W - 1/2) with no flag set
    (each of the W roundings is <= 2^-k / 2, and k + 1 failing ina_scale_for's test gives 2^-k < 2 * amax_s / lim),
    while the oracle at the global k of scale_for_workers returns more than half of the blocks as all zeros."""
    from ina_amd import ops
    b = blk()
    W, V, nblk = 16, 32, 96
    n = nblk * V
    t = torch.from_numpy(ref.bucket(np.random.default_rng(SEED), W, n, V)).to(torch.bfloat16)
    w = t.float().numpy()
    # the oracle alone, on the CPU: the global k leaves more than half of the blocks all zero
    k = ops.scale_for(float(np.abs(w).max()), W, 16)
    g, _ = orc.quantize_reduce_i16_sat(list(w), k, V)
    zero = sum(1 for sl in ref.blocks(n, V) if not g[sl].any())
    assert zero > nblk // 2, zero
    xs = [r.to(DEV) for r in t]
    assert ops.scale_for_workers(xs, bits=16) == k
    out, flags, kb = b.quantize_reduce_i16(xs, V)
    assert not host(flags).any()
    y = host(b.dequantize(out, kb, V)).astype(np.float64)
    exact = w.astype(np.float64).sum(0)
    lim = 32767.0 / W - 0.5
    for s, sl in enumerate(ref.blocks(n, V)):
        amax = float(np.abs(w[:, sl]).max())
        err = float(np.abs(y[sl] - exact[sl]).max())
        assert err <= W * amax / lim, (s, err, W * amax / lim)
