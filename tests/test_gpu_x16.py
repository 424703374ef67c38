"""GPU parity of the bf16 / fp16 gradient paths (include/ina.h "bf16 / fp16 gradients").

Widening a 16-bit float to fp32 is exact, so every expectation is the existing CPU oracle on
the CPU-widened input (`t.float().numpy()`): the quantiser, the fused reduces, the packs and
absmax from a 16-bit bucket give bit for bit what the fp32 entry points give on the widened
bucket, and the dequantiser gives the fp32 result rounded once (to nearest even) to the target
type.  Every comparison is bit-exact; 16-bit outputs are compared as raw bit patterns."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
NS = [1, 7, 8, 9, 511, 512, 513, 4097, 100003]
NMAX, WMAX = 100003, 17


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ina_amd import ops  # noqa: F401


def ops():
    from ina_amd import ops as o
    return o


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(t):
    """The raw bit patterns of a 16-bit float tensor, on the host."""
    torch.cuda.synchronize()
    return t.detach().cpu().view(torch.int16).numpy()


def wide(t):
    """Exact fp32 widening on the CPU: what the oracle takes."""
    return t.detach().cpu().float().numpy()


@functools.lru_cache(maxsize=None)
def grads(dtype):
    """WMAX worker buckets of NMAX values, N(0, 1e-2) with 1 % outliers x100, in
    `dtype`: (host 16-bit tensors, device copies, widened fp32 arrays).  Made once; tests slice."""
    rng = np.random.default_rng(16 if dtype == torch.bfloat16 else 17)
    cpu, dev, w32 = [], [], []
    for _ in range(WMAX):
        x = rng.standard_normal(NMAX) * 1e-2
        x[rng.random(NMAX) < 0.01] *= 100.0
        t = torch.from_numpy(x.astype(np.float32)).to(dtype)
        cpu.append(t)
        dev.append(t.to(DEV))
        w32.append(t.float().numpy())
    return cpu, dev, w32


def fbase(n, seed=5):
    return (np.random.default_rng(seed).standard_normal(n) * 1e-2).astype(np.float32)


# ---- 1. all 65,536 bit patterns ----------------------------------------------------------
def all_patterns(dtype):
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_every_bit_pattern(dtype):
    o = ops()
    x = all_patterns(dtype)
    w, xd = wide(x), x.to(DEV)
    assert np.isnan(w).any() and np.isinf(w).any() and (w == 0).sum() == 2
    for k in (-8, 0, 16, 24):
        got = host(o.quantize(xd, k))
        assert np.array_equal(got, orc.quantize_i32(w, k)), k
        assert (got[np.isnan(w)] == 0).all()
        assert (got[w == np.inf] == 2**31 - 1).all() and (got[w == -np.inf] == -2**31).all()
    if dtype == torch.float16:
        # exact subnormal widening: the smallest fp16 subnormal, 2^-24, is 1 at k = 24
        one = torch.tensor([1, 0x03FF, -32767], dtype=torch.int16).view(torch.float16).to(DEV)
        assert host(o.quantize(one, 24)).tolist() == [1, 1023, -1]


@pytest.mark.parametrize("V", [8, 32, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_i16_every_bit_pattern(dtype, V):
    o = ops()
    x = all_patterns(dtype)
    w, xd = wide(x), x.to(DEV)
    for k in (0, 8):
        q, f = o.quantize_i16(xd, k, V)
        wq, wf = orc.quantize_i16_sat(w, k, V)
        assert np.array_equal(host(q), wq), k
        assert np.array_equal(host(f), wf), k
        nan_slots = np.unique(np.flatnonzero(np.isnan(w)) // V)
        assert (host(q)[np.isnan(w)] == 0).all() and (host(f)[nan_slots] == 1).all()
        assert 0 < host(f).sum() < f.numel()            # both kinds of slot occur


# ---- 2. shapes and tails --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_shapes(dtype):
    o = ops()
    _, dev, w32 = grads(dtype)
    for n in NS:
        assert np.array_equal(host(o.quantize(dev[0][:n].clone(), 16)), orc.quantize_i32(w32[0][:n], 16)), n


@pytest.mark.parametrize("W", [1, 2, 3, 4, 8, 16, 17])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_reduce_shapes(dtype, W):
    o = ops()
    _, dev, w32 = grads(dtype)
    for n in NS:
        got = o.quantize_reduce([d[:n].clone() for d in dev[:W]], 16)
        assert np.array_equal(host(got), orc.quantize_reduce_i32([a[:n] for a in w32[:W]], 16)), n


@pytest.mark.parametrize("V", [8, 32, 256])
@pytest.mark.parametrize("W", [1, 4, 8, 16, 17])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_reduce_i16_shapes(dtype, W, V):
    """k = 14: ordinary values (~1e-2 * 2^14 = 164) and their W-way sums fit int16, an outlier
    (~N(0, 1) * 2^14) saturates when it exceeds 2 sigma -- so some slots flag and some do not."""
    o = ops()
    _, dev, w32 = grads(dtype)
    k, flagged, clean = 14, 0, 0
    for n in NS:
        q, f = o.quantize_reduce_i16([d[:n].clone() for d in dev[:W]], k, V)
        wq, wf = orc.quantize_reduce_i16_sat([a[:n] for a in w32[:W]], k, V)
        assert np.array_equal(host(q), wq), n
        assert np.array_equal(host(f), wf), n
        flagged += int(wf.sum())
        clean += int((wf == 0).sum())
    assert flagged > 0 and clean > 0


# ---- 3. unaligned views ----------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_views(dtype, off):
    """buf[1:] (2-byte offset: the scalar path) and buf[8:] (16-byte offset: the vector path) of
    a larger allocation give what the oracle gives."""
    o = ops()
    n, W = 5001, 4
    _, dev, w32 = grads(dtype)
    views = [d[: n + 16].clone()[off: off + n] for d in dev[:W]]
    ws = [a[off: off + n] for a in w32[:W]]
    assert all(v.data_ptr() % 16 == (2 * off) % 16 for v in views)
    assert np.array_equal(host(o.quantize(views[0], 16)), orc.quantize_i32(ws[0], 16))
    assert np.array_equal(host(o.quantize_reduce(views, 16)), orc.quantize_reduce_i32(ws, 16))
    for V in (32, 12):                                   # 12: no ballot layout, pre-zeroed flags
        for got, want in ((o.quantize_i16(views[0], 14, V), orc.quantize_i16_sat(ws[0], 14, V)),
                          (o.quantize_reduce_i16(views, 14, V), orc.quantize_reduce_i16_sat(ws, 14, V))):
            assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1]), V
    base = fbase(n)
    m = o.absmax_multi(views, base=torch.from_numpy(base).to(DEV))
    assert host(m)[0] == max(np.abs(a - base).max() for a in ws)
    pk = o.quantize_pack_nga(views[0], 16, 32, 1, W, 1, 1)
    assert np.array_equal(host(pk), orc.pack_nga(orc.quantize_i32(ws[0], 16), 32, 1, W, 1, 1,
                                                 stride=o.nga_stride(32)))
    # an unaligned 16-bit OUTPUT of the dequantiser
    s = orc.quantize_i32(ws[0], 16)
    y = torch.zeros(n + 16, dtype=dtype, device=DEV)[off: off + n]
    o.dequantize(torch.from_numpy(s).to(DEV), 16, out=y)
    assert np.array_equal(bits(y), torch.from_numpy(orc.dequantize_i32(s, 16)).to(dtype).view(torch.int16).numpy())


# ---- 4. absmax ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("n", [1, 513, 100003])
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_absmax(dtype, W, n, with_base):
    o = ops()
    cpu, _, _ = grads(dtype)
    xs = [c[:n].clone() for c in cpu[:W]]
    if n > 1:
        xs[-1][n // 2] = float("nan")                    # ignored, as the quantiser maps it to 0
    base = fbase(n) if with_base else None
    b = torch.from_numpy(base).to(DEV) if with_base else None
    want = np.float32(max(np.nanmax(np.abs(wide(x) - (base if with_base else np.float32(0)))) for x in xs))
    dev = [x.to(DEV) for x in xs]
    assert host(o.absmax_multi(dev, base=b))[0] == want
    if W == 1:
        assert host(o.absmax(dev[0], base=b))[0] == want
    for nbits in (32, 16):
        assert o.scale_for_workers(dev, b, bits=nbits) == o.scale_for_workers([d.float() for d in dev], b, bits=nbits)


# ---- 5. packs ----------------------------------------------------------------------------------
def to_split(packed, V):
    hdr = np.zeros((len(packed), 16), np.uint8)
    hdr[:, :15] = packed[:, :15]
    return hdr, np.ascontiguousarray(packed[:, 15:15 + 4 * V])


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("n", [1, 33, 4099])
@pytest.mark.parametrize("V", [32, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_pack_nga(dtype, V, n, with_base):
    o = ops()
    _, dev, w32 = grads(dtype)
    base = fbase(n) if with_base else None
    b = torch.from_numpy(base).to(DEV) if with_base else None
    pk, d = o.quantize_pack_nga(dev[0][:n].clone(), 16, V, 3, 8, 1, 4_000_000_000, base=b, num_slots=1000, desc=True)
    delta = w32[0][:n] - base if with_base else w32[0][:n]
    want = orc.pack_nga(orc.quantize_i32(delta.astype(np.float32), 16), V, 3, 8, 1, 4_000_000_000,
                        num_slots=1000, stride=o.nga_stride(V))
    assert np.array_equal(host(pk), want)
    assert torch.equal(d, o.nga_descriptors(pk))


@pytest.mark.parametrize("V", [32, 256])
@pytest.mark.parametrize("W", [2, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_pack_nga_multi_split(dtype, W, V):
    o = ops()
    n = 4099
    _, dev, w32 = grads(dtype)
    xs = [d[:n].clone() for d in dev[:W]]
    base = fbase(n)
    b = torch.from_numpy(base).to(DEV)
    for bb in (None, b):
        args = (16, V, list(range(1, W + 1)), W, 1, 9)
        h16, p16, d16 = o.quantize_pack_nga_multi_split(xs, *args, base=bb, num_slots=1 << 13, descs=True)
        h32, p32, d32 = o.quantize_pack_nga_multi_split([x.float() for x in xs], *args, base=bb,
                                                        num_slots=1 << 13, descs=True)
        for w in range(W):
            assert torch.equal(h16[w], h32[w]) and torch.equal(p16[w], p32[w]) and torch.equal(d16[w], d32[w]), w
            delta = (w32[w][:n] - base).astype(np.float32) if bb is not None else w32[w][:n]
            wh, wp = to_split(orc.pack_nga(orc.quantize_i32(delta, 16), V, w + 1, W, 1, 9, num_slots=1 << 13), V)
            assert np.array_equal(host(h16[w]), wh) and np.array_equal(host(p16[w]), wp), w


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("V", [32, 256])
@pytest.mark.parametrize("W", [9, 17])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_pack_nga_multi_split_second_group(dtype, W, V, with_base):
    """More than 8 workers: the launches after the first take their own workers' buckets, header
    words and sequence starts (one of them wrapping 2^32 inside the bucket; num_slots no power of
    two).  Rows and descriptors against the oracle and against the fp32 call on the widened bucket."""
    o = ops()
    n = 5 * V + 3
    _, dev, w32 = grads(dtype)
    xs = [d[:n].clone() for d in dev[:W]]
    base = fbase(n) if with_base else None
    b = torch.from_numpy(base).to(DEV) if with_base else None
    seqs = [1000 * w + 7 for w in range(W)]
    seqs[W - 1] = 2**32 - 3                                        # wraps at packet 3 of 6, in the last group
    bitmaps = [0x01000193 * (w + 1) & 0xFFFFFFFF for w in range(W)]
    args = (16, V, bitmaps, W, 1, seqs)
    h16, p16, d16 = o.quantize_pack_nga_multi_split(xs, *args, base=b, num_slots=1000, descs=True)
    h32, p32, d32 = o.quantize_pack_nga_multi_split([x.float() for x in xs], *args, base=b, num_slots=1000,
                                                    descs=True)
    for w in range(W):
        assert torch.equal(h16[w], h32[w]) and torch.equal(p16[w], p32[w]) and torch.equal(d16[w], d32[w]), w
        delta = (w32[w][:n] - base).astype(np.float32) if with_base else w32[w][:n]
        rows = orc.pack_nga(orc.quantize_i32(delta, 16), V, bitmaps[w], W, 1, seqs[w], num_slots=1000)
        wh, wp = to_split(rows, V)
        assert np.array_equal(host(h16[w]), wh) and np.array_equal(host(p16[w]), wp), w
        assert np.array_equal(host(d16[w]), np.ascontiguousarray(rows[:, 4:12]).view(np.int64).ravel()), w


# ---- 6. dequantise to 16-bit ------------------------------------------------------------------
HAND32 = [257, 259, -257,                   # bf16 ties at k = 0 (8 significant bits): to even
          2049, 2051, -2049,                # fp16 ties at k = 0 (11 significant bits)
          65519, 65520, 65536, -65520,      # fp16: the largest value that rounds down, then +-inf
          1, 3, -1, -3, 0,                  # fp16 subnormal results at k = 24 / 25 (3 * 2^-25: a tie)
          (1 << 24) + 1, (1 << 24) + 3, (1 << 30) + 64, -(1 << 24) - 1,   # the fp32 conversion rounds first
          -2**31, 2**31 - 1]
HAND16 = [257, 259, -257, 2049, 2051, -2049, 1, 3, -1, -3, 0, 32767, -32768]


@pytest.mark.parametrize("k", [0, 8, 16, 24, 25])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dequantize_to_16bit(dtype, k):
    o = ops()
    rng = np.random.default_rng(k)
    cases = [np.array(HAND32, np.int64).astype(np.int32), np.array(HAND16, np.int16)]
    for n in (1, 9, 4097):
        cases.append(rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32))
        cases.append((rng.integers(-2**31, 2**31, n, dtype=np.int64) >> rng.integers(0, 31, n)).astype(np.int32))
        cases.append(rng.integers(-2**15, 2**15, n, dtype=np.int64).astype(np.int16))
    for s in cases:
        f32 = orc.dequantize_i32(s, k) if s.dtype == np.int32 else orc.dequantize_i16(s, k)
        want = torch.from_numpy(f32).to(dtype).view(torch.int16).numpy()
        sd = torch.from_numpy(s).to(DEV)
        assert np.array_equal(bits(o.dequantize(sd, k, dtype=dtype)), want), (s.dtype, s.size)
        out = torch.empty(s.size, dtype=dtype, device=DEV)
        assert o.dequantize(sd, k, out=out) is out       # the dtype of `out` decides
        assert np.array_equal(bits(out), want)


def test_dequantize_pins():
    """The hand-made values spelled out: ties to even, fp16 overflow and subnormals."""
    o = ops()

    def dq(vals, k, dtype):
        return bits(o.dequantize(torch.tensor(vals, dtype=torch.int32, device=DEV), k, dtype=dtype)).view(np.uint16).tolist()

    assert dq([257, 259, -257], 0, torch.bfloat16) == [0x4380, 0x4382, 0xC380]          # 256, 260, -256
    assert dq([2049, 2051], 0, torch.float16) == [0x6800, 0x6802]                        # 2048, 2052
    assert dq([65519, 65520, 65536], 0, torch.float16) == [0x7BFF, 0x7C00, 0x7C00]       # 65504, inf, inf
    assert dq([1, 3], 25, torch.float16) == [0x0000, 0x0002]                             # ties: 0, 2 * 2^-24
    assert dq([1], 24, torch.float16) == [0x0001]                                        # 2^-24, not flushed


# ---- 7. unchanged surface ---------------------------------------------------------------------
def test_fp32_calls_still_equal_the_oracle():
    o = ops()
    n, W, V, k = 4099, 4, 32, 16
    _, dev, w32 = grads(torch.bfloat16)
    xs32 = [a[:n] * np.float32(1.001) for a in w32[:W]]            # not bf16-representable any more
    xd = [torch.from_numpy(a).to(DEV) for a in xs32]
    assert np.array_equal(host(o.quantize(xd[0], k)), orc.quantize_i32(xs32[0], k))
    q, f = o.quantize_i16(xd[0], 14, V)
    wq, wf = orc.quantize_i16_sat(xs32[0], 14, V)
    assert np.array_equal(host(q), wq) and np.array_equal(host(f), wf)
    assert np.array_equal(host(o.quantize_reduce(xd, k)), orc.quantize_reduce_i32(xs32, k))
    q, f = o.quantize_reduce_i16(xd, 14, V)
    wq, wf = orc.quantize_reduce_i16_sat(xs32, 14, V)
    assert np.array_equal(host(q), wq) and np.array_equal(host(f), wf)
    assert host(o.absmax(xd[0]))[0] == np.abs(xs32[0]).max()
    assert host(o.absmax_multi(xd))[0] == max(np.abs(a).max() for a in xs32)
    assert o.scale_for_workers(xd) == o.scale_for(float(max(np.abs(a).max() for a in xs32)), W)
    want = orc.pack_nga(orc.quantize_i32(xs32[0], k), V, 1, W, 1, 1, stride=o.nga_stride(V))
    assert np.array_equal(host(o.quantize_pack_nga(xd[0], k, V, 1, W, 1, 1)), want)
    hdrs, pays = o.quantize_pack_nga_multi_split(xd, k, V, list(range(1, W + 1)), W, 1, 1)
    for w in range(W):
        wh, wp = to_split(orc.pack_nga(orc.quantize_i32(xs32[w], k), V, w + 1, W, 1, 1), V)
        assert np.array_equal(host(hdrs[w]), wh) and np.array_equal(host(pays[w]), wp)
    s = orc.quantize_i32(xs32[0], k)
    y = o.dequantize(torch.from_numpy(s).to(DEV), k)
    assert y.dtype == torch.float32 and np.array_equal(host(y), orc.dequantize_i32(s, k))


def test_dtype_rules():
    o = ops()
    x16 = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    xh = torch.zeros(64, dtype=torch.float16, device=DEV)
    x32 = torch.zeros(64, dtype=torch.float32, device=DEV)
    for mix in ([x16, x32], [x32, x16], [x16, xh]):
        for call in (lambda b: o.quantize_reduce(b, 16), lambda b: o.quantize_reduce_i16(b, 8, 32),
                     lambda b: o.absmax_multi(b), lambda b: o.scale_for_workers(b),
                     lambda b: o.quantize_pack_nga_multi_split(b, 16, 32, [1, 2], 2, 1, 1)):
            with pytest.raises(TypeError, match="one dtype"):
                call(mix)
    x64 = torch.zeros(64, dtype=torch.float64, device=DEV)
    for call in (lambda: o.quantize(x64, 16), lambda: o.quantize_i16(x64, 8, 32), lambda: o.quantize_reduce([x64], 16),
                 lambda: o.absmax(x64), lambda: o.quantize_pack_nga(x64, 16, 32, 1, 1, 1, 1),
                 lambda: o.dequantize(torch.zeros(4, dtype=torch.int32, device=DEV), 0, dtype=torch.float64)):
        with pytest.raises(TypeError):
            call()
    # the paths that stay fp32-only say so
    with pytest.raises(TypeError, match="float32 only"):
        o.quantize_i16_wire(x16, 8)
    with pytest.raises(TypeError, match="float32 only"):
        o.quantize_pack_nga_multi([x16, x16], 16, 32, [1, 2], 2, 1, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_data_manager_keeps_16bit_data(dtype):
    from ina_amd.data_manager import DataManager
    cpu, _, _ = grads(dtype)
    t = cpu[0][:4099].reshape(-1)
    a = DataManager("10.0.0.1", "10.0.0.2", data=t, k=16, V=32, device=DEV)
    b = DataManager("10.0.0.1", "10.0.0.2", data=t.float(), k=16, V=32, device=DEV)
    assert torch.equal(a.data, b.data)
    assert torch.equal(a.packets(1, 1, 2), b.packets(1, 1, 2))
    assert np.array_equal(host(a.data), orc.quantize_i32(wide(t), 16))


# ---- 8. round trip -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 10, 20])
def test_bf16_round_trip(k):
    """x = m * 2^-k with |m| < 256 (8 significant bits: exact in bf16, |x * 2^k| < 2^23):
    quantise gives m, dequantise to bf16 gives x back bit for bit."""
    o = ops()
    m = np.random.default_rng(k).integers(-255, 256, 4097)
    x = torch.from_numpy((m * 2.0 ** -k).astype(np.float32)).to(torch.bfloat16)
    assert np.array_equal(wide(x), (m * 2.0 ** -k).astype(np.float32))
    xd = x.to(DEV)
    q = o.quantize(xd, k)
    assert np.array_equal(host(q), m.astype(np.int32))
    assert np.array_equal(bits(o.dequantize(q, k, dtype=torch.bfloat16)), x.view(torch.int16).numpy())
