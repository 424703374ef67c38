"""Parity at the ABI's stated limits: W up to INA_MAX_WORKERS (64), k at both ends of [-126, 127],
and the int16 wire at its 64-rank limit (include/ina.h, csrc/ina_shard.hip).

Every comparison is bit for bit against the CPU oracle (oracle/oracle.py) or tests/_blk_ref.py,
floats through their bit patterns, into 0xA5-filled outputs a few elements longer than the result.
Inputs and expectations are built once in tests/_limits.py.  No Python wrapper refuses a W the C
header allows: every entry point below runs at W = 64 and refuses 65."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _blk_ref as ref
from tests import _limits as L
from tests._limits import DEV, FILL, K16, K32, N1, V1, dev, dev_rows, mixed, ops, same, sent

pytestmark = pytest.mark.gpu

OFFS = pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
WS = pytest.mark.parametrize("W", L.W_LIMIT)
SRC = pytest.mark.parametrize("src", ["f32", "bf16", "f16"])
HDR = dict(count=7, switch_id=1, num_slots=1000)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def small_cap(fn):
    """fn() under a grid cap of 4 workgroups (tuning keys 0 and 3, the ones the product library
    accepts): every kernel under the default cap, and the sum-reduce, strides over n = 70,001."""
    o = ops()
    try:
        o.set_tuning(max_blocks=L.SMALL_CAP, reduce_blocks=L.SMALL_CAP)
        fn()
        torch.cuda.synchronize()
    finally:      # the defaults in csrc/ina_kernels.hip (g_max_blocks, g_reduce_blocks); the ABI has no getter
        o.set_tuning(max_blocks=16384, reduce_blocks=0)


def as_src(x, src):
    """fp32 [W, n] -> (what the device gets, what the oracle gets)."""
    if src == "f32":
        return x, x
    return L.widen(x, L.X16[src])


# =============================================================================================
# part 1: W in {17, 33, 63, 64}
# =============================================================================================
def check_sum_reduce(W, n, off):
    x = L.i32_bufs(W, n)
    want = orc.sum_reduce_i32(list(x))
    out = sent(n, torch.int32, off)
    ops().sum_reduce(dev_rows(x, off), out=out)
    same(out, want, f"sum_reduce W={W} n={n}")
    assert want[5] == (0 if W % 2 == 0 else L.I32_MIN)      # W x INT32_MIN wraps


@WS
@OFFS
def test_sum_reduce(W, off):
    check_sum_reduce(W, N1, off)


def check_sum_reduce_host(W, n, off, pinned):
    """Host buffers: pinned ones are reduced in place over PCIe by one launch over W host pointers,
    pageable ones through the copy pipeline, 256 values a chunk; `off`: views one int32 past the
    allocation's start."""
    x = L.i32_bufs(W, n)
    bufs = []
    for r in x:
        t = torch.empty(n + off, dtype=torch.int32)
        t = t.pin_memory() if pinned else t
        t[off:].copy_(torch.from_numpy(r))
        bufs.append(t[off:])
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32)
    out = out.pin_memory() if pinned else out
    ops().sum_reduce_host(bufs, out=out, chunk=256)
    same(out.numpy(), orc.sum_reduce_i32(list(x)), f"sum_reduce_host W={W} n={n} pinned={pinned}")


@WS
@OFFS
@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_sum_reduce_host(W, off, pinned):
    check_sum_reduce_host(W, N1, off, pinned)


def check_sum_reduce_i16(W, n, off):
    q, clear, flagged = L.i16_plan(W, n, V1)
    want, wf = orc.sum_reduce_i16_sat(list(q), V1)
    mixed(wf)
    assert not wf[list(clear)].any() and wf[list(flagged)].all()
    out, fl = sent(n, torch.int16, off), sent(wf.size, torch.uint8)
    ops().sum_reduce_i16(dev_rows(q, off), V1, out=out, overflow=fl)
    same(out, want, f"sum_reduce_i16 W={W} n={n}")
    same(fl, wf, f"sum_reduce_i16 flags W={W} n={n}")


@WS
@OFFS
def test_sum_reduce_i16(W, off):
    check_sum_reduce_i16(W, N1, off)


def check_quantize_reduce(W, n, off, src):
    xd, xo = as_src(L.f32path_bufs(W, n), src)
    out = sent(n, torch.int32, off)
    ops().quantize_reduce(dev_rows(xd, off), K32, out=out)
    same(out, orc.quantize_reduce_i32(list(xo), K32), f"quantize_reduce {src} W={W} n={n}")


@WS
@OFFS
@SRC
def test_quantize_reduce(W, off, src):
    check_quantize_reduce(W, N1, off, src)


def check_quantize_reduce_i16(W, n, off, src):
    x, clear, flagged = L.f16path_bufs(W, n, V1)
    xd, xo = as_src(x, src)
    want, wf = orc.quantize_reduce_i16_sat(list(xo), K16, V1)
    mixed(wf)
    if src == "f32":
        assert not wf[list(clear)].any() and wf[list(flagged)].all()
    out, fl = sent(n, torch.int16, off), sent(wf.size, torch.uint8)
    ops().quantize_reduce_i16(dev_rows(xd, off), K16, V1, out=out, overflow=fl)
    same(out, want, f"quantize_reduce_i16 {src} W={W} n={n}")
    same(fl, wf, f"quantize_reduce_i16 flags {src} W={W} n={n}")


@WS
@OFFS
@SRC
def test_quantize_reduce_i16(W, off, src):
    check_quantize_reduce_i16(W, N1, off, src)


def check_ps_combines(W, n, off):
    from ina_amd import ps
    local, paras = L.ps_bufs(W, n)
    ws = 1.0 / (W + 1)
    dl, dp = dev(local, off), dev_rows(paras, off)
    out = sent(n, torch.float32, off)
    ops().ps_combine(dl, dp, ws, out=out)
    same(out, orc.ps_combine_f32(local, list(paras), ws), f"ps_combine W={W} n={n}")
    out = sent(n, torch.float32, off)
    ps.combine_ina(dl, dp, K32, ws, out=out)
    same(out, orc.ps_combine_ina_f32(local, list(paras), K32, ws), f"combine_ina W={W} n={n}")


@WS
@OFFS
def test_ps_combine_and_combine_ina(W, off):
    check_ps_combines(W, N1, off)


def check_absmax_multi(W, n, off, src):
    """The maximum only in worker W - 1, then only in worker 16: in the vector loop and in the last
    value; with and without a base, against numpy.  scale_for_workers is that pass and the host function
    scale_for: the oracle has no scale rule of its own, so only "the k of the maximum found" is checked
    here, against the product's scale_for of the numpy maximum, not the rule itself."""
    o = ops()
    x, base = L.quiet_bufs(W, n)
    xd, xo = as_src(x, src)
    rows, db = dev_rows(xd, off), dev(base, off)
    for w in (W - 1, 16):
        for idx in (4 * 37 + 2, n - 1):
            keep = rows[w][idx].clone()
            rows[w][idx] = 3.0
            for b, dbb in ((None, None), (base, db)):
                d = np.array(xo, np.float32)
                d[w, idx] = 3.0
                if b is not None:
                    d = (d - b[None, :]).astype(np.float32)
                want = np.abs(d).max().astype(np.float32)
                assert want == np.abs(d[w, idx]) and want > 2.9
                out = sent(1, torch.float32)
                o.absmax_multi(rows, base=dbb, out=out)
                same(out, np.array([want]), f"absmax_multi {src} W={W} n={n} worker {w} value {idx}")
                for nbits in (32, 16):
                    assert o.scale_for_workers(rows, base=dbb, bits=nbits) == o.scale_for(float(want), W, nbits)
            rows[w][idx] = keep


@WS
@OFFS
@SRC
def test_absmax_multi_and_scale_for_workers(W, off, src):
    check_absmax_multi(W, N1, off, src)


def want_packs(x, base, k, V, seqs, stride):
    for w, r in enumerate(x):
        with np.errstate(all="ignore"):
            d = (r - base).astype(np.float32) if base is not None else r
        yield orc.pack_nga(orc.quantize_i32(d, k), V, w + 1, HDR["count"], HDR["switch_id"], seqs[w],
                           num_slots=HDR["num_slots"], stride=stride)


def check_packs(W, n, off):
    """The multi-worker packs (groups of 8 workers a launch).  Offset buckets: the packed form takes the
    per-worker byte path, the split form refuses them (its rows and buckets are 16-byte aligned)."""
    from ina_amd._lib import InaError
    o = ops()
    x, base = L.f32path_bufs(W, n), L.quiet_bufs(W, n)[1]
    seqs = [2**32 - 30 + 1000 * w for w in range(W)]
    stride, npk = o.nga_stride(V1), -(-n // V1)
    rows, db = dev_rows(x, off), dev(base, off)
    for b, dbb in ((None, None), (base, db)):
        want = list(want_packs(x, b, K32, V1, seqs, stride))
        outs = [sent(npk * stride, torch.uint8) for _ in range(W)]
        _, descs = o.quantize_pack_nga_multi(rows, K32, V1, range(1, W + 1), seq0=seqs, base=dbb, outs=outs,
                                             descs=True, **HDR)
        for w in range(W):
            same(outs[w], want[w], f"quantize_pack_nga_multi W={W} worker {w}")
            same(descs[w], np.ascontiguousarray(want[w][:, 4:12]), f"quantize_pack_nga_multi desc worker {w}")
        if off:
            with pytest.raises(InaError, match="16-byte aligned"):
                o.quantize_pack_nga_multi_split(rows, K32, V1, range(1, W + 1), seq0=seqs, base=None, **HDR)
            continue
        hdrs, pays = o.quantize_pack_nga_multi_split(rows, K32, V1, range(1, W + 1), seq0=seqs, base=dbb, **HDR)
        for w in range(W):
            same(hdrs[w][:, :15].contiguous(), np.ascontiguousarray(want[w][:, :15]), f"split headers worker {w}")
            same(pays[w], np.ascontiguousarray(want[w][:, 15:15 + 4 * V1]), f"split payload worker {w}")


@WS
@OFFS
def test_multi_worker_packs(W, off):
    check_packs(W, N1, off)


def check_blk(W, n, off):
    """The per-block variants, scales GIVEN (the int16 ones raised in every third block, so that some
    blocks saturate) and AUTO (a NaN / an inf in a block flag it)."""
    o = ops()
    x = L.blk_bufs(W, n, V1)
    rows = dev_rows(x, off)
    kb32, kb16 = ref.kblk_ref(x, V1, W, 32), ref.kblk_ref(x, V1, W, 16)
    given16 = kb16.copy()
    given16[::3] = np.minimum(given16[::3].astype(np.int32) + 3, 127).astype(np.int8)
    nblk = kb32.size
    for tag, k32, k16 in (("GIVEN", kb32, given16), ("AUTO", None, None)):
        out, kout = sent(n, torch.int32, off), sent(nblk, torch.int8)
        o.quantize_reduce_blk(rows, V1, kblk=None if k32 is None else dev(k32), out=out, kblk_out=kout)
        same(out, ref.quantize_reduce_i32(x, kb32, V1), f"quantize_reduce_blk {tag} W={W} n={n}")
        want, wf = ref.quantize_reduce_i16(x, kb16 if k16 is None else k16, V1)
        mixed(wf)
        out, fl, kout16 = sent(n, torch.int16, off), sent(nblk, torch.uint8), sent(nblk, torch.int8)
        o.quantize_reduce_i16_blk(rows, V1, kblk=None if k16 is None else dev(k16), out=out, overflow=fl,
                                  kblk_out=kout16)
        same(out, want, f"quantize_reduce_i16_blk {tag} W={W} n={n}")
        same(fl, wf, f"quantize_reduce_i16_blk flags {tag} W={W} n={n}")
        if k32 is None:
            same(kout, kb32, f"AUTO int32 scales W={W}")
            same(kout16, kb16, f"AUTO int16 scales W={W}")
    finite = np.nan_to_num(x, nan=0.0, posinf=3e38, neginf=-3e38).astype(np.float32)    # no inf - inf
    local = (finite[0] * np.float32(0.75)).astype(np.float32)
    kbl = ref.kblk_ref(finite, V1, W, 32, base=local)
    out, kout = sent(n, torch.float32, off), sent(nblk, torch.int8)
    o.ps_combine_ina_blk(dev(local, off), dev_rows(finite, off), V1, 1.0 / (W + 1), out=out, kblk_out=kout)
    same(kout, kbl, f"ps_combine_ina_blk scales W={W}")
    same(out, ref.ps_combine_ina(local, finite, kbl, V1, 1.0 / (W + 1)), f"ps_combine_ina_blk W={W} n={n}")


@WS
@OFFS
def test_per_block_variants(W, off):
    check_blk(W, N1, off)


# which kernels of a case make more than one pass at n = 70,001 under small_cap (4 workgroups); the others
# sit under caps only a lab build can lower and cover 70,001 values in one pass
N70K = [
    ("sum_reduce", check_sum_reduce, (), "strides"),
    ("sum_reduce_host-pinned", check_sum_reduce_host, (True,), "strides"),
    ("sum_reduce_host-pageable", check_sum_reduce_host, (False,), "strides: 274 chunks through the pipeline"),
    ("sum_reduce_i16", check_sum_reduce_i16, (), "strides"),
    ("quantize_reduce-f32", check_quantize_reduce, ("f32",), "one pass (cap 16384 past W = 8)"),
    ("quantize_reduce-bf16", check_quantize_reduce, ("bf16",), "one pass"),
    ("quantize_reduce_i16-f32", check_quantize_reduce_i16, ("f32",), "strides"),
    ("quantize_reduce_i16-f16", check_quantize_reduce_i16, ("f16",), "strides"),
    ("ps_combines", check_ps_combines, (), "one pass (caps 256 and 8192); ps_combine strides in the by-size test below"),
    ("absmax_multi-f32", check_absmax_multi, ("f32",), "one pass (cap 512); strides in the by-size test below"),
    ("absmax_multi-bf16", check_absmax_multi, ("bf16",), "one pass (cap 512); strides in the by-size test below"),
    ("packs", check_packs, (), "one pass (cap 16384)"),
    ("blk", check_blk, (), "the int16 reduce strides; the int32 reduce, the scales and the combine make one pass"),
]


@pytest.mark.parametrize("check,args", [c[1:3] for c in N70K], ids=[c[0] for c in N70K])
def test_n_70001_at_64_workers_under_a_small_cap(check, args):
    """One case an entry point at n = 70,001 and W = 64 under a grid cap of 4 workgroups (tuning keys 0
    and 3: the two caps the product library lets a caller lower).  N70K says which kernels stride
    there; the rest run the size in one pass, W = 64 all the same."""
    small_cap(lambda: check(64, L.N_STRIDE, 0, *args))


COMBINE_CAP, MULTI_CAP, BLOCK = 256, 512, 256     # g_combine_blocks, the absmax_multi grids (test_gpu_geometry.py)


def scaled_rows(x0, W):
    """[W, n]: worker w holds x0 * (1 + w / 16), as test_gpu_geometry.py's noise()."""
    return (x0[None, :] * (1 + np.arange(W, dtype=np.float32)[:, None] / 16)).astype(np.float32)


def test_ps_combine_strides_past_its_cap_at_64_workers():
    """ps_combine's cap (256 workgroups) cannot be lowered, so n is taken past it, as
    test_ps_combine_past_its_cap does at W = 3 and 6: at W = 64 two chunks are in flight a thread, and
    3 * 65,536 + 69 chunks and one value give one two-chunk pass, a full and a ragged one-chunk pass and
    the scalar tail."""
    W, S = 64, COMBINE_CAP * BLOCK
    n = 4 * (3 * S + 69) + 1
    rng = np.random.default_rng(64)
    local = rng.standard_normal(n).astype(np.float32)
    paras = (local[None, :] + scaled_rows((rng.standard_normal(n) * 1e-2).astype(np.float32), W)).astype(np.float32)
    paras[W - 1, [5, 4 * 2 * S + 7, 4 * 3 * S + 70, n - 1]] += np.float32(1e3)      # every pass needs worker W - 1
    out = sent(n, torch.float32)
    ops().ps_combine(dev(local), dev_rows(paras), 1.0 / (W + 1), out=out)
    same(out, orc.ps_combine_f32(local, list(paras), 1.0 / (W + 1)), f"ps_combine W={W} n={n}")


@SRC
def test_absmax_multi_strides_past_its_cap_at_64_workers(src):
    """absmax_multi's grids stop at 512 workgroups of one chunk a thread: 131,072 + 69 chunks and one
    value make a full pass, a ragged one and the scalar tail.  The maximum is planted in the second pass
    and in the tail, in worker W - 1 and in worker 16 alone, with a base."""
    o, W, S = ops(), 64, MULTI_CAP * BLOCK
    n = 4 * (S + 69) + 1
    rng = np.random.default_rng(65)
    xd, xo = as_src(scaled_rows((rng.standard_normal(n) * 1e-3).astype(np.float32), W), src)
    base = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    quiet = np.abs(xo - base[None, :]).max()
    assert quiet < 0.1
    rows, db = dev_rows(xd), dev(base)
    for w in (W - 1, 16):
        for idx in (4 * (S + 5) + 2, n - 1):
            keep = rows[w][idx].clone()
            rows[w][idx] = 3.0
            out = sent(1, torch.float32)
            o.absmax_multi(rows, base=db, out=out)
            same(out, np.abs(np.float32(3.0) - base[idx:idx + 1]), f"absmax_multi {src} n={n} worker {w} value {idx}")
            rows[w][idx] = keep


def refuses(calls, exc, pattern):
    """Every call raises `exc` with a message matching `pattern`; a failure names the call's index."""
    import re
    for i, call in enumerate(calls):
        try:
            call()
        except exc as e:
            assert re.search(pattern, str(e)), (i, str(e))
        else:
            pytest.fail(f"call {i} did not raise")


def test_w65_is_refused_by_every_wrapper():
    """The largest W every wrapper takes is 64 (the tests above run it); 65 is a Python error."""
    from ina_amd import ps
    o = ops()
    i32 = [torch.zeros(8, dtype=torch.int32, device=DEV)] * 65
    i16 = [torch.zeros(8, dtype=torch.int16, device=DEV)] * 65
    f32 = [torch.zeros(8, dtype=torch.float32, device=DEV)] * 65
    bf = [torch.zeros(8, dtype=torch.bfloat16, device=DEV)] * 65
    calls = [lambda: o.sum_reduce(i32), lambda: o.sum_reduce_host([t.cpu() for t in i32]),
             lambda: o.sum_reduce_i16(i16, 4), lambda: o.quantize_reduce(f32, 0), lambda: o.quantize_reduce(bf, 0),
             lambda: o.quantize_reduce_i16(f32, 0, 4), lambda: o.quantize_reduce_i16(bf, 0, 4),
             lambda: o.ps_combine(f32[0], f32, 0.5), lambda: ps.combine_ina(f32[0], f32, 0, 0.5),
             lambda: o.absmax_multi(f32), lambda: o.absmax_multi(bf), lambda: o.scale_for_workers(f32),
             lambda: o.quantize_pack_nga_multi(f32, 0, 4, range(65), 1, 1, 1),
             lambda: o.quantize_pack_nga_multi_split(f32, 0, 4, range(65), 1, 1, 1),
             lambda: o.quantize_reduce_blk(f32, 4), lambda: o.quantize_reduce_i16_blk(f32, 4),
             lambda: o.ps_combine_ina_blk(f32[0], f32, 4, 0.5)]
    refuses(calls, ValueError, r"need 1\.\.64 worker buffers, got 65")


# =============================================================================================
# part 2: k in {-126, -125, 31, 126, 127}; -127 and 128 are refused
# =============================================================================================
KS = pytest.mark.parametrize("k", L.K_LIMITS)
WSTEPS = pytest.mark.parametrize("ws", [1.0, 1.0 / 3], ids=["ws1", "ws3rd"])


@KS
@OFFS
def test_dequantize_at_k_limits(k, off):
    """int32 and int16 sources to fp32 / bf16 / fp16, and the fp32 output of i16_wire_finish.  At
    k = 127 the scale 2^-127 is a subnormal kernel argument: +-1 must come out as +-2^-127, not 0; at
    k = -126 INT32_MAX overflows to +inf."""
    o = ops()
    s32, s16 = L.deq_sources()
    for s, fn in ((s32, orc.dequantize_i32), (s16, orc.dequantize_i16)):
        want = fn(s, k)
        one, top = S_AT(s, 1), S_AT(s, int(s.max()))
        if k == 127:
            assert L.bits(want)[one] == 0x00400000 and L.bits(want)[S_AT(s, -1)] == 0x80400000
        if k == -126 and s.dtype == np.int32:
            assert L.bits(want)[top] == 0x7F800000
        d = dev(s, off)
        out = sent(s.size, torch.float32, off)
        o.dequantize(d, k, out=out)
        same(out, want, f"dequantize {s.dtype} -> fp32 k={k}")
        for name, dt in L.X16.items():
            out = sent(s.size, dt, off)
            o.dequantize(d, k, out=out)
            same(out, L.round16(want, dt), f"dequantize {s.dtype} -> {name} k={k}")
    y, fl = sent(s16.size, torch.float32, off), sent(-(-s16.size // V1), torch.uint8)
    o.i16_wire_finish(dev(s16.astype(np.int32), off), k, V1, y=y, overflow=fl, want_out16=False)
    same(y, orc.dequantize_i16(s16, k), f"i16_wire_finish y k={k}")
    same(y, orc.i16_wire_finish(s16.astype(np.int32), k, V1)[1], f"i16_wire_finish y (oracle's finish) k={k}")


def S_AT(s, v):
    return int(np.flatnonzero(s == v)[0])


@KS
@WSTEPS
@OFFS
def test_ps_apply_at_k_limits(k, ws, off):
    local, s, want, fma = L.ps_case(k, ws, L.N_DEQ)
    out = sent(s.size, torch.float32, off)
    ops().ps_apply(dev(local, off), dev(s, off), k, ws, out=out)
    same(out, want, f"ps_apply k={k} ws={ws} ({fma.size} values where one rounding differs)")


@KS
@WSTEPS
@OFFS
def test_combine_ina_at_k_limits(k, ws, off):
    from ina_amd import ps
    local, paras, want, fma = L.combine_ina_case(k, ws)
    out = sent(local.size, torch.float32, off)
    ps.combine_ina(dev(local, off), dev_rows(paras, off), k, ws, out=out)
    same(out, want, f"combine_ina k={k} ws={ws} ({fma.size} values where one rounding differs)")


SEQ0, SLOTS = 4_000_000_000, 128


@KS
@WSTEPS
def test_apply_completed_at_k_limits(k, ws):
    """ops.apply_completed takes packed rows only (split rows with an integer k exist only in the fused
    switch step, below): the sums as one completed packet a slot, with and without ack rows."""
    o = ops()
    local, s, want, _ = L.ps_case(k, ws, L.N_DEQ)
    pk = o.pack_nga(dev(s), V1, 3, 2, 1, SEQ0, num_slots=SLOTS)
    act = torch.full((pk.shape[0],), orc.ACT_FWD_AGG, dtype=torch.uint8, device=DEV)
    for acks in (None, torch.zeros_like(pk)):
        out = sent(s.size, torch.float32)
        o.apply_completed(pk, act, V1, SEQ0, dev(local), k, ws, out=out[:s.size], acks=acks)
        same(out, want, f"apply_completed k={k} ws={ws}")


@KS
@WSTEPS
@pytest.mark.parametrize("V", [8, 32])
def test_fused_switch_ps_step_at_k_limits(k, ws, V):
    """The integer-k PS step fused into ina_switch: process_apply (packed rows), process_apply_split and
    sort + run_apply, one tiny batch of W = 2 workers whose every slot completes."""
    o = ops()
    n = (48 if V == 8 else 24) * V - 3
    local, s, want, fma = L.ps_case(k, ws, n)
    rng = np.random.default_rng(abs(k) + V)
    q0 = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    q = [q0, (s.astype(np.int64) - q0).astype(np.int32)]
    assert np.array_equal(orc.sum_reduce_i32(q), s)
    dl, npk = dev(local), -(-n // V)

    def packed():
        rows, desc = zip(*[o.pack_nga(dev(b), V, w + 1, 2, 1, SEQ0, num_slots=SLOTS, desc=True) for w, b in enumerate(q)])
        return torch.cat(rows), torch.cat(desc)

    def done(act, out, what):
        same(act, want_act, f"{what}: actions")
        same(out, want, f"{what} k={k} ws={ws} V={V} ({fma.size} values where one rounding differs)")

    pk, desc = packed()
    torch.cuda.synchronize()
    want_act = orc.Switch(V, num_slots=SLOTS, switch_id=1).run(pk.cpu().numpy(), stride=pk.shape[1])[1]
    assert np.array_equal(want_act, np.repeat([orc.ACT_DROP, orc.ACT_FWD_AGG], npk))      # every slot completes
    out = sent(n, torch.float32)
    act, _ = o.Switch(V, SLOTS, 1, DEV).process_apply(pk, SEQ0, dl, k, ws, out=out[:n])
    done(act, out, "process_apply")

    pk, desc = packed()
    sw, out = o.Switch(V, SLOTS, 1, DEV), sent(n, torch.float32)
    act = sw.sort(pk, desc)
    sw.run_apply(pk, act, SEQ0, dl, k, ws, out=out[:n])
    done(act, out, "sort + run_apply")

    hp = [o.pack_nga_split(dev(b), V, w + 1, 2, 1, SEQ0, num_slots=SLOTS) for w, b in enumerate(q)]
    hdr, pay = torch.cat([h for h, _ in hp]), torch.cat([p for _, p in hp])
    out = sent(n, torch.float32)
    act, _ = o.Switch(V, SLOTS, 1, DEV).process_apply_split(hdr, pay, SEQ0, dl, k, ws, out=out[:n])
    done(act, out, "process_apply_split")


@pytest.mark.parametrize("k", [-126, 127])
@OFFS
def test_quantise_side_at_k_limits(k, off):
    """quantize_reduce (W = 3 and 8), quantize_i16, quantize_reduce_i16, quantize_i16_wire,
    quantize_pack_nga and quantize_pack_nga_multi (with and without base) at both ends of k."""
    o = ops()
    V, n = V1, 8 * V1 + 5
    for W in (3, 8):
        x = L.quant_inputs(W, n, V)
        rows = dev_rows(x, off)
        out = sent(n, torch.int32, off)
        o.quantize_reduce(rows, k, out=out)
        same(out, orc.quantize_reduce_i32(list(x), k), f"quantize_reduce W={W} k={k}")
    x = L.quant_inputs(3, n, V)
    rows = dev_rows(x, off)
    for what, bufs, call, fn in (("quantize_i16", x[0], lambda out, fl: o.quantize_i16(rows[0], k, V, out=out, overflow=fl),
                                  orc.quantize_i16_sat),
                                 ("quantize_reduce_i16", list(x), lambda out, fl: o.quantize_reduce_i16(rows, k, V, out=out, overflow=fl),
                                  orc.quantize_reduce_i16_sat)):
        want, wf = fn(bufs, k, V)
        mixed(wf)
        out, fl = sent(n, torch.int16, off), sent(wf.size, torch.uint8)
        call(out, fl)
        same(out, want, f"{what} k={k}")
        same(fl, wf, f"{what} flags k={k}")
    out = sent(n, torch.int32, off)
    o.quantize_i16_wire(rows[1], k, out=out)
    same(out, orc.quantize_i16_wire(x[1], k), f"quantize_i16_wire k={k}")
    base = (x[2] * np.float32(0.5)).astype(np.float32)
    base[~np.isfinite(base)] = 0                      # x - base without inf - inf
    stride, npk, seqs = o.nga_stride(V), -(-n // V), [5, 6, 7]
    for b in (None, base):
        db = None if b is None else dev(b, off)
        want = list(want_packs(x, b, k, V, seqs, stride))
        out = sent(npk * stride, torch.uint8)
        o.quantize_pack_nga(rows[0], k, V, 1, seq0=seqs[0], base=db, out=out, **HDR)
        same(out, want[0], f"quantize_pack_nga k={k}")
        outs = [sent(npk * stride, torch.uint8) for _ in range(3)]
        o.quantize_pack_nga_multi(rows, k, V, [1, 2, 3], seq0=seqs, base=db, outs=outs, **HDR)
        for w in range(3):
            same(outs[w], want[w], f"quantize_pack_nga_multi k={k} worker {w}")


@pytest.mark.parametrize("k", L.K_REFUSED)
def test_k_outside_the_range_is_refused(k):
    """-127 and 128 raise from every wrapper that takes an integer k; a caller's output keeps its bytes."""
    from ina_amd import ps
    from ina_amd._lib import InaError
    o = ops()
    V, n = 8, 32
    f = torch.ones(n, dtype=torch.float32, device=DEV)
    i32, i16 = torch.ones(n, dtype=torch.int32, device=DEV), torch.ones(n, dtype=torch.int16, device=DEV)
    outs = {dt: sent(n, dt) for dt in (torch.int32, torch.int16, torch.float32, torch.bfloat16, torch.float16, torch.uint8)}
    oi32, oi16, of32, fl = outs[torch.int32], outs[torch.int16], outs[torch.float32], outs[torch.uint8]
    stride = o.nga_stride(V)
    pk, desc = o.pack_nga(i32, V, 1, 1, 1, 1, num_slots=SLOTS, desc=True)
    hdr, pay = o.pack_nga_split(i32, V, 1, 1, 1, 1, num_slots=SLOTS)
    before = [t.clone() for t in (pk, hdr, pay)]
    act = torch.ones(pk.shape[0], dtype=torch.uint8, device=DEV)
    rows = torch.full((n // V, stride), FILL, dtype=torch.uint8, device=DEV)
    sw = o.Switch(V, SLOTS, 1, DEV)

    def run_apply():
        a = sw.sort(pk, desc)
        sw.run_apply(pk, a, 1, f, k, 0.5, out=of32[:n])

    calls = [lambda: o.quantize(f, k, out=oi32), lambda: o.quantize(f.bfloat16(), k, out=oi32),
             lambda: o.quantize_i16(f, k, V, out=oi16, overflow=fl), lambda: o.quantize_i16(f.half(), k, V, out=oi16, overflow=fl),
             lambda: o.quantize_i16_wire(f, k, out=oi32), lambda: o.i16_wire_finish(i32, k, V, out16=oi16, y=of32, overflow=fl),
             lambda: o.dequantize(i32, k, out=of32), lambda: o.dequantize(i16, k, out=of32),
             lambda: o.dequantize(i32, k, out=outs[torch.bfloat16]), lambda: o.dequantize(i16, k, out=outs[torch.float16]),
             lambda: o.quantize_reduce([f, f], k, out=oi32), lambda: o.quantize_reduce([f.half()] * 2, k, out=oi32),
             lambda: o.quantize_reduce_i16([f, f], k, V, out=oi16, overflow=fl),
             lambda: o.quantize_reduce_i16([f.bfloat16()] * 2, k, V, out=oi16, overflow=fl),
             lambda: o.ps_apply(f, i32, k, 0.5, out=of32), lambda: ps.combine_ina(f, [f, f], k, 0.5, out=of32),
             lambda: o.quantize_pack_nga(f, k, V, 1, 1, 1, 1, out=rows), lambda: o.quantize_pack_nga(f.half(), k, V, 1, 1, 1, 1, out=rows),
             lambda: o.quantize_pack_nga_multi([f], k, V, [1], 1, 1, 1, outs=[rows]),
             lambda: o.quantize_pack_nga_multi_split([f], k, V, [1], 1, 1, 1),
             lambda: o.quantize_pack_nga_multi_split([f.bfloat16()], k, V, [1], 1, 1, 1),
             lambda: o.apply_completed(pk, act, V, 1, f, k, 0.5, out=of32[:n]),
             lambda: sw.process_apply(pk, 1, f, k, 0.5, out=of32[:n]),
             lambda: sw.process_apply_split(hdr, pay, 1, f, k, 0.5, out=of32[:n]), run_apply]
    refuses(calls, InaError, "k out of range")
    torch.cuda.synchronize()
    for t in list(outs.values()) + [rows]:
        assert bool((t.view(torch.uint8) == FILL).all())
    assert all(torch.equal(a, b) for a, b in zip((pk, hdr, pay), before))
    assert not bool(sw.count.any()) and not bool(sw.regs.any())


# =============================================================================================
# part 3: the int16 wire on the device with 1, 2, 63 and 64 ranks
# =============================================================================================
@pytest.mark.parametrize("V", L.WIRE_V)
@pytest.mark.parametrize("R", [1, 2, 63, 64])
def test_i16_wire_at_the_rank_limit(R, V):
    """Each rank's bucket -> ops.quantize_i16_wire (== the oracle's wire), summed on the host in int64
    (inside int32), -> ops.i16_wire_finish == the one-GPU fused reduce over the R buckets
    (orc.quantize_reduce_i16_sat) and its dequantisation.  V % 4 == 0 with V / 4 a power of two <= 64
    takes the ballot flag writer, other V and every offset view the scalar kernel after a memset.  The
    three sizes: a partial last slot, n % 4 != 0, several waves; every flag is written over a 0xA5
    sentinel and nothing past ceil(n / V) changes."""
    from ina_amd import _lib
    o, k = ops(), L.WIRE_K
    kinds = set()
    for which, n in enumerate(L.wire_sizes(V)):
        x, where = L.wire_case(R, V, which)
        kinds |= set(where)
        rows, wrows = dev_rows(x), dev_rows(np.zeros((R, n), np.int32))
        for r in range(R):
            o.quantize_i16_wire(rows[r], k, out=wrows[r])
        torch.cuda.synchronize()
        wires = torch.stack(wrows).cpu().numpy()
        assert np.array_equal(wires, np.stack([orc.quantize_i16_wire(b, k) for b in x]))
        wsum = wires.astype(np.int64).sum(axis=0)
        assert np.abs(wsum).max() < 2**31
        if R == 64:             # the extremes of the 22-bit field and of the count above it
            for kind, word in (("all_hi", 64 * 32767), ("all_lo", -2**21), ("all_clamp", 64 * 32767 + (64 << 22)),
                               ("all_nan", 64 << 22), ("one_short_of_clamp", 63 * 32767 - 32768 + (63 << 22)),
                               ("one_clamps_low", 63 * 3 - 32768 + (1 << 22))):
                assert all(wsum[e] == word for e in where.get(kind, []))
        wsum = wsum.astype(np.int32)
        want16, wf = orc.quantize_reduce_i16_sat(list(x), k, V)
        want_y = orc.dequantize_i16(want16, k)
        mixed(wf)
        for e in where.get("one_clamps_low", []):
            assert wf[e // V] == 1 and want16[e] == 3 * (R - 1) - 32768    # in range, flagged all the same
        for off in (0, 1):
            ws = dev(wsum, off)
            for a, b, flags in ((1, 0, 1), (0, 1, 1), (1, 1, 1), (1, 1, 0)):
                tag = f"R={R} V={V} n={n} off={off} out16={a} y={b} flags={flags}"
                o16 = sent(n, torch.int16) if a else None
                y = sent(n, torch.float32) if b else None
                fl = sent(wf.size, torch.uint8)
                if flags:
                    o.i16_wire_finish(ws, k, V, out16=o16, y=y, overflow=fl, want_out16=False, want_y=False)
                    same(fl, wf, tag + ": flags")
                else:
                    _lib.check(o.load().ina_i16_wire_finish(ws.data_ptr(), n, k, V, o16.data_ptr(), y.data_ptr(), None,
                                                            torch.cuda.current_stream().cuda_stream), "i16_wire_finish")
                    same(fl, np.empty(0, np.uint8), tag + ": no flag buffer given")
                if a:
                    same(o16, want16, tag + ": out16")
                if b:
                    same(y, want_y, tag + ": y")
    assert kinds == set(L.WIRE_KINDS)          # the three sizes of this V planted every kind
