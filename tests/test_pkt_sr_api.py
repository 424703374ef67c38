"""Stochastic rounding on the packet path: the surface and the argument checks (include/ina_pkt_sr.h,
ina_amd.sr's packs, ina_amd.loopback), with no GPU.  The header declares exactly the seven functions,
refuses a lone include and is included by ina.h once, directly after ina_sr.h; the names are in
SIGNATURES_PKT_SR and in no other table or header, exported and bound, each with its round-to-nearest
sibling's arguments plus the ina_sr_t before the stream; the checks come in the siblings' order with
their messages before any device work, then a null sr and e0 % 4, and the empty bucket is a no-op where
the sibling has it; the Python calls and worker_serve refuse by name; the yardstick's PS update is the
oracle's arithmetic; and the bias case holds on the replay alone."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _sr_pkt_ref as P

# aligned addresses that are never touched
X, BASE, PK, DESC, KB, PRM = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20
ONE, X16, BLK, MS, MSX, MSB, SCALES = ("ina_quantize_pack_nga_sr_desc", "ina_quantize_pack_nga_x16_sr_desc",
                                       "ina_quantize_pack_nga_blk_sr_desc", "ina_quantize_pack_nga_multi_split_sr",
                                       "ina_quantize_pack_nga_multi_split_x16_sr",
                                       "ina_quantize_pack_nga_multi_split_blk_sr", "ina_block_scales_sr_f32")
PACKS = (ONE, X16, BLK, MS, MSX, MSB)
NAMES = set(PACKS) | {SCALES}
SIBLING = {ONE: ("SIGNATURES", "ina_quantize_pack_nga_desc"), X16: ("SIGNATURES_X16", "ina_quantize_pack_nga_x16_desc"),
           BLK: ("SIGNATURES_PKT_BLK", "ina_quantize_pack_nga_blk_desc"),
           MS: ("SIGNATURES", "ina_quantize_pack_nga_multi_split"),
           MSX: ("SIGNATURES_X16", "ina_quantize_pack_nga_multi_split_x16"),
           MSB: ("SIGNATURES_PKT_BLK", "ina_quantize_pack_nga_multi_split_blk")}
BAD_TYPE = b"16-bit type must be INA_X16_BF16 (1) or INA_X16_F16 (2)"
NOSR = "none"


def _lib():
    from ina_amd import _lib as L
    return L


def _call(name, x=X, base=BASE, n=64, k=9, V=32, t=1, sr=None, e0=0, pkts=PK, stride=None, desc=DESC, kblk=KB,
          W=2, mode=0, degree=2, prm="ok", slots=16384, hdr=PK, pay=PK + (1 << 16), xs="ok"):
    """The call `name` on never-touched addresses, one argument at a time made bad."""
    L = _lib()
    lib = L.load()
    srp = None if sr is NOSR else ctypes.byref(L.SrParams(0x1234, e0, 0, 0))
    stride = 16 + 4 * max(V, 0) if stride is None else stride
    one = ctypes.byref(L.NgaParams(1, 2, 0, 1, 0, 1, slots, V)) if prm == "ok" else None
    many = (L.NgaParams * W)(*[L.NgaParams(1 << w, W, 0, 1, 0, 1, slots, V) for w in range(W)]) if prm == "ok" else None
    arr = lambda p, step=1 << 12: L.ptr_array([p + w * step if p else None for w in range(W)])  # noqa: E731
    xa = arr(x) if xs == "ok" else None
    args = {ONE: (x, base, n, k, one, pkts, stride, desc, srp, None),
            X16: (x, t, base, n, k, one, pkts, stride, desc, srp, None),
            BLK: (x, base, n, kblk, one, pkts, stride, desc, srp, None),
            MS: (xa, W, base, n, k, many, arr(hdr), arr(pay), arr(desc), srp, None),
            MSX: (xa, t, W, base, n, k, many, arr(hdr), arr(pay), arr(desc), srp, None),
            MSB: (xa, W, base, n, kblk, mode, degree, many, arr(hdr), arr(pay), arr(desc), srp, None)}[name]
    return getattr(lib, name)(*args), lib.ina_last_error_string()


def _einval(name, msg, **kw):
    rc, err = _call(name, **kw)
    assert rc == _lib().INA_EINVAL and msg in err, (name, kw, rc, err)


def test_header_declares_the_seven_and_they_are_exported_and_bound():
    L = _lib()
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_pkt_sr.h")).read()
    includes = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(inc, "ina.h")).read(), flags=re.M)
    assert includes.count("ina_pkt_sr.h") == 1
    assert includes.index("ina_pkt_sr.h") == includes.index("ina_sr.h") + 1            # directly after
    assert re.search(r"#ifndef INA_SR_H\n#error", src)                                 # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == NAMES == set(L.SIGNATURES_PKT_SR)
    tables = [t for t in dir(L) if t.startswith("SIGNATURES") and t != "SIGNATURES_PKT_SR"]
    assert len(tables) >= 11
    for t in tables:
        assert not declared & set(getattr(L, t)), t
    for h in sorted(os.listdir(inc)):                                                  # declared nowhere else
        if h == "ina_pkt_sr.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = L.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == L.SIGNATURES_PKT_SR[name] and fn.restype is ctypes.c_int, name
    vp, srp = ctypes.c_void_p, ctypes.POINTER(L.SrParams)
    for name, (table, sib) in SIBLING.items():                       # the sibling's arguments, sr before the stream
        want = list(getattr(L, table)[sib])
        assert L.SIGNATURES_PKT_SR[name] == want[:-1] + [srp, vp], name
    assert L.SIGNATURES_PKT_SR[SCALES] == L.SIGNATURES_BLK["ina_block_scales_f32"]


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_pkt_sr.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { ina_sr_t s = {1, 0, 0, 0}; return '
                 'ina_quantize_pack_nga_sr_desc(0, 0, 0, 1, 0, 0, 0, 0, &s, 0) + '
                 'ina_quantize_pack_nga_x16_sr_desc(0, INA_X16_BF16, 0, 0, 1, 0, 0, 0, 0, &s, 0) + '
                 'ina_quantize_pack_nga_blk_sr_desc(0, 0, 0, 0, 0, 0, 0, 0, &s, 0) + '
                 'ina_quantize_pack_nga_multi_split_sr(0, 1, 0, 0, 1, 0, 0, 0, 0, &s, 0) + '
                 'ina_quantize_pack_nga_multi_split_x16_sr(0, INA_X16_F16, 1, 0, 0, 1, 0, 0, 0, 0, &s, 0) + '
                 'ina_quantize_pack_nga_multi_split_blk_sr(0, 1, 0, 0, 0, INA_BLK_AUTO, 1, 0, 0, 0, 0, &s, 0) + '
                 'ina_block_scales_sr_f32(0, 1, 0, 0, 8, 1, 32, 0, 0); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_checks_come_in_the_siblings_order_then_sr_then_e0():
    worst = dict(sr=NOSR, e0=2)                            # what must be reported last
    for t in (0, 3, -1):                                   # the type code first, before everything
        for name in (X16, MSX):
            _einval(name, BAD_TYPE, t=t)
            _einval(name, BAD_TYPE, t=t, n=0, k=500, x=None, **worst)
    for k in (-127, 128, 500):
        for name in (ONE, X16, MS, MSX):
            _einval(name, b"k out of range [-126,127]", k=k)
            _einval(name, b"k out of range", k=k, n=0, x=None, prm=None, **worst)
    # the packed calls: pointers, the descriptor's alignment, the geometry, the empty bucket, the rows, then sr
    for name in (ONE, X16, BLK):
        _einval(name, b"null pointer", x=None, **worst)
        _einval(name, b"descriptors must be 8-byte aligned", desc=DESC + 4, prm=None, **worst)
        _einval(name, b"bad nga params", prm=None, **worst)
        _einval(name, b"bad nga params", V=0, **worst)
        _einval(name, b"bad nga params", slots=0, **worst)
        _einval(name, b"stride < 15 + 4V", stride=15 + 4 * 32 - 1, pkts=None, **worst)
        _einval(name, b"null pointer", pkts=None, **worst)
        _einval(name, b"null sr", sr=NOSR)
        _einval(name, b"null sr", sr=NOSR, base=None, desc=None)
        for e0 in (1, 2, 3, 6, (1 << 40) + 1):
            _einval(name, b"e0 must be a multiple of 4", e0=e0)
    _einval(BLK, b"null pointer", kblk=None, **worst)
    _einval(X16, b"16-bit buffers must be 2-byte aligned", x=X + 1, desc=DESC + 4, **worst)
    # the split calls: check_multi_split's order, then sr
    wbad = b"x, prm, hdr, pay non-null and W in [1, 64]"
    for name in (MS, MSX, MSB):
        _einval(name, wbad, W=0, **worst)
        _einval(name, wbad, W=65, **worst)
        _einval(name, wbad, xs=None, **worst)
        _einval(name, wbad, prm=None, **worst)
        _einval(name, b"split rows need V a multiple of 4 in [4, 256]", V=6, **worst)
        _einval(name, b"split rows need V", V=260, **worst)
        _einval(name, b"split rows need V", slots=0, **worst)
        _einval(name, b"base must be 16-byte aligned", base=BASE + 4, x=None, **worst)
        _einval(name, b"null worker buffer", x=None, **worst)
        _einval(name, b"null worker buffer", hdr=None, **worst)
        _einval(name, b"worker buffers and rows must be 16-byte aligned", x=X + 8, **worst)
        _einval(name, b"descriptors must be non-null and 8-byte aligned", desc=DESC + 4, **worst)
        _einval(name, b"null sr", sr=NOSR)
        _einval(name, b"null sr", sr=NOSR, base=None)
        for e0 in (1, 2, 3, 6, (1 << 40) + 1):
            _einval(name, b"e0 must be a multiple of 4", e0=e0)
    # the block-scaled split call: mode, then what ina_scale_for_sr refuses, then the rest
    _einval(MSB, b"mode must be INA_BLK_GIVEN (0) or INA_BLK_AUTO (1)", mode=2, degree=0, W=0, **worst)
    _einval(MSB, b"degree must be >= 1", mode=1, degree=0, W=0, **worst)
    _einval(MSB, b"too many summands (degree) for this width", mode=1, degree=2147483647, W=0, **worst)
    rc, err = _call(MSB, mode=0, degree=0, n=0)            # GIVEN does not look at degree
    assert rc == _lib().INA_OK, err
    _einval(MSB, b"null kblk", kblk=None, **worst)
    _einval(MSB, b"null kblk", kblk=None, mode=1, **worst)


def test_empty_bucket_is_a_no_op_where_the_sibling_has_it():
    L = _lib()
    for name in PACKS:
        for kw in ({}, dict(sr=NOSR), dict(e0=2), dict(base=None, desc=None)):
            rc, err = _call(name, n=0, **kw)
            assert rc == L.INA_OK, (name, kw, err)
    for name in (ONE, X16, BLK):                           # after the stride, before the rows
        rc, err = _call(name, n=0, x=None, pkts=None, kblk=None, sr=NOSR)
        assert rc == L.INA_OK, (name, err)
        _einval(name, b"stride < 15 + 4V", n=0, stride=8)
    for name in (MS, MSX, MSB):                            # after the geometry, before the buffers
        rc, err = _call(name, n=0, x=None, hdr=None, pay=None, kblk=None, base=BASE + 4, sr=NOSR)
        assert rc == L.INA_OK, (name, err)
        _einval(name, b"split rows need V", n=0, V=6)


def test_block_scales_sr_checks_are_the_siblings_with_the_extra_quantum():
    L = _lib()
    lib = L.load()
    xs = L.ptr_array([X, X + 4096])

    def call(f, W=2, n=64, V=32, degree=2, bits=32, kblk=KB, xs=xs, base=BASE):
        return getattr(lib, f)(xs, W, base, n, V, degree, bits, kblk, None), lib.ina_last_error_string()

    for kw, msg in ((dict(V=0), b"V must be"), (dict(bits=8), b"bits must be 16 or 32"),
                    (dict(degree=0), b"degree must be >= 1"), (dict(W=0), b"W must be in [1, 64]"),
                    (dict(W=65), b"W must be in [1, 64]"), (dict(xs=None), b"W must be in [1, 64]"),
                    (dict(kblk=None), b"null kblk"),
                    (dict(xs=L.ptr_array([X, None])), b"null worker buffer")):
        for f in (SCALES, "ina_block_scales_f32"):
            rc, err = call(f, **kw)
            assert rc == L.INA_EINVAL and msg in err, (f, kw, err)
    # lim = (2^(bits-1) - 1) / degree - 1: what ina_scale_for_sr refuses, one degree earlier than to nearest
    rc, err = call(SCALES, bits=16, degree=32767)
    assert rc == L.INA_EINVAL and b"too many summands (degree) for this width" in err
    k = ctypes.c_int(0)
    assert lib.ina_scale_for_sr(1.0, 32767, 16, ctypes.byref(k)) == L.INA_EINVAL
    assert call("ina_block_scales_f32", bits=16, degree=32767, n=0)[0] == L.INA_OK
    assert call(SCALES, bits=16, degree=16383, n=0)[0] == L.INA_OK and lib.ina_scale_for_sr(1.0, 16383, 16, ctypes.byref(k)) == L.INA_OK
    assert call(SCALES, n=0, kblk=None, xs=None)[0] == L.INA_OK                     # the empty bucket: the sibling's place
    assert call("ina_block_scales_f32", n=0, kblk=None, xs=None)[0] == L.INA_OK


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind _req's device test are
    reached without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def test_python_calls_refuse_by_name_before_any_device_call():
    from ina_amd import sr
    kw = dict(V=32, bitmap=1, count=2, switch_id=1, seq0=1)
    mkw = dict(V=32, bitmaps=[1, 2], count=2, switch_id=1, seq0=1)
    f32, bf, fp = (_FakeDev(torch.zeros(64, dtype=d)) for d in (torch.float32, torch.bfloat16, torch.float16))
    kblk = _FakeDev(torch.zeros(2, dtype=torch.int8))
    one = lambda x, k=9, seed=1, **more: sr.quantize_pack_nga(x, k, seed=seed, **kw, **more)          # noqa: E731
    many = lambda xs, k=9, seed=1, **more: sr.quantize_pack_nga_multi_split(xs, k, seed=seed, **mkw, **more)  # noqa: E731
    for f, x in ((one, f32), (many, [f32, f32])):
        for seed in (1.5, "7", None, True):
            with pytest.raises(TypeError, match="seed must be an int"):
                f(x, seed=seed)
        with pytest.raises(ValueError, match=r"seed must be in \[0, 2\^64\)"):
            f(x, seed=1 << 64)
        for e0 in (1, 2, 7):
            with pytest.raises(ValueError, match=f"e0 must be a multiple of 4, got {e0}"):
                f(x, e0=e0)
        with pytest.raises(ValueError, match=r"sub must be in \[0, 2\^32\)"):
            f(x, sub=1 << 32)
        with pytest.raises(TypeError, match="k must be an int"):
            f(x, k=9.0)
        with pytest.raises(ValueError, match="base and xs? differ in length"):
            f(x, base=_FakeDev(torch.zeros(63)))
    with pytest.raises(TypeError, match="k must be an int or an int8 tensor"):         # only the split pack computes scales
        one(f32, k=None)
    for x16 in (bf, fp):                                   # a 16-bit bucket with block scales
        with pytest.raises(ValueError, match=f"stochastic rounding with block scales takes fp32 buckets: x is {x16.dtype}"):
            one(x16, k=kblk)
        for k in (kblk, None):
            with pytest.raises(ValueError, match=rf"block scales takes fp32 buckets: xs\[1\] is {x16.dtype}"):
                many([f32, x16], k=k)
        with pytest.raises(ValueError, match=rf"block scales takes fp32 buckets: xs\[0\] is {x16.dtype}"):
            sr.block_scales([x16], 32)
        with pytest.raises(TypeError, match="all workers of one call share one dtype"):    # mixed dtypes
            many([f32, x16])
    with pytest.raises(TypeError, match="all workers of one call share one dtype"):
        many([bf, fp])
    with pytest.raises(ValueError, match="x must be a device .* no CPU fallback"):
        one(torch.zeros(64))
    with pytest.raises(TypeError, match="kblk must be torch.int8"):
        one(f32, k=_FakeDev(torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="kblk holds 1 elements, needs 2"):
        one(f32, k=_FakeDev(torch.zeros(1, dtype=torch.int8)))
    with pytest.raises(ValueError, match="degree 2147483647 cannot be summed at 32 bits"):  # fits to nearest, not here
        many([f32, f32], k=None, degree=2147483647)
    with pytest.raises(ValueError, match="degree 32767 cannot be summed at 16 bits"):
        sr.block_scales([f32], 32, bits=16, degree=32767)
    prm = inspect.signature(sr.quantize_pack_nga_multi_split).parameters
    assert [prm[p].default for p in ("step", "sub", "e0", "base", "degree", "kblk_out")] == [0, 0, 0, None, None, None]
    prm = inspect.signature(sr.block_scales).parameters
    assert list(prm) == ["xs", "V", "bits", "degree", "base", "out"] and prm["bits"].default == 32


def test_loopback_arguments():
    from ina_amd import loopback
    prm = inspect.signature(loopback.worker_serve).parameters
    assert prm["rounding"].default == "nearest" and prm["seed"].default == 0
    prm = inspect.signature(loopback.worker_send).parameters
    assert [prm[p].default for p in ("rounding", "seed", "step", "sub")] == ["nearest", 0, 0, 0]
    assert "rounding" not in inspect.signature(loopback.ps_serve).parameters          # the PS sees integers
    args = (0, 2, 1, "/nonexistent/switch.sock", None, None)         # refused before any socket is opened
    with pytest.raises(ValueError, match="not combined with error_feedback"):
        loopback.worker_serve(*args, rounding="stochastic", error_feedback=True)
    with pytest.raises(ValueError, match="unknown rounding 'sr'"):
        loopback.worker_serve(*args, rounding="sr")
    with pytest.raises(TypeError, match="seed must be an int"):
        loopback.worker_serve(*args, rounding="stochastic", seed=1.5)
    with pytest.raises(ValueError, match="not combined with error_feedback"):
        loopback.worker_send(None, None, None, 1, 2, 32, 9, 1, residual=torch.zeros(4), rounding="stochastic")
    from tests.conftest import REPO
    src = open(os.path.join(REPO, "examples", "config1_loopback.py")).read()
    assert '"--rounding"' in src and '"--seed"' in src


def test_the_helpers_ps_update_is_the_oracles_arithmetic():
    """With nearest rounding substituted, the helper's update equals orc.ps_combine_ina_f32 bit for bit."""
    rng = np.random.default_rng(11)
    n, W = 4099, 3
    local = rng.standard_normal(n).astype(np.float32)
    paras = [(local + rng.standard_normal(n).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 2, n)).astype(np.float32)
             for _ in range(W)]
    for k in (16, 9, 30, -3):                              # 30: the W-way sum wraps
        qs = [orc.quantize_i32((p - local).astype(np.float32), k) for p in paras]
        for ws in (1.0 / (W + 1), 0.1):
            want = orc.ps_combine_ina_f32(local, paras, k, ws)
            got = P.ps_update(local, qs, k, 32, ws)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, ws)
    # per-packet scales all equal to k read as k; -127 / -128 as -126
    qs = [orc.quantize_i32((p - local).astype(np.float32), 16) for p in paras]
    kb = np.full((n + 31) // 32, 16, np.int8)
    assert np.array_equal(P.ps_update(local, qs, kb, 32, 0.25), P.ps_update(local, qs, 16, 32, 0.25))
    assert list(P.scales_read(np.array([-128, -127, -126, 0, 127], np.int8))) == [-126, -126, -126, 0, 127]


def test_the_helpers_scales_are_sr_refs():
    """_sr_pkt_ref.scale_for_sr (bisection) is _sr_ref.scale_for_sr (the scan) and ina_scale_for_sr."""
    from ina_amd import sr
    from tests import _sr_ref as S
    rng = np.random.default_rng(5)
    amax = [0.0, 1e-45, 1.1754942e-38, 3e-30, 2.0 ** -20, 0.3, 1.0, 1.0000001, 510.0, 32766.0, 2.0 ** 31, 1e30, 3e38]
    amax += list(np.exp(rng.uniform(np.log(1e-44), np.log(1e38), 60)))
    for bits in (16, 32):
        for W in (1, 2, 8, 64):
            for a in amax:
                a = np.float32(a)
                assert P.scale_for_sr(a, W, bits) == S.scale_for_sr(a, W, bits) == sr.scale_for(float(a), W, bits), (a, W, bits)
    x = np.zeros(32, np.float32)
    x[3], x[9], x[20] = np.nan, -0.75, np.inf
    got = P.block_scales([x, 2 * x], 8, 2)
    assert list(got) == [127, S.scale_for_sr(1.5, 2, 32), -126, 127]


def test_bias_case_on_the_replay():
    """W = 4 workers of 65,536 values 0.3f * 2^-9 at k = 9: to nearest every sum is 0; stochastically the
    mean of the sums lies within 5 sigma of 1.2, sigma = sqrt(4 * 0.21 / 65,536) = 0.00358."""
    assert not P.bias_case(2024, "nearest").any()
    sigma = (4 * 0.21 / 65536) ** 0.5
    for seed, mean in ((2024, 1.20502), (7, 1.19716)):
        s = P.bias_case(seed)
        assert set(np.unique(s)) <= set(range(5))
        print(f"seed {seed}: mean {s.mean():.5f} ({abs(s.mean() - 1.2) / sigma:.1f} sigma)")
        assert abs(s.mean() - 1.2) <= 5 * sigma
        assert abs(s.mean() - mean) < 5e-6
