"""Stochastic rounding: the yardstick's generator, the surface and the argument checks (include/ina_sr.h,
ina_amd.sr, ina_amd.dist), with no GPU.  Philox4x32-10 of tests/_sr_ref.py gives the Random123 known
answers; the header declares exactly the seven functions, refuses a lone include and is included by
ina.h once, after ina_x16.h; the names are in SIGNATURES_SR and in no other table or header, exported
and bound, each with its round-to-nearest sibling's arguments plus the base and the ina_sr_t; the checks
come in the siblings' order with their messages before any device work, then a null sr and e0 % 4, and
n == 0 is a no-op; ina_scale_for_sr equals the rule in exact rationals; ina_amd.sr and the aggregator
refuse by name."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _sr_ref as sref

# aligned addresses that are never touched, far enough apart for any n used here
X, BASE, Q, OVF = 1 << 20, 2 << 20, 3 << 20, 4 << 20
F32, F16S, X32, X16S, FW, XW = ("ina_quantize_sr_f32_i32", "ina_quantize_sr_f32_i16_sat", "ina_quantize_sr_x16_i32",
                                "ina_quantize_sr_x16_i16_sat", "ina_quantize_sr_f32_i16_wire",
                                "ina_quantize_sr_x16_i16_wire")
DEVICE = (F32, F16S, X32, X16S, FW, XW)
NAMES = set(DEVICE) | {"ina_scale_for_sr"}
TYPED, SLOTTED = (X32, X16S, XW), (F16S, X16S)
BAD_TYPE = b"16-bit type must be INA_X16_BF16 (1) or INA_X16_F16 (2)"
NOSR = "none"


def _calls(x=X, base=BASE, q=Q, ovf=OVF, n=64, k=9, V=32, t=1, sr=None, e0=0):
    from ina_amd import _lib
    p = None if sr is NOSR else ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0))
    return {F32: (x, base, q, n, k, p, None), F16S: (x, base, q, n, k, V, ovf, p, None),
            X32: (x, t, base, q, n, k, p, None), X16S: (x, t, base, q, n, k, V, ovf, p, None),
            FW: (x, q, n, k, p, None), XW: (x, t, q, n, k, p, None)}


def _rc(name, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    return getattr(lib, name)(*_calls(**kw)[name]), lib.ina_last_error_string()


def _einval(name, msg, **kw):
    from ina_amd import _lib
    rc, err = _rc(name, **kw)
    assert rc == _lib.INA_EINVAL and msg in err, (name, kw, rc, err)


def test_philox_known_answers():
    """The Random123 tables' philox4x32_10 entries."""
    got = [int(v[0]) for v in sref.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = [int(v[0]) for v in sref.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)]
    assert got == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # an element's word: counter ((e0 + e) >> 2, step, sub), output word (e0 + e) & 3, the key the seed's halves
    w = sref.words(8, 0x299F31D0A4093822, step=0x13198A2E, sub=0x03707344, e0=4 * 0x85A308D3243F6A88 % (1 << 64))
    idx = (4 * 0x85A308D3243F6A88 % (1 << 64)) >> 2
    for e in range(8):
        i = idx + (e >> 2)
        want = sref.philox4x32_10(i & 0xFFFFFFFF, i >> 32, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
        assert int(w[e]) == int(want[e & 3][0])
    u = sref.uniform(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], np.uint32))
    assert u.dtype == np.float32 and list(u) == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


def test_header_declares_the_seven_and_they_are_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_sr.h")).read()
    includes = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(inc, "ina.h")).read(), flags=re.M)
    assert includes.count("ina_sr.h") == 1 and includes.index("ina_x16.h") < includes.index("ina_sr.h")
    assert re.search(r"#ifndef INA_\w+_H\n#error", src)                                    # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == NAMES == set(_lib.SIGNATURES_SR) and set(_calls()) == set(DEVICE)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16) | set(_lib.SIGNATURES_BLK) |
              set(_lib.SIGNATURES_PKT_BLK) | set(_lib.SIGNATURES_SWITCH_BLK) | set(_lib.SIGNATURES_SHARD_BLK) |
              set(_lib.SIGNATURES_BLK_X16) | set(_lib.SIGNATURES_EF) | set(_lib.SIGNATURES_SHARD_EF) |
              set(_lib.SIGNATURES_SHARD_X16))
    assert not declared & others
    for h in sorted(os.listdir(inc)):                                                      # declared nowhere else
        if h == "ina_sr.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SIGNATURES_SR[name] and fn.restype is ctypes.c_int, name
    # the siblings' arguments with the base after x / xtype (the first four) and the ina_sr_t before the stream
    vp, srp = ctypes.c_void_p, ctypes.POINTER(_lib.SrParams)
    for name, sib, base_at in ((F32, _lib.SIGNATURES["ina_quantize_f32_i32"], 1),
                               (F16S, _lib.SIGNATURES["ina_quantize_f32_i16_sat"], 1),
                               (X32, _lib.SIGNATURES_X16["ina_quantize_x16_i32"], 2),
                               (X16S, _lib.SIGNATURES_X16["ina_quantize_x16_i16_sat"], 2),
                               (FW, _lib.SIGNATURES["ina_quantize_f32_i16_wire"], None),
                               (XW, _lib.SIGNATURES_SHARD_X16["ina_quantize_x16_i16_wire"], None)):
        want = list(sib) if base_at is None else sib[:base_at] + [vp] + sib[base_at:]
        assert _lib.SIGNATURES_SR[name] == want[:-1] + [srp, vp], name
    assert _lib.SIGNATURES_SR["ina_scale_for_sr"] == _lib.SIGNATURES["ina_scale_for"]
    # ina_sr_t as the header lays it out: two 64-bit words, two 32-bit words
    assert [(f[0], ctypes.sizeof(f[1])) for f in _lib.SrParams._fields_] == [("seed", 8), ("e0", 8), ("step", 4), ("sub", 4)]
    assert ctypes.sizeof(_lib.SrParams) == 24
    m = re.search(r"typedef struct ina_sr \{(.*?)\} ina_sr_t;", code, flags=re.S)
    assert re.findall(r"(uint\d+_t)\s+(\w+);", m.group(1)) == [("uint64_t", "seed"), ("uint64_t", "e0"),
                                                              ("uint32_t", "step"), ("uint32_t", "sub")]


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_sr.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { ina_sr_t s = {1, 0, 0, 0}; int k; return '
                 'ina_quantize_sr_f32_i32(0, 0, 0, 0, 1, &s, 0) + ina_quantize_sr_f32_i16_sat(0, 0, 0, 0, 1, 8, 0, &s, 0) + '
                 'ina_quantize_sr_x16_i32(0, INA_X16_BF16, 0, 0, 0, 1, &s, 0) + '
                 'ina_quantize_sr_x16_i16_sat(0, INA_X16_F16, 0, 0, 0, 1, 8, 0, &s, 0) + '
                 'ina_quantize_sr_f32_i16_wire(0, 0, 0, 1, &s, 0) + ina_quantize_sr_x16_i16_wire(0, INA_X16_BF16, 0, 0, 1, &s, 0) + '
                 'ina_scale_for_sr(1.0f, 1, 16, &k); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_checks_come_in_the_siblings_order_then_sr_then_e0():
    for t in (0, 3, -1):                                   # the type code first, before everything
        for name in TYPED:
            _einval(name, BAD_TYPE, t=t)
            _einval(name, BAD_TYPE, t=t, n=0)
            _einval(name, BAD_TYPE, t=t, k=500, V=0, x=None, q=None, sr=NOSR, e0=2)
    for k in (-127, 128, 500):
        for name in DEVICE:
            _einval(name, b"k out of range [-126,127]", k=k)
            _einval(name, b"k out of range", k=k, n=0)     # before the empty call's no-op
            _einval(name, b"k out of range", k=k, V=0, x=None, q=None, sr=NOSR)
    for V in (0, -1):
        for name in SLOTTED:
            _einval(name, b"V must be > 0", V=V)
            _einval(name, b"V must be > 0", V=V, n=0)
            _einval(name, b"V must be > 0", V=V, x=None, sr=NOSR, e0=2)
    for name in DEVICE:
        _einval(name, b"null pointer", x=None)
        _einval(name, b"null pointer", q=None)
        _einval(name, b"null pointer", x=None, q=None, sr=NOSR, e0=2)    # the sibling's checks first
        _einval(name, b"null sr", sr=NOSR)
        _einval(name, b"null sr", sr=NOSR, base=None, ovf=None)
        for e0 in (1, 2, 3, 6, (1 << 40) + 1):
            _einval(name, b"e0 must be a multiple of 4", e0=e0)
    for name in TYPED:
        _einval(name, b"16-bit buffers must be 2-byte aligned", x=X + 1)
        _einval(name, b"null pointer", x=X + 1, q=None)
        _einval(name, b"16-bit buffers must be 2-byte aligned", x=X + 1, sr=NOSR)   # before the sr checks


def test_empty_bucket_is_a_no_op():
    from ina_amd import _lib
    for name in DEVICE:
        for kw in ({}, dict(x=None, base=None, q=None, ovf=None), dict(sr=NOSR), dict(e0=2), dict(x=X + 1)):
            rc, err = _rc(name, n=0, **kw)
            assert rc == _lib.INA_OK, (name, kw, err)                    # nothing is looked at


AMAX = [0.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 3e-30, 1e-9, 2.0 ** -20, 0.3, 0.99999994, 1.0, 1.0000001, 3.0,
        509.99, 510.0, 511.0, 32766.0, 32767.0, 65536.0, 2.0 ** 31, 1e12, 1e30]


def test_scale_for_sr_is_the_rule_in_exact_rationals():
    from ina_amd import _lib, sr
    lib = _lib.load()
    rng = np.random.default_rng(7)
    more = np.exp(rng.uniform(np.log(1e-44), np.log(1e30), 200)).astype(np.float32)
    for bits in (16, 32):
        for W in (1, 8, 64):
            for a in [np.float32(v) for v in AMAX] + list(more):
                k = ctypes.c_int(-999)
                assert lib.ina_scale_for_sr(float(a), W, bits, ctypes.byref(k)) == _lib.INA_OK
                assert k.value == sref.scale_for_sr(a, W, bits) == sr.scale_for(float(a), W, bits), (a, W, bits)
                n = ctypes.c_int(-999)                                   # never more room than to nearest leaves
                assert lib.ina_scale_for(float(a), W, bits, ctypes.byref(n)) == _lib.INA_OK and k.value <= n.value
    # one more quantum than ina_scale_for: at amax * 2^k + 1/2 on the nearest limit the two differ
    assert sr.scale_for(32766.0, 1, 16) == 0 and sr.scale_for(32766.5, 1, 16) == -1
    k = ctypes.c_int(0)
    for args, msg in (((1.0, 0, 16), b"W >= 1, bits 16 or 32"), ((1.0, 1, 8), b"W >= 1, bits 16 or 32"),
                      ((-1.0, 1, 16), b"absmax must be finite and >= 0"), ((float("nan"), 1, 16), b"absmax must be finite"),
                      ((float("inf"), 1, 32), b"absmax must be finite"), ((1.0, 32767, 16), b"too many workers for this width"),
                      ((1.0, 40000, 16), b"too many workers")):
        assert lib.ina_scale_for_sr(*args, ctypes.byref(k)) == _lib.INA_EINVAL and msg in lib.ina_last_error_string(), args
    assert lib.ina_scale_for_sr(1.0, 1, 16, None) == _lib.INA_EINVAL and b"null k_out" in lib.ina_last_error_string()
    assert lib.ina_scale_for_sr(1.0, 16383, 16, ctypes.byref(k)) == _lib.INA_OK          # 32767 / 16383 - 1 > 0


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind _req's device test are
    reached without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def test_python_calls_refuse_by_name_before_any_device_call():
    from ina_amd import sr
    calls = [(lambda x, **kw: sr.quantize(x, 9, 1, **kw), torch.int32),
             (lambda x, **kw: sr.quantize_i16(x, 9, 32, 1, **kw), torch.int16),
             (lambda x, **kw: sr.quantize_i16_wire(x, 9, 1, **kw), torch.int32)]
    for f, odt in calls:
        for dt in DTYPES:
            with pytest.raises(ValueError, match="x must be a device .* no CPU fallback"):
                f(torch.zeros(64, dtype=dt))
            dx = _FakeDev(torch.zeros(64, dtype=dt))
            for e0 in (1, 2, 7):
                with pytest.raises(ValueError, match=f"e0 must be a multiple of 4, got {e0}"):
                    f(dx, e0=e0)
            with pytest.raises(ValueError, match="out must be a device .* no CPU fallback"):
                f(dx, out=torch.zeros(64, dtype=odt))
            with pytest.raises(TypeError, match=f"out must be {odt}"):
                f(dx, out=_FakeDev(torch.zeros(64, dtype=torch.int64)))
            with pytest.raises(ValueError, match="out holds 63 elements, needs 64"):
                f(dx, out=_FakeDev(torch.zeros(63, dtype=odt)))
            with pytest.raises(ValueError, match="x must be contiguous"):
                f(_FakeDev(torch.zeros(128, dtype=dt)[::2]))
            with pytest.raises(ValueError, match=r"step must be in \[0, 2\^32\)"):
                f(dx, step=1 << 32)
            with pytest.raises(ValueError, match=r"sub must be in \[0, 2\^32\)"):
                f(dx, sub=-1)
            with pytest.raises(TypeError, match="step must be an int"):
                f(dx, step=1.5)
        with pytest.raises(TypeError, match="x must be torch.float32"):
            f(_FakeDev(torch.zeros(64, dtype=torch.float64)))
        with pytest.raises(TypeError, match="x must be a torch.Tensor"):
            f([0.0] * 64)
    dx = _FakeDev(torch.zeros(64))
    with pytest.raises(ValueError, match=r"seed must be in \[0, 2\^64\)"):
        sr.quantize(dx, 9, 1 << 64)
    for f in (lambda **kw: sr.quantize(dx, 9, 1, **kw), lambda **kw: sr.quantize_i16(dx, 9, 32, 1, **kw)):
        with pytest.raises(ValueError, match="base must be a device .* no CPU fallback"):
            f(base=torch.zeros(64))
        with pytest.raises(TypeError, match="base must be torch.float32"):
            f(base=_FakeDev(torch.zeros(64, dtype=torch.bfloat16)))
        with pytest.raises(ValueError, match="base and x differ in length"):
            f(base=_FakeDev(torch.zeros(63)))
    with pytest.raises(ValueError, match="V must be > 0"):
        sr.quantize_i16(dx, 9, 0, 1)
    out = _FakeDev(torch.zeros(64, dtype=torch.int16))
    with pytest.raises(TypeError, match="overflow must be torch.uint8"):
        sr.quantize_i16(dx, 9, 32, 1, out=out, overflow=_FakeDev(torch.zeros(2, dtype=torch.int8)))
    with pytest.raises(ValueError, match="overflow holds 1 elements, needs 2"):
        sr.quantize_i16(dx, 9, 32, 1, out=out, overflow=_FakeDev(torch.zeros(1, dtype=torch.uint8)))
    assert "base" not in inspect.signature(sr.quantize_i16_wire).parameters       # the wire has no base


def test_aggregator_arguments():
    from ina_amd.dist import RangeAggregator, ShardedAggregator
    cpu = torch.device("cpu")
    prm = inspect.signature(ShardedAggregator.__init__).parameters
    assert prm["rounding"].default == "nearest" and prm["seed"].default == 0
    assert "rounding" not in inspect.signature(RangeAggregator.__init__).parameters      # out of scope
    for bad in ("stochastic_rounding", "sr", None, True):
        with pytest.raises(ValueError, match="rounding must be 'nearest' or 'stochastic'"):
            ShardedAggregator(1000, k=9, device=cpu, rounding=bad)
    for wire in ("i16", "i32"):
        with pytest.raises(ValueError, match="rounding='stochastic'.*k='block'.*rounding='nearest'"):
            ShardedAggregator(1000, k="block", wire=wire, V=32, device=cpu, rounding="stochastic")
        with pytest.raises(ValueError, match="rounding='stochastic' and error_feedback=True exclude each other"):
            ShardedAggregator(1000, k=9, wire=wire, V=32, device=torch.device("cuda", 0), rounding="stochastic",
                              error_feedback=True)
        for seed in (-1, 1 << 64, 1.5, None):
            with pytest.raises(ValueError, match="seed must be an int"):
                ShardedAggregator(1000, k=9, wire=wire, V=32, device=cpu, rounding="stochastic", seed=seed)
        for coll in ("rs_ag", "a2a", "allreduce"):
            for dt in DTYPES:
                agg = ShardedAggregator(1000, k=9, wire=wire, V=32, device=cpu, collective=coll, out_dtype=dt,
                                        rounding="stochastic", seed=(1 << 64) - 1)
                assert agg.rounding == "stochastic" and agg.seed == (1 << 64) - 1 and agg.step == 0
                assert agg.full.dtype == dt and agg.residual is None
        agg = ShardedAggregator(1000, k=9, wire=wire, V=32, device=cpu)
        assert agg.rounding == "nearest" and agg.step == 0
        agg = ShardedAggregator(1000, k=9, wire=wire, V=32, device=cpu, rounding="stochastic")
        agg.step = 41
        assert agg.step == 41
        agg.step = (1 << 32) - 1
        for bad in (-1, 1 << 32, 2.0, None):
            with pytest.raises(ValueError, match="step must be an int"):
                agg.step = bad
        assert agg.step == (1 << 32) - 1
        with pytest.raises(ValueError, match="x must be a device .* no CPU fallback"):      # no CPU path: refused by name
            agg(torch.zeros(1000))
