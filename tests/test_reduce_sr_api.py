"""Stochastic rounding in the fused quantise + reduce calls: the surface and the argument checks
(include/ina_reduce_sr.h, ina_amd.sr, dist.StochasticRangeAggregator), with no GPU.  The header declares
exactly the four functions, refuses a lone include and is included by ina.h once, directly after
ina_pkt_sr.h; the names are in SIGNATURES_REDUCE_SR and in no other table or header, exported and bound,
each with its round-to-nearest sibling's arguments plus the ina_sr_t before the stream; the checks come in
the siblings' order with their messages before any device work (every pointer here is never
dereferenced), then a null sr and e0 % 4, and n == 0 is a no-op; ina_amd.sr and the aggregator refuse by
name."""
import ctypes
import inspect
import os
import re

import pytest
import torch

# addresses that are never touched
B0, B1, OUT, OVF = 1 << 20, 2 << 20, 3 << 20, 4 << 20
F32, F16S, X32, X16S = ("ina_quantize_reduce_sr_f32_i32", "ina_quantize_reduce_sr_f32_i16_sat",
                        "ina_quantize_reduce_sr_x16_i32", "ina_quantize_reduce_sr_x16_i16_sat")
NAMES = (F32, F16S, X32, X16S)
TYPED, SLOTTED = (X32, X16S), (F16S, X16S)
SIBLING = {F32: ("SIGNATURES", "ina_quantize_reduce_f32_i32"), F16S: ("SIGNATURES", "ina_quantize_reduce_f32_i16_sat"),
           X32: ("SIGNATURES_X16", "ina_quantize_reduce_x16_i32"),
           X16S: ("SIGNATURES_X16", "ina_quantize_reduce_x16_i16_sat")}
BAD_TYPE = b"16-bit type must be INA_X16_BF16 (1) or INA_X16_F16 (2)"
NONE = "none"


def _calls(bufs=(B0, B1), W=None, out=OUT, ovf=OVF, n=64, k=9, V=32, t=1, sr=None, e0=0):
    from ina_amd import _lib
    p = None if sr is NONE else ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0))
    arr = None if bufs is NONE else _lib.ptr_array(list(bufs))
    W = (0 if bufs is NONE else len(bufs)) if W is None else W
    return {F32: (arr, W, out, n, k, p, None), F16S: (arr, W, out, n, k, V, ovf, p, None),
            X32: (arr, t, W, out, n, k, p, None), X16S: (arr, t, W, out, n, k, V, ovf, p, None)}


def _rc(name, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    return getattr(lib, name)(*_calls(**kw)[name]), lib.ina_last_error_string()


def _einval(name, msg, **kw):
    from ina_amd import _lib
    rc, err = _rc(name, **kw)
    assert rc == _lib.INA_EINVAL and msg in err, (name, kw, rc, err)


def test_header_declares_the_four_and_they_are_exported_and_bound():
    from ina_amd import _lib as L
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_reduce_sr.h")).read()
    includes = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(inc, "ina.h")).read(), flags=re.M)
    assert includes.count("ina_reduce_sr.h") == 1
    assert includes.index("ina_reduce_sr.h") == includes.index("ina_pkt_sr.h") + 1     # directly after
    assert re.search(r"#ifndef INA_PKT_SR_H\n#error", src)                             # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == set(NAMES) == set(L.SIGNATURES_REDUCE_SR) == set(_calls())
    tables = [t for t in dir(L) if t.startswith("SIGNATURES") and t != "SIGNATURES_REDUCE_SR"]
    assert len(tables) >= 12
    for t in tables:
        assert not declared & set(getattr(L, t)), t
    for h in sorted(os.listdir(inc)):                                                  # declared nowhere else
        if h == "ina_reduce_sr.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = L.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == L.SIGNATURES_REDUCE_SR[name] and fn.restype is ctypes.c_int, name
    vp, srp = ctypes.c_void_p, ctypes.POINTER(L.SrParams)
    for name, (table, sib) in SIBLING.items():                       # the sibling's arguments, sr before the stream
        want = list(getattr(L, table)[sib])
        assert L.SIGNATURES_REDUCE_SR[name] == want[:-1] + [srp, vp], name
    # the header says what it leaves out
    head = src[: src.index("#ifndef INA_REDUCE_SR_H")]
    for word in ("Not here", "block scales", "base", "error feedback", "PS combine"):
        assert word in head, word


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_reduce_sr.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { ina_sr_t s = {1, 0, 0, 0}; return '
                 'ina_quantize_reduce_sr_f32_i32(0, 1, 0, 0, 1, &s, 0) + '
                 'ina_quantize_reduce_sr_f32_i16_sat(0, 1, 0, 0, 1, 8, 0, &s, 0) + '
                 'ina_quantize_reduce_sr_x16_i32(0, INA_X16_BF16, 1, 0, 0, 1, &s, 0) + '
                 'ina_quantize_reduce_sr_x16_i16_sat(0, INA_X16_F16, 1, 0, 0, 1, 8, 0, &s, 0); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_checks_come_in_the_siblings_order_then_sr_then_e0():
    from ina_amd import _lib
    for t in (0, 3, -1):                                   # the type code first, before everything
        for name in TYPED:
            _einval(name, BAD_TYPE, t=t)
            _einval(name, BAD_TYPE, t=t, n=0)
            _einval(name, BAD_TYPE, t=t, k=500, V=0, bufs=NONE, out=None, sr=NONE, e0=2)
    for k in (-127, 128, 500):
        for name in NAMES:
            _einval(name, b"k out of range [-126,127]", k=k)
            _einval(name, b"k out of range", k=k, n=0)     # before the empty call's no-op
            _einval(name, b"k out of range", k=k, V=0, bufs=NONE, out=None, sr=NONE)
    for V in (0, -1):
        for name in SLOTTED:
            _einval(name, b"V must be > 0", V=V)
            _einval(name, b"V must be > 0", V=V, n=0)
            _einval(name, b"V must be > 0", V=V, bufs=NONE, sr=NONE, e0=2)
    for name in NAMES:
        for kw in (dict(bufs=NONE, W=2), dict(W=0), dict(W=-1), dict(W=_lib.MAX_WORKERS + 1, bufs=(B0,) * 65)):
            _einval(name, b"W must be in [1, 64]", **kw)
            _einval(name, b"W must be in [1, 64]", out=None, sr=NONE, e0=2, **kw)
        _einval(name, b"null worker buffer", bufs=(B0, None))
        _einval(name, b"null worker buffer", bufs=(None, B1), out=None, sr=NONE)
        _einval(name, b"null out", out=None)
        _einval(name, b"null out", out=None, sr=NONE, e0=2)               # the sibling's checks first
        _einval(name, b"null sr", sr=NONE)
        _einval(name, b"null sr", sr=NONE, ovf=None)
        for e0 in (1, 2, 3, 6, (1 << 40) + 1):
            _einval(name, b"e0 must be a multiple of 4", e0=e0)
        rc, err = _rc(name, bufs=(B0,) * _lib.MAX_WORKERS, sr=NONE)       # W = 64 passes the limit: the next refusal
        assert rc == _lib.INA_EINVAL and b"null sr" in err
    for name in TYPED:
        _einval(name, b"16-bit buffers must be 2-byte aligned", bufs=(B0, B1 + 1))
        _einval(name, b"16-bit buffers must be 2-byte aligned", bufs=(B0 + 1, B1), out=None, sr=NONE)   # before out, sr
        _einval(name, b"null worker buffer", bufs=(None, B1 + 1))         # worker by worker, as the sibling
    # each is the sibling's own refusal, message for message
    lib = _lib.load()
    arr = _lib.ptr_array([B0, None])
    for sib, args in (("ina_quantize_reduce_f32_i32", (arr, 2, OUT, 64, 9, None)),
                      ("ina_quantize_reduce_f32_i16_sat", (arr, 2, OUT, 64, 9, 32, OVF, None)),
                      ("ina_quantize_reduce_x16_i32", (arr, 1, 2, OUT, 64, 9, None)),
                      ("ina_quantize_reduce_x16_i16_sat", (arr, 1, 2, OUT, 64, 9, 32, OVF, None))):
        assert getattr(lib, sib)(*args) == _lib.INA_EINVAL and b"null worker buffer" in lib.ina_last_error_string()


def test_empty_bucket_is_a_no_op():
    from ina_amd import _lib
    for name in NAMES:
        for kw in ({}, dict(bufs=NONE, out=None, ovf=None), dict(sr=NONE), dict(e0=2), dict(W=0), dict(W=65),
                   dict(bufs=(B0 + 1, None))):
            rc, err = _rc(name, n=0, **kw)
            assert rc == _lib.INA_OK, (name, kw, err)                    # nothing is looked at


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind the device test are reached
    without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def test_python_calls_refuse_by_name_before_any_device_call():
    from ina_amd import sr
    calls = [(lambda b, k=9, **kw: sr.quantize_reduce(b, k, 1, **kw), torch.int32),
             (lambda b, k=9, **kw: sr.quantize_reduce_i16(b, k, 32, 1, **kw), torch.int16)]
    for f, odt in calls:
        for dt in DTYPES:
            with pytest.raises(ValueError, match=r"bufs\[0\] must be a device .* no CPU fallback"):
                f([torch.zeros(64, dtype=dt)] * 2)
            dx = _FakeDev(torch.zeros(64, dtype=dt))
            other = torch.bfloat16 if dt != torch.bfloat16 else torch.float16
            with pytest.raises(TypeError, match=r"all workers of one call share one dtype: bufs\[0\] is .*bufs\[1\] is"):
                f([dx, _FakeDev(torch.zeros(64, dtype=other))])
            with pytest.raises(ValueError, match="worker buffers differ in length"):
                f([dx, _FakeDev(torch.zeros(63, dtype=dt))])
            with pytest.raises(ValueError, match=r"bufs\[1\] must be contiguous"):
                f([dx, _FakeDev(torch.zeros(128, dtype=dt)[::2])])
            for e0 in (1, 2, 7):
                with pytest.raises(ValueError, match=f"e0 must be a multiple of 4, got {e0}"):
                    f([dx, dx], e0=e0)
            with pytest.raises(ValueError, match=r"e0 must be in \[0, 2\^64\)"):
                f([dx, dx], e0=-4)
            with pytest.raises(ValueError, match=r"step must be in \[0, 2\^32\)"):
                f([dx, dx], step=1 << 32)
            with pytest.raises(ValueError, match=r"sub must be in \[0, 2\^32\)"):
                f([dx, dx], sub=-1)
            with pytest.raises(TypeError, match="step must be an int"):
                f([dx, dx], step=1.5)
            with pytest.raises(ValueError, match="out must be a device .* no CPU fallback"):
                f([dx, dx], out=torch.zeros(64, dtype=odt))
            with pytest.raises(TypeError, match=f"out must be {odt}"):
                f([dx, dx], out=_FakeDev(torch.zeros(64, dtype=torch.int64)))
            with pytest.raises(ValueError, match="out holds 63 elements, needs 64"):
                f([dx, dx], out=_FakeDev(torch.zeros(63, dtype=odt)))
            # block scales: an int8 tensor of scales, None (computed) and "block" are refused as such
            for k in (_FakeDev(torch.zeros(2, dtype=torch.int8)), None, "block"):
                with pytest.raises(ValueError, match="block scales are not combined with stochastic rounding on the fused"):
                    f([dx, dx], k=k)
            with pytest.raises(TypeError, match="k must be an int"):
                f([dx, dx], k=9.0)
        with pytest.raises(TypeError, match=r"bufs\[0\] must be torch.float32"):
            f([_FakeDev(torch.zeros(64, dtype=torch.float64))])
        with pytest.raises(ValueError, match="need 1..64 worker buffers, got 65"):
            f([_FakeDev(torch.zeros(64))] * 65)
        with pytest.raises(ValueError, match="need 1..64 worker buffers, got 0"):
            f([])
    dx = _FakeDev(torch.zeros(64))
    with pytest.raises(ValueError, match=r"seed must be in \[0, 2\^64\)"):
        sr.quantize_reduce([dx], 9, 1 << 64)
    with pytest.raises(TypeError, match="seed must be an int"):
        sr.quantize_reduce_i16([dx], 9, 32, None)
    for V in (0, -8):
        with pytest.raises(ValueError, match="V must be > 0"):
            sr.quantize_reduce_i16([dx], 9, V, 1)
    out = _FakeDev(torch.zeros(64, dtype=torch.int16))
    with pytest.raises(TypeError, match="overflow must be torch.uint8"):
        sr.quantize_reduce_i16([dx], 9, 32, 1, out=out, overflow=_FakeDev(torch.zeros(2, dtype=torch.int8)))
    with pytest.raises(ValueError, match="overflow holds 1 elements, needs 2"):
        sr.quantize_reduce_i16([dx], 9, 32, 1, out=out, overflow=_FakeDev(torch.zeros(1, dtype=torch.uint8)))
    for f in (sr.quantize_reduce, sr.quantize_reduce_i16):                 # no base, as in the siblings
        prm = inspect.signature(f).parameters
        assert "base" not in prm and [prm[p].default for p in ("step", "sub", "e0")] == [0, 0, 0]


def test_aggregator_arguments():
    from ina_amd import dist
    from ina_amd.dist import RangeAggregator, StochasticRangeAggregator
    cpu = torch.device("cpu")
    assert issubclass(StochasticRangeAggregator, RangeAggregator)
    base = inspect.signature(RangeAggregator.__init__).parameters
    assert "rounding" not in base and "seed" not in base                  # RangeAggregator keeps its arguments
    prm = inspect.signature(StochasticRangeAggregator.__init__).parameters
    assert list(prm) == list(base) + ["seed"] and prm["seed"].default == 0
    assert all(prm[p].default == base[p].default for p in base)
    for k in ("block", None):
        for wire in ("i32", "i16"):
            with pytest.raises(ValueError, match="StochasticRangeAggregator takes a global integer k.*k='block'"):
                StochasticRangeAggregator(1000, k=k, wire=wire, V=32, device=cpu)
    for seed in (-1, 1 << 64, 1.5, None, True):
        with pytest.raises(ValueError, match="seed must be an int"):
            StochasticRangeAggregator(1000, k=9, device=cpu, seed=seed)
    with pytest.raises(ValueError, match="wire must be 'i32' or 'i16'"):      # RangeAggregator's own refusals stay
        StochasticRangeAggregator(1000, k=9, wire="i8", device=cpu)
    for wire in ("i32", "i16"):
        for dt in DTYPES:
            agg = StochasticRangeAggregator(1000, k=9, wire=wire, V=32, device=cpu, out_dtype=dt, seed=(1 << 64) - 1)
            assert agg.rounding == "stochastic" and agg.seed == (1 << 64) - 1 and agg.step == 0
            assert agg.full.dtype == dt and agg.range == (0, 1000) and not agg.blk
        agg = StochasticRangeAggregator(1000, k=9, wire=wire, V=32, device=cpu)
        agg.step = 41
        assert agg.step == 41
        agg.step = (1 << 32) - 1
        for bad in (-1, 1 << 32, 2.0, None, True):
            with pytest.raises(ValueError, match="step must be an int"):
                agg.step = bad
        assert agg.step == (1 << 32) - 1
        with pytest.raises(ValueError, match=r"bufs\[0\] must be a device .* no CPU fallback"):   # no CPU path
            agg([torch.zeros(1000)] * 2)
        assert agg.step == (1 << 32) - 1                                  # a refused call is no step
        with pytest.raises(ValueError, match="every worker slice must hold this rank's 1000 values"):
            agg([torch.zeros(999)])
    # a range that starts off a multiple of 4 cannot be an e0: refused when the plan is made

    class _Rank1:
        @staticmethod
        def is_initialized():
            return True

        @staticmethod
        def get_world_size(group=None):
            return 2

        @staticmethod
        def get_rank(group=None):
            return 1

    real = dist.dist
    try:
        dist.dist = _Rank1
        with pytest.raises(ValueError, match="range starts at 501, not a multiple of 4"):
            StochasticRangeAggregator(1001, k=9, device=cpu, align=1)
        agg = StochasticRangeAggregator(1001, k=9, device=cpu, align=4)
        assert agg.range == (504, 1001)
    finally:
        dist.dist = real
