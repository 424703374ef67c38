"""Stochastic rounding with per-block scales: the surface and the argument checks (include/ina_blk_sr.h,
ina_amd.blk_sr, dist.BlockStochasticAggregator, dist.BlockStochasticRangeAggregator), with no GPU.  The
header declares exactly the nine functions, refuses a lone include and reaches ina.h once, directly after
ina_reduce_sr.h's declarations; the names are in SIGNATURES_BLK_SR and in no other table or header,
exported and bound, each with its round-to-nearest sibling's arguments plus the ina_sr_t before the stream;
the checks come in the siblings' order with their messages before any device work (no pointer here is ever
dereferenced), then a null sr and e0 % 4, and n == 0 is a no-op; ina_amd.blk_sr and the aggregators refuse
by name, and the constructors that refused the pair before still do."""
import ctypes
import inspect
import os
import re

import pytest
import torch

X, X1, KB, OUT, OVF = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20          # addresses that are never touched
SCALES = "ina_block_scales_sr_x16"
Q32, QX32 = "ina_quantize_blk_sr_f32_i32", "ina_quantize_blk_sr_x16_i32"
W32, WX32 = "ina_quantize_blk_sr_f32_i16_wire", "ina_quantize_blk_sr_x16_i16_wire"
R32, R16 = "ina_quantize_reduce_blk_sr_f32_i32", "ina_quantize_reduce_blk_sr_f32_i16_sat"
RX32, RX16 = "ina_quantize_reduce_blk_sr_x16_i32", "ina_quantize_reduce_blk_sr_x16_i16_sat"
NAMES = (SCALES, Q32, QX32, W32, WX32, R32, R16, RX32, RX16)
ROUNDING = NAMES[1:]                       # the eight that draw random words
TYPED = (SCALES, QX32, WX32, RX32, RX16)
SINGLE, WIRES, REDUCES = (Q32, QX32, W32, WX32), (W32, WX32), (R32, R16, RX32, RX16)
SIBLING = {SCALES: ("SIGNATURES_BLK_X16", "ina_block_scales_x16"),
           Q32: ("SIGNATURES_BLK", "ina_quantize_blk_f32_i32"), QX32: ("SIGNATURES_BLK_X16", "ina_quantize_blk_x16_i32"),
           W32: ("SIGNATURES_SHARD_BLK", "ina_quantize_blk_f32_i16_wire"),
           WX32: ("SIGNATURES_SHARD_X16", "ina_quantize_blk_x16_i16_wire"),
           R32: ("SIGNATURES_BLK", "ina_quantize_reduce_blk_f32_i32"),
           R16: ("SIGNATURES_BLK", "ina_quantize_reduce_blk_f32_i16_sat"),
           RX32: ("SIGNATURES_BLK_X16", "ina_quantize_reduce_blk_x16_i32"),
           RX16: ("SIGNATURES_BLK_X16", "ina_quantize_reduce_blk_x16_i16_sat")}
BAD_TYPE = b"16-bit type must be INA_X16_BF16 (1) or INA_X16_F16 (2)"
NONE = "none"


def _calls(x=X, bufs=(X, X1), W=None, kblk=KB, out=OUT, ovf=OVF, n=64, V=32, t=1, mode=0, degree=2, bits=16,
           sr=None, e0=0):
    from ina_amd import _lib
    p = None if sr is NONE else ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0))
    arr = None if bufs is NONE else _lib.ptr_array(list(bufs))
    W = (0 if bufs is NONE else len(bufs)) if W is None else W
    return {SCALES: (arr, t, W, None, n, V, degree, bits, kblk, None),
            Q32: (x, kblk, V, out, n, p, None), QX32: (x, t, kblk, V, out, n, p, None),
            W32: (x, kblk, V, out, n, p, None), WX32: (x, t, kblk, V, out, n, p, None),
            R32: (arr, W, kblk, mode, degree, V, out, n, p, None),
            R16: (arr, W, kblk, mode, degree, V, out, n, ovf, p, None),
            RX32: (arr, t, W, kblk, mode, degree, V, out, n, p, None),
            RX16: (arr, t, W, kblk, mode, degree, V, out, n, ovf, p, None)}


def _rc(name, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    return getattr(lib, name)(*_calls(**kw)[name]), lib.ina_last_error_string()


def _einval(name, msg, **kw):
    from ina_amd import _lib
    rc, err = _rc(name, **kw)
    assert rc == _lib.INA_EINVAL and msg in err, (name, kw, rc, err)


def test_header_declares_the_nine_and_they_are_exported_and_bound():
    from ina_amd import _lib as L
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_blk_sr.h")).read()
    # included once: by ina_reduce_sr.h, as its last line before the guard closes, so that it reaches ina.h
    # directly after that header's declarations (ina.h itself names no block-scale header with an infix)
    texts = {h: open(os.path.join(inc, h)).read() for h in sorted(os.listdir(inc))}
    hits = [h for h, text in texts.items() for _ in re.findall(r'^#include "ina_blk_sr\.h"', text, flags=re.M)]
    assert hits == ["ina_reduce_sr.h"]
    rs = re.sub(r"/\*.*?\*/", "", texts["ina_reduce_sr.h"], flags=re.S)
    assert re.search(r'\)\s*;\s*#include "ina_blk_sr\.h"\s*#endif\s*$', rs)
    includes = re.findall(r'^#include "(\w+\.h)"', texts["ina.h"], flags=re.M)
    assert includes.count("ina_reduce_sr.h") == 1
    assert re.search(r"#ifndef INA_REDUCE_SR_H\n#error", src)                          # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == set(NAMES) == set(L.SIGNATURES_BLK_SR) == set(_calls()) and len(NAMES) == 9
    tables = [t for t in dir(L) if t.startswith("SIGNATURES") and t != "SIGNATURES_BLK_SR"]
    assert len(tables) >= 13
    for t in tables:
        assert not declared & set(getattr(L, t)), t
    for h, text in texts.items():                                                      # declared nowhere else
        if h == "ina_blk_sr.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = L.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == L.SIGNATURES_BLK_SR[name] and fn.restype is ctypes.c_int, name
    vp, srp = ctypes.c_void_p, ctypes.POINTER(L.SrParams)
    for name, (table, sib) in SIBLING.items():            # the sibling's arguments, sr before the stream
        want = list(getattr(L, table)[sib])
        assert L.SIGNATURES_BLK_SR[name] == (want if name == SCALES else want[:-1] + [srp, vp]), name
    head = src[: src.index("#ifndef INA_BLK_SR_H")]
    for word in ("Not here", "standalone int16 quantiser", "base", "error feedback", "PS combine", "chunks > 1",
                 "Per block", "Composition", "Integers", "Slices", "Layouts"):
        assert word in head, word
    # the two headers that refused the pair now point here
    for h in ("ina_sr.h", "ina_reduce_sr.h"):
        tail = texts[h][texts[h].index("Not here"):]
        assert "ina_blk_sr.h" in tail[: tail.index("*/")], h


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_blk_sr.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { ina_sr_t s = {1, 0, 0, 0}; return '
                 'ina_block_scales_sr_x16(0, INA_X16_BF16, 1, 0, 0, 8, 1, 16, 0, 0) + '
                 'ina_quantize_blk_sr_f32_i32(0, 0, 8, 0, 0, &s, 0) + '
                 'ina_quantize_blk_sr_x16_i32(0, INA_X16_F16, 0, 8, 0, 0, &s, 0) + '
                 'ina_quantize_blk_sr_f32_i16_wire(0, 0, 8, 0, 0, &s, 0) + '
                 'ina_quantize_blk_sr_x16_i16_wire(0, INA_X16_F16, 0, 8, 0, 0, &s, 0) + '
                 'ina_quantize_reduce_blk_sr_f32_i32(0, 1, 0, INA_BLK_AUTO, 1, 8, 0, 0, &s, 0) + '
                 'ina_quantize_reduce_blk_sr_f32_i16_sat(0, 1, 0, INA_BLK_GIVEN, 1, 8, 0, 0, 0, &s, 0) + '
                 'ina_quantize_reduce_blk_sr_x16_i32(0, INA_X16_BF16, 1, 0, INA_BLK_AUTO, 1, 8, 0, 0, &s, 0) + '
                 'ina_quantize_reduce_blk_sr_x16_i16_sat(0, INA_X16_BF16, 1, 0, INA_BLK_GIVEN, 1, 8, 0, 0, 0, &s, 0); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_checks_come_in_the_siblings_order_then_sr_then_e0():
    from ina_amd import _lib
    for t in (0, 3, -1):                                   # the type code first, before everything
        for name in TYPED:
            _einval(name, BAD_TYPE, t=t)
            _einval(name, BAD_TYPE, t=t, n=0)
            _einval(name, BAD_TYPE, t=t, V=0, mode=7, bufs=NONE, x=None, kblk=None, out=None, sr=NONE, e0=2)
    for V in (0, -1, -256):                                # then V, before the empty call's no-op
        for name in NAMES:
            _einval(name, b"V must be >= 1", V=V)
            _einval(name, b"V must be >= 1", V=V, n=0)
            _einval(name, b"V must be >= 1", V=V, mode=7, degree=0, bits=5, bufs=NONE, x=None, kblk=None, out=None,
                    sr=NONE, e0=2)
    for name in REDUCES:                                   # mode, then degree under AUTO, then kblk
        for mode in (-1, 2, 7):
            _einval(name, b"mode must be INA_BLK_GIVEN (0) or INA_BLK_AUTO (1)", mode=mode)
            _einval(name, b"mode must be", mode=mode, n=0, degree=0, kblk=None, bufs=NONE, out=None, sr=NONE)
        for degree in (0, -3):
            _einval(name, b"degree must be >= 1", mode=1, degree=degree)
            _einval(name, b"degree must be >= 1", mode=1, degree=degree, n=0, kblk=None, bufs=NONE, sr=NONE)
        _rc(name, mode=0, degree=0, n=0)                   # degree is ignored when the scales are given
        assert _rc(name, mode=0, degree=0, n=0)[0] == _lib.INA_OK
        _einval(name, b"null kblk", kblk=None)
        _einval(name, b"null kblk", kblk=None, n=0)
        _einval(name, b"null kblk", kblk=None, bufs=NONE, out=None, sr=NONE, e0=2)
    # the stochastic rule's degrees: (2^(bits-1) - 1) / degree - 1 <= 0 is refused, where nearest's - 1/2 is not yet
    for name in (R16, RX16):
        for degree in (32767, 40000, 65533):
            _einval(name, b"too many summands (degree) for this width", mode=1, degree=degree)
        rc, err = _rc(name, mode=1, degree=32766, sr=NONE)
        assert rc == _lib.INA_EINVAL and b"null sr" in err                 # accepted: the next refusal
    for name in (R32, RX32):
        _einval(name, b"too many summands (degree) for this width", mode=1, degree=2147483647)
    for degree, bits, msg in ((0, 16, b"degree must be >= 1"), (32767, 16, b"too many summands"), (2, 8, b"bits must be 16 or 32"),
                              (2147483647, 32, b"too many summands")):
        _einval(SCALES, msg, degree=degree, bits=bits)
        _einval(SCALES, msg, degree=degree, bits=bits, n=0, bufs=NONE, kblk=None)
    lib = _lib.load()
    arr = _lib.ptr_array([X, X1])
    assert lib.ina_block_scales_x16(arr, 1, 2, None, 64, 32, 32767, 16, None, None) == _lib.INA_EINVAL
    assert b"null kblk" in lib.ina_last_error_string()                     # the nearest sibling takes 32767: another rule
    # W, the worker buffers and out
    for name in REDUCES + (SCALES,):
        for kw in (dict(bufs=NONE, W=2), dict(W=0), dict(W=-1), dict(W=_lib.MAX_WORKERS + 1, bufs=(X,) * 65)):
            _einval(name, b"W must be in [1, 64]", **kw)
            _einval(name, b"W must be in [1, 64]", out=None, sr=NONE, e0=2, **kw)
        _einval(name, b"null worker buffer", bufs=(X, None))
        _einval(name, b"null worker buffer", bufs=(None, X1), out=None, sr=NONE)
    _einval(SCALES, b"null kblk", kblk=None)
    for name in REDUCES:
        _einval(name, b"null out", out=None)
        _einval(name, b"null out", out=None, sr=NONE, e0=2)                 # the sibling's checks first
        rc, err = _rc(name, bufs=(X,) * _lib.MAX_WORKERS, sr=NONE)          # W = 64 passes the limit
        assert rc == _lib.INA_EINVAL and b"null sr" in err
    for name in (RX32, RX16, SCALES):
        _einval(name, b"16-bit buffers must be 2-byte aligned", bufs=(X, X1 + 1))
        _einval(name, b"16-bit buffers must be 2-byte aligned", bufs=(X + 1, X1), out=None, sr=NONE)
    # the single-bucket calls: the sibling's null checks, the alignment of a 16-bit bucket
    for name in (Q32, QX32):
        for kw in (dict(x=None), dict(out=None), dict(kblk=None)):
            _einval(name, b"null pointer", **kw)
            _einval(name, b"null pointer", sr=NONE, e0=2, **kw)
    for name in WIRES:
        _einval(name, b"null kblk", kblk=None)
        _einval(name, b"null kblk", kblk=None, x=None, out=None, sr=NONE)
        for kw in (dict(x=None), dict(out=None)):
            _einval(name, b"null pointer", **kw)
            _einval(name, b"null pointer", sr=NONE, e0=2, **kw)
    for name in (QX32, WX32):
        _einval(name, b"16-bit buffers must be 2-byte aligned", x=X + 1)
        _einval(name, b"16-bit buffers must be 2-byte aligned", x=X + 1, sr=NONE, e0=2)
    # then the stochastic checks, for the eight that round
    for name in ROUNDING:
        _einval(name, b"null sr", sr=NONE)
        _einval(name, b"null sr", sr=NONE, ovf=None)
        for e0 in (1, 2, 3, 6, (1 << 40) + 1):
            _einval(name, b"e0 must be a multiple of 4", e0=e0)
            _einval(name, b"e0 must be a multiple of 4", e0=e0, mode=1, V=12)
    # each refusal above is the sibling's own, message for message
    for sib, args, msg in (("ina_quantize_blk_f32_i32", (X, None, 32, OUT, 64, None), b"null pointer"),
                           ("ina_quantize_blk_f32_i16_wire", (X, None, 32, OUT, 64, None), b"null kblk"),
                           ("ina_quantize_blk_x16_i16_wire", (X + 1, 1, KB, 32, OUT, 64, None), b"2-byte aligned"),
                           ("ina_quantize_reduce_blk_f32_i32", (arr, 2, KB, 0, 2, 32, None, 64, None), b"null out"),
                           ("ina_quantize_reduce_blk_x16_i16_sat", (arr, 1, 2, KB, 5, 2, 32, OUT, 64, OVF, None),
                            b"mode must be")):
        assert getattr(lib, sib)(*args) == _lib.INA_EINVAL and msg in lib.ina_last_error_string(), sib


def test_empty_bucket_is_a_no_op():
    from ina_amd import _lib
    for name in NAMES:
        for kw in ({}, dict(bufs=NONE, x=None, out=None, ovf=None), dict(sr=NONE), dict(e0=2), dict(W=0), dict(W=65),
                   dict(bufs=(X + 1, None), x=X + 1)):
            rc, err = _rc(name, n=0, **kw)
            assert rc == _lib.INA_OK, (name, kw, err)                       # nothing is looked at


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
    from ina_amd import blk_sr as bs
    kb = _FakeDev(torch.zeros(2, dtype=torch.int8))
    fused = [(lambda b, **kw: bs.quantize_reduce(b, 32, 1, **kw), torch.int32),
             (lambda b, **kw: bs.quantize_reduce_i16(b, 32, 1, **kw), torch.int16)]
    for f, odt in fused:
        for dt in DTYPES:
            with pytest.raises(ValueError, match=r"bufs\[0\] must be a device .* no CPU fallback"):
                f([torch.zeros(64, dtype=dt)] * 2)
            dx = _FakeDev(torch.zeros(64, dtype=dt))
            other = torch.bfloat16 if dt != torch.bfloat16 else torch.float16
            with pytest.raises(TypeError, match=r"all workers of one call share one dtype: bufs\[0\] is .*bufs\[1\] is"):
                f([dx, _FakeDev(torch.zeros(64, dtype=other))])
            with pytest.raises(ValueError, match="worker buffers differ in length"):
                f([dx, _FakeDev(torch.zeros(63, dtype=dt))])
            for e0 in (1, 2, 7):
                with pytest.raises(ValueError, match=f"e0 must be a multiple of 4, got {e0}"):
                    f([dx, dx], e0=e0)
            with pytest.raises(ValueError, match=r"step must be in \[0, 2\^32\)"):
                f([dx, dx], step=1 << 32)
            with pytest.raises(ValueError, match=r"sub must be in \[0, 2\^32\)"):
                f([dx, dx], sub=-1)
            with pytest.raises(TypeError, match="kblk must be torch.int8"):
                f([dx, dx], kblk=_FakeDev(torch.zeros(2, dtype=torch.uint8)))
            with pytest.raises(ValueError, match="kblk holds 1 elements, needs 2"):
                f([dx, dx], kblk=_FakeDev(torch.zeros(1, dtype=torch.int8)))
            with pytest.raises(ValueError, match="kblk must be a device"):
                f([dx, dx], kblk=torch.zeros(2, dtype=torch.int8))
            with pytest.raises(TypeError, match=f"out must be {odt}"):
                f([dx, dx], kblk=kb, out=_FakeDev(torch.zeros(64, dtype=torch.int64)))
            with pytest.raises(ValueError, match="out holds 63 elements, needs 64"):
                f([dx, dx], kblk=kb, out=_FakeDev(torch.zeros(63, dtype=odt)))
            for degree in (0, -1):
                with pytest.raises(ValueError, match=f"degree {degree} cannot be summed"):
                    f([dx, dx], degree=degree)
        with pytest.raises(TypeError, match=r"bufs\[0\] must be torch.float32"):
            f([_FakeDev(torch.zeros(64, dtype=torch.float64))])
        with pytest.raises(ValueError, match="need 1..64 worker buffers, got 65"):
            f([_FakeDev(torch.zeros(64))] * 65)
    dx = _FakeDev(torch.zeros(64))
    with pytest.raises(ValueError, match="degree 32767 cannot be summed at 16 bits"):      # the stochastic rule
        bs.quantize_reduce_i16([dx], 32, 1, degree=32767)
    with pytest.raises(ValueError, match="degree 32767 cannot be summed at 16 bits"):
        bs.block_scales([dx], 32, bits=16, degree=32767)
    with pytest.raises(ValueError, match="bits must be 16 or 32"):
        bs.block_scales([dx], 32, bits=8)
    with pytest.raises(ValueError, match=r"seed must be in \[0, 2\^64\)"):
        bs.quantize_reduce([dx], 32, 1 << 64)
    with pytest.raises(TypeError, match="seed must be an int"):
        bs.quantize(dx, kb, 32, None)
    out = _FakeDev(torch.zeros(64, dtype=torch.int16))
    with pytest.raises(TypeError, match="overflow must be torch.uint8"):
        bs.quantize_reduce_i16([dx], 32, 1, kblk=kb, out=out, overflow=_FakeDev(torch.zeros(2, dtype=torch.int8)))
    with pytest.raises(ValueError, match="overflow holds 1 elements, needs 2"):
        bs.quantize_reduce_i16([dx], 32, 1, kblk=kb, out=out, overflow=_FakeDev(torch.zeros(1, dtype=torch.uint8)))
    for f in (bs.quantize, bs.quantize_i16_wire):
        for dt in DTYPES:
            x = _FakeDev(torch.zeros(64, dtype=dt))
            with pytest.raises(ValueError, match="x must be a device .* no CPU fallback"):
                f(torch.zeros(64, dtype=dt), kb, 32, 1)
            with pytest.raises(ValueError, match="V must be >= 1"):
                f(x, kb, 0, 1)
            with pytest.raises((TypeError, ValueError), match="kblk must be"):
                f(x, None, 32, 1)
            with pytest.raises(ValueError, match="kblk holds 2 elements, needs 4"):
                f(x, kb, 16, 1)
            with pytest.raises(ValueError, match="e0 must be a multiple of 4, got 6"):
                f(x, kb, 32, 1, e0=6)
            with pytest.raises(TypeError, match="out must be torch.int32"):
                f(x, kb, 32, 1, out=_FakeDev(torch.zeros(64, dtype=torch.int16)))
        with pytest.raises(TypeError, match="x must be torch.float32"):
            f(_FakeDev(torch.zeros(64, dtype=torch.float64)), kb, 32, 1)
    for f in (bs.quantize, bs.quantize_i16_wire, bs.quantize_reduce, bs.quantize_reduce_i16):   # no base
        prm = inspect.signature(f).parameters
        assert "base" not in prm and [prm[p].default for p in ("step", "sub", "e0")] == [0, 0, 0]
    assert list(inspect.signature(bs.quantize_reduce).parameters) == [
        "bufs", "V", "seed", "kblk", "degree", "step", "sub", "e0", "out", "kblk_out"]
    assert list(inspect.signature(bs.quantize_reduce_i16).parameters) == [
        "bufs", "V", "seed", "kblk", "degree", "step", "sub", "e0", "out", "overflow", "kblk_out"]
    assert not hasattr(bs, "quantize_i16")                 # the W = 1 fused call is that operation


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


def test_aggregator_arguments():
    from ina_amd import dist
    from ina_amd.dist import (BlockStochasticAggregator, BlockStochasticRangeAggregator, RangeAggregator,
                              ShardedAggregator, StochasticRangeAggregator)
    cpu = torch.device("cpu")
    assert issubclass(BlockStochasticAggregator, ShardedAggregator)
    assert issubclass(BlockStochasticRangeAggregator, RangeAggregator)
    prm = inspect.signature(BlockStochasticAggregator.__init__).parameters
    assert not {"k", "chunks", "error_feedback", "rounding"} & set(prm) and prm["seed"].default == 0
    assert {"wire", "V", "collective", "out_dtype", "align", "group", "device"} <= set(prm)
    prm = inspect.signature(BlockStochasticRangeAggregator.__init__).parameters
    base = inspect.signature(RangeAggregator.__init__).parameters
    assert list(prm) == [p for p in base if p != "k"] + ["seed"] and prm["seed"].default == 0
    for cls in (BlockStochasticAggregator, BlockStochasticRangeAggregator):
        for seed in (-1, 1 << 64, 1.5, None, True):
            with pytest.raises(ValueError, match="seed must be an int"):
                cls(1000, device=cpu, seed=seed)
        with pytest.raises(ValueError, match="wire must be 'i32' or 'i16'"):          # the base classes' refusals stay
            cls(1000, wire="i8", device=cpu)
        with pytest.raises(ValueError, match="V must be > 0"):
            cls(1000, V=0, device=cpu)
        with pytest.raises(ValueError, match="out_dtype must be"):
            cls(1000, out_dtype=torch.float64, device=cpu)
        for wire in ("i32", "i16"):
            for dt in DTYPES:
                agg = cls(1000, wire=wire, V=32, device=cpu, out_dtype=dt, seed=(1 << 64) - 1)
                assert agg.rounding == "stochastic" and agg.seed == (1 << 64) - 1 and agg.step == 0 and agg.blk
                assert agg.k == "block" and agg.full.dtype == dt and agg.kblk.numel() == 32 and agg.scale_bytes == 0
            agg = cls(1000, wire=wire, V=32, device=cpu)
            agg.step = 41
            assert agg.step == 41
            agg.step = (1 << 32) - 1
            for bad in (-1, 1 << 32, 2.0, None, True):
                with pytest.raises(ValueError, match="step must be an int"):
                    agg.step = bad
            arg = torch.zeros(1000) if cls is BlockStochasticAggregator else [torch.zeros(1000)] * 2
            with pytest.raises(ValueError, match="must be a device .* no CPU fallback"):   # no CPU path
                agg(arg)
            assert agg.step == (1 << 32) - 1                                              # a refused call is no step
    with pytest.raises(ValueError, match="collective must be"):
        BlockStochasticAggregator(1000, collective="ring", device=cpu)
    for coll in ("rs_ag", "a2a", "allreduce"):
        agg = BlockStochasticAggregator(1000, collective=coll, wire="i16", V=32, device=cpu)
        assert agg.stochastic and agg.chunks == 1 and not agg.error_feedback and agg.residual is None
    with pytest.raises(ValueError, match="bucket size changed"):
        BlockStochasticAggregator(1000, device=cpu)(torch.zeros(999))
    with pytest.raises(ValueError, match="every worker slice must hold this rank's 1000 values"):
        BlockStochasticRangeAggregator(1000, device=cpu)([torch.zeros(999)])
    real = dist.dist
    try:                                   # a range that starts off a multiple of 4 cannot be an e0
        dist.dist = _Rank1
        with pytest.raises(ValueError, match="range starts at 501, not a multiple of 4"):
            BlockStochasticRangeAggregator(1001, V=1, device=cpu, align=1)
        agg = BlockStochasticRangeAggregator(1001, V=4, device=cpu, align=4)
        assert agg.range == (504, 1001)
        assert BlockStochasticAggregator(1001, V=32, device=cpu).scale_bytes == 32        # the MIN of the scales
    finally:
        dist.dist = real
    # the constructors that refused the pair before still do, by name
    with pytest.raises(ValueError, match="rounding='stochastic' takes a global integer k.*k='block'"):
        ShardedAggregator(1000, k="block", rounding="stochastic", device=cpu)
    with pytest.raises(ValueError, match="StochasticRangeAggregator takes a global integer k.*k='block'"):
        StochasticRangeAggregator(1000, k="block", device=cpu)
    with pytest.raises(ValueError, match="exclude each other"):
        ShardedAggregator(1000, rounding="stochastic", error_feedback=True, device=cpu)
    from ina_amd import sr
    with pytest.raises(ValueError, match="block scales are not combined with stochastic rounding on the fused"):
        sr.quantize_reduce([_FakeDev(torch.zeros(64))], _FakeDev(torch.zeros(2, dtype=torch.int8)), 1)
