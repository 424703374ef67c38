"""Per-block scales for bf16 / fp16 buckets: the surface and the argument checks (include/ina_x16_blk.h,
ina_amd.blk), with no GPU.  The header declares exactly the eight functions, refuses a lone include and
is the last one ina.h includes; the names are in SIGNATURES_BLK_X16 and in no other table, exported and
bound; a bad type code, bad V / W / degree / bits / mode, null scales and null buffers come back as
INA_EINVAL with the fp32 siblings' messages before any device work and n == 0 is a no-op; ina_amd.blk
refuses CPU tensors, float64, mixed dtypes, a 16-bit base and short or non-int8 scales, and hands fp32
buckets to the ops functions."""
import ctypes
import os
import re

import pytest
import torch

FAKE = 1 << 20            # an aligned address that is never touched

NAMES = {
    "ina_block_scales_x16", "ina_quantize_blk_x16_i32", "ina_quantize_blk_x16_i16_sat",
    "ina_quantize_reduce_blk_x16_i32", "ina_quantize_reduce_blk_x16_i16_sat",
    "ina_dequantize_blk_i32_x16", "ina_dequantize_blk_i16_x16", "ina_quantize_pack_nga_multi_split_blk_x16",
}
PACK = "ina_quantize_pack_nga_multi_split_blk_x16"
REDUCES = ("ina_quantize_reduce_blk_x16_i32", "ina_quantize_reduce_blk_x16_i16_sat")
MULTI = ("ina_block_scales_x16",) + REDUCES + (PACK,)          # the calls that take W buffers


def _calls(xtype=1, n=64, V=32, W=2, degree=2, bits=32, mode=1, kblk=FAKE, bufs=FAKE):
    """name -> argument tuple over fake aligned pointers, for every entry point."""
    from ina_amd import _lib
    nw = max(W, 1)
    arr = _lib.ptr_array([bufs] * nw)
    rows = _lib.ptr_array([FAKE] * nw)
    prm = (_lib.NgaParams * nw)(*[_lib.NgaParams(1, 2, 0, 1, 0, 1, 16384, V)] * nw)
    return {
        "ina_block_scales_x16": (arr, xtype, W, None, n, V, degree, bits, kblk, None),
        "ina_quantize_blk_x16_i32": (bufs, xtype, kblk, V, FAKE, n, None),
        "ina_quantize_blk_x16_i16_sat": (bufs, xtype, kblk, V, FAKE, n, None, None),
        "ina_quantize_reduce_blk_x16_i32": (arr, xtype, W, kblk, mode, degree, V, FAKE, n, None),
        "ina_quantize_reduce_blk_x16_i16_sat": (arr, xtype, W, kblk, mode, degree, V, FAKE, n, None, None),
        "ina_dequantize_blk_i32_x16": (FAKE, kblk, V, FAKE, xtype, n, None),
        "ina_dequantize_blk_i16_x16": (FAKE, kblk, V, FAKE, xtype, n, None),
        PACK: (arr, xtype, W, None, n, kblk, mode, degree, prm, rows, rows, None, None),
    }


def _einval(name, msg, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    assert getattr(lib, name)(*_calls(**kw)[name]) == _lib.INA_EINVAL, (name, kw)
    assert msg in lib.ina_last_error_string(), (name, kw, lib.ina_last_error_string())


def test_header_declares_the_eight_and_they_are_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_x16_blk.h")).read()
    ina_h = open(os.path.join(inc, "ina.h")).read()
    includes = re.findall(r'^#include "(\w+\.h)"', ina_h, flags=re.M)
    assert includes[-1] == "ina_x16_blk.h" and includes.count("ina_x16_blk.h") == 1       # included last
    assert re.search(r"#ifndef INA_\w+_H\n#error", src)                                    # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == NAMES == set(_lib.SIGNATURES_BLK_X16) == set(_calls())
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16) | set(_lib.SIGNATURES_BLK) |
              set(_lib.SIGNATURES_PKT_BLK) | set(_lib.SIGNATURES_SWITCH_BLK) | set(_lib.SIGNATURES_SHARD_BLK))
    assert not declared & others
    for h in sorted(os.listdir(inc)):                                                      # declared nowhere else
        if h == "ina_x16_blk.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SIGNATURES_BLK_X16[name] and fn.restype is ctypes.c_int, name
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    # (xs, xtype, W, base, n, V, degree, bits, kblk_out, stream) and (s, kblk, V, y, ytype, n, stream)
    assert _lib.SIGNATURES_BLK_X16["ina_block_scales_x16"] == [vp, i, i, vp, sz, i, i, i, vp, vp]
    assert _lib.SIGNATURES_BLK_X16["ina_dequantize_blk_i32_x16"] == [vp, vp, i, vp, i, sz, vp]
    assert lib.ina_version() == b"ina-mi355x 0.2 (gfx950)"


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_x16_blk.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { return ina_dequantize_blk_i16_x16(0, 0, 1, 0, INA_X16_BF16, 0, 0); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("xtype", [0, 3])
def test_bad_type_code_is_einval(xtype):
    for name in NAMES:
        _einval(name, b"INA_X16_BF16 (1) or INA_X16_F16 (2)", xtype=xtype)
        _einval(name, b"INA_X16_BF16", xtype=xtype, n=0)                # before the empty call's no-op


@pytest.mark.parametrize("xtype", [1, 2])
@pytest.mark.parametrize("V", [0, -1, -256])
def test_bad_v_is_einval(xtype, V):
    for name in NAMES - {PACK}:
        _einval(name, b"V must be", xtype=xtype, V=V)
    _einval(PACK, b"V a multiple of 4", xtype=xtype, V=V)      # the split rows' rule, as in the fp32 pack


@pytest.mark.parametrize("xtype", [1, 2])
@pytest.mark.parametrize("W", [0, -1, 65])
def test_bad_w_is_einval(xtype, W):
    for name in MULTI:
        _einval(name, b"W in [1, 64]" if name == PACK else b"W must be", xtype=xtype, W=W)


@pytest.mark.parametrize("xtype", [1, 2])
def test_bad_degree_bits_and_mode_are_einval(xtype):
    for degree in (0, -3):
        for name in MULTI:
            _einval(name, b"degree", xtype=xtype, degree=degree)
    # too many summands for 16 bits: 32767 / degree - 1/2 <= 0 (ina_scale_for's rule)
    for degree in (65534, 70000):
        _einval("ina_block_scales_x16", b"degree", xtype=xtype, degree=degree, bits=16)
        _einval("ina_quantize_reduce_blk_x16_i16_sat", b"degree", xtype=xtype, degree=degree)
    for bits in (0, 8, 31, 64):
        _einval("ina_block_scales_x16", b"bits", xtype=xtype, bits=bits)
    for mode in (2, -1, 7):
        for name in REDUCES + (PACK,):
            _einval(name, b"mode", xtype=xtype, mode=mode)


@pytest.mark.parametrize("xtype", [1, 2])
def test_null_scales_and_buffers_are_einval(xtype):
    from ina_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        for mode in (0, 1):
            _einval(name, b"null", xtype=xtype, kblk=None, mode=mode)
    for name in NAMES - {"ina_dequantize_blk_i32_x16", "ina_dequantize_blk_i16_x16"}:
        _einval(name, b"null", xtype=xtype, bufs=None)
    assert lib.ina_dequantize_blk_i32_x16(None, FAKE, 32, FAKE, xtype, 64, None) == _lib.INA_EINVAL
    assert lib.ina_dequantize_blk_i16_x16(FAKE, FAKE, 32, None, xtype, 64, None) == _lib.INA_EINVAL
    # an odd address cannot hold 16-bit values
    _einval("ina_quantize_blk_x16_i32", b"2-byte aligned", xtype=xtype, bufs=FAKE + 1)
    assert lib.ina_dequantize_blk_i32_x16(FAKE, FAKE, 32, FAKE + 1, xtype, 64, None) == _lib.INA_EINVAL
    assert b"2-byte aligned" in lib.ina_last_error_string()


@pytest.mark.parametrize("xtype", [1, 2])
def test_empty_bucket_is_a_no_op(xtype):
    from ina_amd import _lib
    lib = _lib.load()
    for name, args in _calls(xtype=xtype, n=0).items():
        assert getattr(lib, name)(*args) == _lib.INA_OK, name
    for name, args in _calls(xtype=xtype, n=0, kblk=None, bufs=None).items():      # nothing is looked at
        if name in REDUCES:
            continue                                                               # mode / kblk are checked first
        assert getattr(lib, name)(*args) == _lib.INA_OK, name


def _blk_calls(kb):
    from ina_amd import blk
    return [
        lambda t, **kw: blk.block_scales([t, t], 32, **kw),
        lambda t, **kw: blk.quantize(t, kb, 32),
        lambda t, **kw: blk.quantize_i16(t, kb, 32),
        lambda t, **kw: blk.quantize_reduce([t, t], 32),
        lambda t, **kw: blk.quantize_reduce_i16([t, t], 32, kblk=kb),
        lambda t, **kw: blk.quantize_pack_nga_multi_split([t, t], 32, [1, 2], 2, 1, 1, **kw),
    ]


def test_blk_is_exported_and_refuses_cpu_tensors_and_other_dtypes():
    import ina_amd
    from ina_amd import blk
    assert ina_amd.blk is blk
    kb = torch.zeros(2, dtype=torch.int8)
    s32 = torch.zeros(64, dtype=torch.int32)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        x = torch.zeros(64, dtype=dt)
        for f in _blk_calls(kb):
            with pytest.raises(ValueError, match="no CPU fallback"):
                f(x)
        with pytest.raises(ValueError, match="no CPU fallback"):
            blk.dequantize(s32, kb, 32, dtype=dt)
        with pytest.raises(ValueError, match="no CPU fallback"):
            blk.dequantize(s32, kb, 32, out=torch.zeros(64, dtype=dt))
    for f in _blk_calls(kb):
        with pytest.raises(TypeError, match="must be torch.float32"):
            f(_FakeDev(torch.zeros(64, dtype=torch.float64)))       # a device tensor of another dtype
    with pytest.raises(TypeError, match="dtype must be float32, bfloat16 or float16"):
        blk.dequantize(s32, kb, 32, dtype=torch.float64)
    with pytest.raises(TypeError, match="int32 or int16"):
        blk.dequantize(torch.zeros(64), kb, 32, dtype=torch.bfloat16)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_blk_refuses_mixed_dtypes_a_16bit_base_and_bad_scales(dt):
    from ina_amd import blk
    x, f = torch.zeros(64, dtype=dt), torch.zeros(64)
    other = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
    for pair in ([x, f], [f, x], [x, x.to(other)]):
        for call in (lambda p: blk.block_scales(p, 32), lambda p: blk.quantize_reduce(p, 32),
                     lambda p: blk.quantize_reduce_i16(p, 32),
                     lambda p: blk.quantize_pack_nga_multi_split(p, 32, [1, 2], 2, 1, 1)):
            with pytest.raises(TypeError, match="one dtype"):
                call(pair)
    # V, degree and bits are refused before the tensors are looked at, as in ops
    with pytest.raises(ValueError, match="V must be"):
        blk.block_scales([x], 0)
    with pytest.raises(ValueError, match="degree"):
        blk.block_scales([x], 32, bits=16, degree=65534)
    with pytest.raises(ValueError, match="bits must be 16 or 32"):
        blk.block_scales([x], 32, bits=8, degree=1)


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind _req's device test are
    reached without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_blk_refuses_a_16bit_base_and_short_or_non_int8_scales(dt):
    from ina_amd import blk
    x = _FakeDev(torch.zeros(64, dtype=dt))
    with pytest.raises(TypeError, match="base must be torch.float32"):
        blk.block_scales([x, x], 32, base=x)
    with pytest.raises(TypeError, match="base must be torch.float32"):
        blk.quantize_pack_nga_multi_split([x, x], 32, [1, 2], 2, 1, 1, base=x)
    short = _FakeDev(torch.zeros(1, dtype=torch.int8))
    wide = _FakeDev(torch.zeros(2, dtype=torch.int32))
    cpu = torch.zeros(2, dtype=torch.int8)
    s32 = _FakeDev(torch.zeros(64, dtype=torch.int32))
    for kb, exc, msg in ((short, ValueError, "holds 1 elements, needs 2"), (wide, TypeError, "must be torch.int8"),
                         (cpu, ValueError, "no CPU fallback")):
        for call in (lambda: blk.quantize(x, kb, 32), lambda: blk.quantize_i16(x, kb, 32),
                     lambda: blk.quantize_reduce([x, x], 32, kblk=kb), lambda: blk.quantize_reduce_i16([x, x], 32, kblk=kb),
                     lambda: blk.block_scales([x, x], 32, out=kb), lambda: blk.dequantize(s32, kb, 32, dtype=dt),
                     lambda: blk.quantize_pack_nga_multi_split([x, x], 32, [1, 2], 2, 1, 1, kblk=kb)):
            with pytest.raises(exc, match=msg):
                call()


def test_blk_forwards_fp32_buckets_to_ops():
    """On CPU float32 input every blk function ends in the ops function's own refusal, raised from ops."""
    import traceback
    from ina_amd import blk, ops
    kb = torch.zeros(2, dtype=torch.int8)
    x = torch.zeros(64)
    calls = _blk_calls(kb) + [lambda t: blk.dequantize(torch.zeros(64, dtype=torch.int32), kb, 32),
                              lambda t: blk.dequantize(torch.zeros(64, dtype=torch.int32), kb, 32, out=t)]
    want = ["block_scales", "quantize_blk", "quantize_i16_blk", "quantize_reduce_blk", "quantize_reduce_i16_blk",
            "quantize_pack_nga_multi_split_blk", "dequantize_blk", "dequantize_blk"]
    for f, name in zip(calls, want):
        with pytest.raises(ValueError, match="no CPU fallback") as ei:
            f(x)
        frames = [(os.path.basename(fr.filename), fr.name) for fr in traceback.extract_tb(ei.value.__traceback__)]
        assert ("ops.py", name) in frames, (name, frames)
    # and the ops wrappers still refuse 16-bit buckets by name
    with pytest.raises(ValueError, match="block scales take fp32 buckets"):
        ops.block_scales([x.bfloat16()], 32)
