"""The bf16 / fp16 entry points' argument checks (include/ina.h "bf16 / fp16 gradients"), with
no GPU: a bad type code, k out of range and null buffers come back as INA_EINVAL before any
device work, n == 0 is a no-op, and the Python layer still refuses CPU tensors as such.

(ina_absmax_multi_x16 at n == 0 zeroes *out_dev like its fp32 sibling, which is device work, so
its n == 0 case is not exercised here.)"""
import ctypes

import pytest
import torch


def _calls(xtype=1, k=8, n=64):
    """name -> argument tuple with null buffers, for every 16-bit entry point."""
    from ina_amd import _lib
    P = _lib.ptr_array
    prm = _lib.NgaParams(1, 2, 0, 1, 0, 1, 16384, 32)
    prm2 = (_lib.NgaParams * 2)(prm, prm)
    return {
        "ina_quantize_x16_i32": (None, xtype, None, n, k, None),
        "ina_quantize_x16_i16_sat": (None, xtype, None, n, k, 32, None, None),
        "ina_quantize_reduce_x16_i32": (P([None, None]), xtype, 2, None, n, k, None),
        "ina_quantize_reduce_x16_i16_sat": (P([None, None]), xtype, 2, None, n, k, 32, None, None),
        "ina_absmax_multi_x16": (P([None, None]), xtype, 2, None, n, None, None),
        "ina_quantize_pack_nga_x16_desc": (None, xtype, None, n, k, ctypes.byref(prm), None, 144, None, None),
        "ina_quantize_pack_nga_multi_split_x16": (P([None, None]), xtype, 2, None, n, k, prm2, P([None, None]),
                                                  P([None, None]), None, None),
        "ina_dequantize_i32_x16": (None, None, xtype, n, k, None),
        "ina_dequantize_i16_x16": (None, None, xtype, n, k, None),
    }


def test_every_declared_x16_symbol_is_exported_and_bound():
    """Every function include/ina_x16.h declares (ina.h includes it) is exported by libina.so,
    has its signature in _lib.SIGNATURES_X16, and is covered by the argument checks below."""
    import os
    import re
    from ina_amd import _lib
    from tests.conftest import REPO
    src = open(os.path.join(REPO, "include", "ina_x16.h")).read()
    assert '#include "ina_x16.h"' in open(os.path.join(REPO, "include", "ina.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", src, flags=re.M))
    lib = _lib.load()
    assert len(declared) == 9 and all("x16" in n for n in declared)
    assert declared == set(_lib.SIGNATURES_X16) == set(_calls())
    assert not set(_lib.SIGNATURES_X16) & set(_lib.SIGNATURES)
    for n in declared:
        fn = getattr(lib, n)
        assert list(fn.argtypes) == _lib.SIGNATURES_X16[n] and fn.restype is ctypes.c_int, n
    assert (_lib.X16_BF16, _lib.X16_F16) == (1, 2)
    assert re.search(r"#define\s+INA_X16_BF16\s+1\b", src) and re.search(r"#define\s+INA_X16_F16\s+2\b", src)


@pytest.mark.parametrize("xtype", [0, 3, -1])
def test_bad_type_code_is_einval(xtype):
    from ina_amd import _lib
    lib = _lib.load()
    # otherwise valid arguments (fake, aligned pointers that are never touched): the type code
    # alone is refused
    for name, args in _calls(xtype).items():
        assert getattr(lib, name)(*args) == _lib.INA_EINVAL, name
        assert b"INA_X16_BF16" in lib.ina_last_error_string(), name
    fake = 1 << 20
    assert lib.ina_quantize_x16_i32(fake, xtype, fake, 64, 8, None) == _lib.INA_EINVAL
    assert lib.ina_dequantize_i32_x16(fake, fake, xtype, 64, 8, None) == _lib.INA_EINVAL
    assert b"INA_X16_F16" in lib.ina_last_error_string()


@pytest.mark.parametrize("xtype", [1, 2])
def test_k_range_null_buffers_and_empty_buckets(xtype):
    from ina_amd import _lib
    lib = _lib.load()
    for k in (128, -127, 500):
        for name, args in _calls(xtype, k=k).items():
            if name == "ina_absmax_multi_x16":           # takes no k
                continue
            assert getattr(lib, name)(*args) == _lib.INA_EINVAL, (name, k)
            assert b"k out of range" in lib.ina_last_error_string(), (name, k)
    for name, args in _calls(xtype).items():             # n = 64 with null buffers
        assert getattr(lib, name)(*args) == _lib.INA_EINVAL, name
        assert lib.ina_last_error_string() and b"k out of range" not in lib.ina_last_error_string(), name
    for name, args in _calls(xtype, n=0).items():        # n == 0: nothing to do, nothing touched
        if name == "ina_absmax_multi_x16":
            continue
        assert getattr(lib, name)(*args) == _lib.INA_OK, name
    # an odd address cannot hold 16-bit values
    fake = 1 << 20
    assert lib.ina_quantize_x16_i32(fake + 1, xtype, fake, 64, 8, None) == _lib.INA_EINVAL
    assert b"2-byte aligned" in lib.ina_last_error_string()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cpu_16bit_tensors_are_refused_as_cpu_tensors(dtype):
    """Not a dtype error any more: the 16-bit dtypes are accepted, a CPU tensor is not."""
    from ina_amd import ops
    x = torch.zeros(16, dtype=dtype)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.quantize(x, 16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.quantize_reduce([x, x], 16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.absmax(x)
    with pytest.raises(TypeError, match="one dtype"):
        ops.quantize_reduce([x, x.float()], 16)
