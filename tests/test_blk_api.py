"""The per-block-scale entry points' surface and argument checks (include/ina_blk.h), with no
GPU: the header declares exactly the nine functions, they are exported and bound, bad bits /
degree / V / W / mode and a null scale array come back as INA_EINVAL before any device work,
n == 0 is a no-op, and the Python layer refuses CPU tensors and 16-bit dtypes."""
import ctypes
import os
import re

import pytest
import torch

FAKE = 1 << 20            # an aligned address that is never touched

NAMES = {
    "ina_block_scales_f32", "ina_quantize_blk_f32_i32", "ina_quantize_blk_f32_i16_sat",
    "ina_quantize_reduce_blk_f32_i32", "ina_quantize_reduce_blk_f32_i16_sat",
    "ina_dequantize_blk_i32_f32", "ina_dequantize_blk_i16_f32", "ina_ps_apply_blk_i32",
    "ina_ps_combine_ina_blk_f32",
}


def _calls(n=64, V=32, W=2, degree=2, bits=32, mode=1, kblk=FAKE, bufs=FAKE):
    """name -> argument tuple over fake aligned pointers, for every block-scale entry point."""
    from ina_amd import _lib
    arr = _lib.ptr_array([bufs] * max(W, 1))
    return {
        "ina_block_scales_f32": (arr, W, None, n, V, degree, bits, kblk, None),
        "ina_quantize_blk_f32_i32": (bufs, kblk, V, FAKE, n, None),
        "ina_quantize_blk_f32_i16_sat": (bufs, kblk, V, FAKE, n, None, None),
        "ina_quantize_reduce_blk_f32_i32": (arr, W, kblk, mode, degree, V, FAKE, n, None),
        "ina_quantize_reduce_blk_f32_i16_sat": (arr, W, kblk, mode, degree, V, FAKE, n, None, None),
        "ina_dequantize_blk_i32_f32": (FAKE, kblk, V, FAKE, n, None),
        "ina_dequantize_blk_i16_f32": (FAKE, kblk, V, FAKE, n, None),
        "ina_ps_apply_blk_i32": (FAKE, FAKE, kblk, V, 0.5, FAKE, n, None),
        "ina_ps_combine_ina_blk_f32": (FAKE, arr, W, V, 0.5, FAKE, n, None, None),
    }


def _einval(name, msg=None, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    assert getattr(lib, name)(*_calls(**kw)[name]) == _lib.INA_EINVAL, (name, kw)
    if msg is not None:
        assert msg in lib.ina_last_error_string(), (name, kw, lib.ina_last_error_string())


def test_header_declares_the_nine_and_they_are_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    src = open(os.path.join(REPO, "include", "ina_blk.h")).read()
    ina_h = open(os.path.join(REPO, "include", "ina.h")).read()
    assert ina_h.index('#include "ina_x16.h"') < ina_h.index('#include "ina_blk.h"')
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == NAMES == set(_lib.SIGNATURES_BLK) == set(_calls())
    assert not set(_lib.SIGNATURES_BLK) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16))
    lib = _lib.load()
    for n in declared:
        fn = getattr(lib, n)
        assert list(fn.argtypes) == _lib.SIGNATURES_BLK[n] and fn.restype is ctypes.c_int, n
    assert re.search(r"#define\s+INA_BLK_GIVEN\s+0\b", code) and re.search(r"#define\s+INA_BLK_AUTO\s+1\b", code)
    assert (_lib.BLK_GIVEN, _lib.BLK_AUTO) == (0, 1)
    # nothing of this is declared in the two headers whose function sets other tests pin
    for other in ("ina.h", "ina_x16.h"):
        assert "_blk_" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", other)).read(), flags=re.S)


@pytest.mark.parametrize("bits", [0, 8, 31, 64])
def test_bad_bits_is_einval(bits):
    _einval("ina_block_scales_f32", b"bits", bits=bits)


def test_bad_degree_is_einval():
    for degree in (0, -3):
        _einval("ina_block_scales_f32", b"degree", degree=degree)
        _einval("ina_quantize_reduce_blk_f32_i32", b"degree", degree=degree)
        _einval("ina_quantize_reduce_blk_f32_i16_sat", b"degree", degree=degree)
    # too many summands for 16 bits: 32767 / degree - 1/2 <= 0 (ina_scale_for's rule)
    for degree in (65534, 70000):
        _einval("ina_block_scales_f32", b"degree", degree=degree, bits=16)
        _einval("ina_quantize_reduce_blk_f32_i16_sat", b"degree", degree=degree)
    from ina_amd import _lib
    k = ctypes.c_int(0)
    assert _lib.load().ina_scale_for(1.0, 65534, 16, ctypes.byref(k)) == _lib.INA_EINVAL


@pytest.mark.parametrize("V", [0, -1, -256])
def test_bad_v_is_einval(V):
    for name in NAMES:
        _einval(name, b"V must be", V=V)


@pytest.mark.parametrize("W", [0, -1, 65])
def test_bad_w_is_einval(W):
    for name in ("ina_block_scales_f32", "ina_quantize_reduce_blk_f32_i32", "ina_quantize_reduce_blk_f32_i16_sat",
                 "ina_ps_combine_ina_blk_f32"):
        _einval(name, b"W must be", W=W)


@pytest.mark.parametrize("mode", [2, -1, 7])
def test_bad_mode_is_einval(mode):
    _einval("ina_quantize_reduce_blk_f32_i32", b"mode", mode=mode)
    _einval("ina_quantize_reduce_blk_f32_i16_sat", b"mode", mode=mode)


def test_null_scales_and_buffers_are_einval():
    for name in NAMES - {"ina_ps_combine_ina_blk_f32"}:        # its kblk_out may be NULL
        for mode in (0, 1):
            _einval(name, kblk=None, mode=mode)
    for name in ("ina_block_scales_f32", "ina_quantize_blk_f32_i32", "ina_quantize_reduce_blk_f32_i32",
                 "ina_quantize_reduce_blk_f32_i16_sat", "ina_ps_combine_ina_blk_f32"):
        _einval(name, bufs=None)


def test_empty_bucket_is_a_no_op():
    from ina_amd import _lib
    lib = _lib.load()
    for name, args in _calls(n=0).items():
        assert getattr(lib, name)(*args) == _lib.INA_OK, name
    for name, args in _calls(n=0, kblk=None, bufs=None).items():      # nothing is looked at
        if name in ("ina_quantize_reduce_blk_f32_i32", "ina_quantize_reduce_blk_f32_i16_sat"):
            continue                                                   # mode / kblk are checked first
        assert getattr(lib, name)(*args) == _lib.INA_OK, name


def test_ops_refuse_cpu_tensors_and_16bit_dtypes():
    from ina_amd import ops, ps
    x = torch.zeros(64)
    kb = torch.zeros(2, dtype=torch.int8)
    calls = [
        lambda t: ops.block_scales([t, t], 32),
        lambda t: ops.quantize_blk(t, kb, 32),
        lambda t: ops.quantize_i16_blk(t, kb, 32),
        lambda t: ops.quantize_reduce_blk([t, t], 32),
        lambda t: ops.quantize_reduce_i16_blk([t, t], 32, kblk=kb),
        lambda t: ops.ps_apply_blk(t, torch.zeros(64, dtype=torch.int32), kb, 32, 0.5),
        lambda t: ps.combine_ina(t, [t, t], "block", 0.5, block=32),
    ]
    for f in calls:
        with pytest.raises(ValueError, match="no CPU fallback"):
            f(x)
        for dt in (torch.bfloat16, torch.float16):
            with pytest.raises(ValueError, match="block scales take fp32 buckets"):
                f(x.to(dt))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.dequantize_blk(torch.zeros(64, dtype=torch.int32), kb, 32)
    with pytest.raises(ValueError, match="block scales take fp32 buckets"):
        ops.dequantize_blk(torch.zeros(64, dtype=torch.int32), kb, 32, out=torch.zeros(64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="V must be"):
        ops.block_scales([x], 0)
    with pytest.raises(ValueError, match="degree"):
        ops.block_scales([x], 32, bits=16, degree=65534)


def test_combine_ina_refuses_an_unknown_k():
    from ina_amd import ps
    x = torch.zeros(64)
    with pytest.raises(ValueError, match="unknown k 'blocks'"):
        ps.combine_ina(x, [x, x], "blocks", 0.5)
