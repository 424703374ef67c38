"""The rotation's surface and refusals (include/ina_rot.h, ina_amd.rot), with no GPU: the header declares
exactly the functions of _lib.SIGNATURES_ROT and reaches ina.h through ina_blk_sr.h; every refusal is
INA_EINVAL by name before any device work (no pointer here is ever dereferenced, and a launch on this
machine would be INA_EHIP); ina_amd.rot and ps.combine_ina refuse by name."""
import ctypes
import os
import re

import pytest
import torch

X, X1, KB, OUT, OVF, LOCAL = (i << 20 for i in range(1, 7))          # addresses that are never touched
SCALES, R32, R16 = "ina_block_scales_rot", "ina_quantize_reduce_rot_i32", "ina_quantize_reduce_rot_i16_sat"
D32, D16, COMB = "ina_dequantize_rot_i32", "ina_dequantize_rot_i16", "ina_ps_combine_ina_rot_f32"
NAMES = (SCALES, R32, R16, D32, D16, COMB)


def _rc(name, x=X, kblk=KB, out=OUT, n=512, V=32, t=0, mode=1, degree=2, bits=16, sr=True, e0=0):
    from ina_amd import _lib
    p = ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0)) if sr else None
    arr = _lib.ptr_array([x, X1])
    args = {SCALES: (arr, t, 2, n, V, degree, bits, kblk, p, None),
            R32: (arr, t, 2, kblk, mode, degree, V, out, n, p, None),
            R16: (arr, t, 2, kblk, mode, degree, V, out, n, OVF, p, None),
            D32: (x, kblk, V, out, n, p, None), D16: (x, kblk, V, out, n, p, None),
            COMB: (LOCAL, arr, 2, V, 0.1, out, n, kblk, p, None)}[name]
    lib = _lib.load()
    return getattr(lib, name)(*args), lib.ina_last_error_string()


ALL, TYPED = NAMES, (SCALES, R32, R16)
V_MSG, E0_MSG = b"V must be a power of two in [8, 256]", b"e0 must be a multiple of 128 and of V"
REFUSALS = {"V=12": (ALL, dict(V=12, n=48), V_MSG), "V=4": (ALL, dict(V=4), V_MSG), "V=512": (ALL, dict(V=512), V_MSG),
            "n%V": (ALL, dict(n=500), b"n must be a multiple of V"),
            "misaligned-in": (ALL, dict(x=X + 8), b"16-byte aligned"),
            "misaligned-out": (NAMES[1:], dict(out=OUT + 4), b"16-byte aligned"),
            "null-sr": (ALL, dict(sr=False), b"null sr"),
            "e0%128": (ALL, dict(e0=64), E0_MSG), "e0%V": (ALL, dict(e0=128, V=256), E0_MSG),
            "xtype": (TYPED, dict(t=3), b"xtype must be"),
            "degree": ((SCALES, R16), dict(degree=70000, bits=16), b"too many summands")}      # ina_scale_for's rule


@pytest.mark.parametrize("name,case", [(n, c) for c, v in REFUSALS.items() for n in v[0]])
def test_refused_by_name_before_any_device_work(name, case):
    from ina_amd import _lib
    _, kw, msg = REFUSALS[case]
    rc, err = _rc(name, **kw)
    assert rc == _lib.INA_EINVAL and msg in err, (name, case, rc, err)
    assert _rc(name, n=0)[0] == _lib.INA_OK                                # n == 0 is a no-op


def test_header_and_table_name_the_same_functions():
    from ina_amd import _lib as L
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "ina_rot.h")).read(), flags=re.S)
    assert set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M)) == set(L.SIGNATURES_ROT) == set(NAMES)
    assert re.search(r"#ifndef INA_BLK_SR_H\n#error", code)
    hits = [h for h in os.listdir(inc) if re.search(r'^#include "ina_rot\.h"', open(os.path.join(inc, h)).read(), flags=re.M)]
    assert hits == ["ina_blk_sr.h"]
    for t in (t for t in dir(L) if t.startswith("SIGNATURES") and t != "SIGNATURES_ROT"):
        assert not set(NAMES) & set(getattr(L, t)), t
    lib = L.load()
    for name in NAMES:
        assert list(getattr(lib, name).argtypes) == L.SIGNATURES_ROT[name]


def test_python_refusals():
    from ina_amd import ps, rot
    cpu = torch.zeros(64)
    for call in (lambda: rot.quantize_reduce([cpu], 32, 1), lambda: rot.block_scales([cpu], 32, 1),
                 lambda: rot.dequantize(cpu.int(), torch.zeros(2, dtype=torch.int8), 32, 1),
                 lambda: ps.combine_ina(cpu, [cpu], "block", 0.1, block=32, rotate=1)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="rotate needs k=\"block\""):
        ps.combine_ina(cpu, [cpu], 16, 0.1, rotate=1)
