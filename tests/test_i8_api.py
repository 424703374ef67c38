"""The 8-bit wire's surface and refusals (include/ina_i8.h, ina_amd.i8, dist.ByteWireAggregator), with no GPU:
the header declares exactly the functions of _lib.SIGNATURES_I8 and reaches ina.h through ina_rot.h; every
refusal is INA_EINVAL by name, in the header's order, before any device work (no pointer here is ever
dereferenced, and a launch on this machine would be INA_EHIP); the scale rule against an exact search."""
import ctypes
import os
import re

import pytest
import torch

from tests import _i8_ref as ref

X, X1, KB, OUT, OVF = (i << 20 for i in range(1, 6))                  # addresses that are never touched
SCALE, SCALES, QUANT, SUM = "ina_scale_for_i8", "ina_block_scales_i8", "ina_quantize_i8_wire", "ina_sum_i8_slices"


def _rc(name, x=X, x1=X1, kblk=KB, out=OUT, n=512, V=32, t=0, W=2, sr=True, e0=0):
    from ina_amd import _lib
    p = ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0)) if sr else None
    arr = _lib.ptr_array([x, x1])
    args = {SCALES: (arr, t, W, n, V, kblk, p, None), QUANT: (x, t, kblk, V, out, n, OVF, p, None),
            SUM: (arr, W, out, n, None)}[name]
    lib = _lib.load()
    return getattr(lib, name)(*args), lib.ina_last_error_string()


BLOCK = (SCALES, QUANT)
V_MSG, E0_MSG, AL_MSG = b"V must be a power of two in [8, 256]", b"e0 must be a multiple of 128 and of V", b"16-byte aligned"
# each case breaks one rule and every rule the header checks AFTER it, so the message proves the order
REFUSALS = {"xtype": (BLOCK, dict(t=3, V=12, kblk=None), b"xtype must be"),
            "V=12": (BLOCK, dict(V=12, n=50, kblk=None), V_MSG), "V=4": (BLOCK, dict(V=4), V_MSG),
            "V=512": (BLOCK, dict(V=512), V_MSG),
            "null-kblk": (BLOCK, dict(kblk=None, n=500), b"null kblk"),
            "n%V": (BLOCK, dict(n=500, x=None, W=0), b"n must be a multiple of V"),
            "W": ((SCALES,), dict(W=65, x=X + 8), b"W must be in [1, 64]"),
            "null": (BLOCK, dict(x=None, out=OUT + 4), b"null"),
            "misaligned-in": (BLOCK, dict(x=X + 8, e0=64), AL_MSG),
            "misaligned-out": ((QUANT,), dict(out=OUT + 4, e0=64), AL_MSG),
            "e0%128": (BLOCK, dict(e0=64), E0_MSG), "e0%V": (BLOCK, dict(e0=128, V=256), E0_MSG),
            "G=0": ((SUM,), dict(W=0, x=None), b"G must be in [1, 64]"), "G=65": ((SUM,), dict(W=65), b"G must be in"),
            "null-slice": ((SUM,), dict(x1=None, out=None), b"null worker buffer"),
            "null-out16": ((SUM,), dict(out=None, x=X + 8), b"null out16"),
            "misaligned-slice": ((SUM,), dict(x1=X1 + 8), AL_MSG), "misaligned-out16": ((SUM,), dict(out=OUT + 2), AL_MSG)}


@pytest.mark.parametrize("name,case", [(n, c) for c, v in REFUSALS.items() for n in v[0]])
def test_refused_by_name_in_the_headers_order(name, case):
    from ina_amd import _lib
    _, kw, msg = REFUSALS[case]
    rc, err = _rc(name, **kw)
    assert rc == _lib.INA_EINVAL and msg in err, (name, case, rc, err)
    assert _rc(name, n=0)[0] == _lib.INA_OK                                # n == 0 is a no-op


@pytest.mark.parametrize("absmax", (0.0, 1e-45, 1.1754942e-38, 126.5, 126.50001, 127.0, 63.25, 63.250004, 3e38))
def test_scale_rule_against_an_exact_search(absmax):
    from ina_amd import i8
    a = float(torch.tensor(absmax, dtype=torch.float32))
    assert i8.scale_for(a) == ref.scale_for(a)
    assert {0.0: 127, 126.5: 0, 127.0: -1}.get(absmax, i8.scale_for(a)) == i8.scale_for(a)


def test_header_and_table_name_the_same_functions():
    from ina_amd import _lib as L
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    text = open(os.path.join(inc, "ina_i8.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M)) == set(L.SIGNATURES_I8) == {SCALE, SCALES, QUANT, SUM}
    assert re.search(r"#ifndef INA_ROT_H\n#error", code)
    hits = [h for h in os.listdir(inc) if re.search(r'^#include "ina_i8\.h"', open(os.path.join(inc, h)).read(), flags=re.M)]
    assert hits == ["ina_rot.h"]
    for name, args in L.SIGNATURES_I8.items():
        assert list(getattr(L.load(), name).argtypes) == args
    assert "Not here" in text and "G * 128 <= 32767" in text


def test_python_refusals():
    from ina_amd import _lib, dist, i8
    for bad in (-1.0, float("nan"), float("inf")):                                         # ina_scale_for's rule
        with pytest.raises(_lib.InaError, match="absmax must be finite"):
            i8.scale_for(bad)
    assert _lib.load().ina_scale_for_i8(1.0, None) == _lib.INA_EINVAL and b"null k_out" in _lib.load().ina_last_error_string()
    cpu, kb = torch.zeros(64), torch.zeros(2, dtype=torch.int8)
    for call in (lambda: i8.block_scales([cpu], 32), lambda: i8.quantize(cpu, kb, 32, rotate=1),
                 lambda: i8.sum_slices([cpu.to(torch.int8)])):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    for kw, msg in ((dict(V=12), "V must be a power of two"), (dict(V=512), "V must be a power of two"),
                    (dict(n=1000), "multiple of V"), (dict(seed=-1), "seed must be"), (dict(seed=1.5), "seed must be")):
        with pytest.raises(ValueError, match=msg):
            dist.ByteWireAggregator(**{"n": 1024, "V": 256, "device": "cpu", **kw})
    with pytest.raises(ValueError, match="wire must be 'i32' or 'i16'"):                   # unchanged
        dist.ShardedAggregator(1024, wire="i8", device="cpu")
    agg = dist.ByteWireAggregator(1000, V=64, device="cpu", rotate=False, align=96)
    assert agg.plan.shard % 384 == 0 and agg.kblk.numel() == 16 and (agg.kblk == 127).all()
