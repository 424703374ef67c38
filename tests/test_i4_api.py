"""The 4-bit wire's surface and refusals (include/ina_i4.h, ina_amd.i4, dist.NibbleWireAggregator), with no GPU:
INA_EINVAL by name, in the header's order, before any device work (no pointer here is ever dereferenced)."""
import ctypes
import os
import re

import pytest
import torch

from tests import _i4_ref as ref
from tests.conftest import REPO

X, X1, KB, OUT, OVF, SH = (i << 20 for i in range(1, 7))               # addresses that are never touched
SCALES, QUANT, SUM, RQ = "ina_block_scales_i4", "ina_quantize_i4_wire", "ina_sum_i4_slices", "ina_sum_i4_slices_requant"
BLOCK, SUMS = (SCALES, QUANT), (SUM, RQ)


def _rc(name, x=X, x1=X1, kblk=KB, out=OUT, sh=SH, n=512, V=32, t=0, W=2, e0=0, slices=True):
    from ina_amd import _lib
    p, arr = ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0)), _lib.ptr_array([x, x1]) if slices else None
    args = {SCALES: (arr, t, W, n, V, kblk, p, None), QUANT: (x, t, kblk, V, out, n, OVF, p, None),
            SUM: (arr, W, out, n, None), RQ: (arr, W, V, out, sh, n, None)}[name]
    return getattr(_lib.load(), name)(*args), _lib.load().ina_last_error_string()


V_MSG, AL_MSG, E0_MSG = b"V must be a power of two in [8, 256]", b"16-byte aligned", b"e0 must be a multiple of 128 and of V"
# each case breaks one rule and every rule the header checks AFTER it, so the message proves the order
REFUSALS = {"xtype": (BLOCK, dict(t=3, V=12, kblk=None), b"xtype must be"),
            "V=12": (BLOCK, dict(V=12, n=50, kblk=None), V_MSG), "V=4": (BLOCK, dict(V=4, kblk=None), V_MSG),
            "V=512": (BLOCK, dict(V=512, kblk=None), V_MSG), "null-kblk": (BLOCK, dict(kblk=None, n=500), b"null kblk"),
            "n%V": (BLOCK, dict(n=500, x=None, W=0), b"n must be a multiple of V"),
            "W": ((SCALES,), dict(W=65, x=X + 8), b"W must be in [1, 64]"), "null": (BLOCK, dict(x=None, out=OUT + 4, e0=64), b"null"),
            "null-q4": ((QUANT,), dict(out=None, x=X + 8, e0=64), b"null pointer"),
            "misaligned-in": (BLOCK, dict(x=X + 8, e0=64), AL_MSG), "misaligned-q4": ((QUANT,), dict(out=OUT + 4, e0=64), AL_MSG),
            "e0%128": (BLOCK, dict(e0=64), E0_MSG), "e0%V": (BLOCK, dict(e0=128, V=256), E0_MSG),
            "G=0": (SUMS, dict(W=0, V=12, n=500), b"G must be in [1, 64]"), "G=65": (SUMS, dict(W=65, V=12, n=500), b"G must be in"),
            "null-slices": (SUMS, dict(slices=False, V=12, n=500), b"G must be in [1, 64]"),
            "n%8": ((SUM,), dict(n=500, x1=None), b"n must be a multiple of 8"),
            "sum-V": ((RQ,), dict(V=12, sh=None), V_MSG), "null-shift": ((RQ,), dict(sh=None, n=500), b"null shift"),
            "sum-n%V": ((RQ,), dict(n=504, x1=None), b"n must be a multiple of V"),
            "null-slice": (SUMS, dict(x1=None, out=None), b"null worker buffer"),
            "null-out16": ((SUM,), dict(out=None, x=X + 8), b"null out16"), "null-q8": ((RQ,), dict(out=None, x=X + 8), b"null q8"),
            "misaligned-slice": (SUMS, dict(x1=X1 + 8), AL_MSG), "misaligned-out": (SUMS, dict(out=OUT + 8), AL_MSG)}


@pytest.mark.parametrize("name,case", [(n, c) for c, v in REFUSALS.items() for n in v[0]])
def test_refused_by_name_in_the_headers_order(name, case):
    from ina_amd import _lib
    rc, err = _rc(name, **REFUSALS[case][1])
    assert rc == _lib.INA_EINVAL and REFUSALS[case][2] in err, (name, case, rc, err)
    assert _rc(name, n=0)[0] == _lib.INA_OK                                # n == 0 is a no-op


@pytest.mark.parametrize("absmax", (0.0, 2.0 ** -149, 1.1754942e-38, 6.5, 6.5000005, 6.4999995, 3.25, 3.2500002, 7.0,
                                    6.5 * 2.0 ** -100, 6.5 * 2.0 ** 100 * (1 + 2.0 ** -23), 3e38))
def test_scale_rule_at_its_edges(absmax):
    from ina_amd import _lib, i4
    a = float(torch.tensor(absmax, dtype=torch.float32))
    assert i4.scale_for(a) == ref.scale_for(a) == {0.0: 127, 6.5: 0, 7.0: -1, 3.25: 1, 3e38: -126}.get(absmax, i4.scale_for(a))
    with pytest.raises(_lib.InaError, match="absmax must be finite"):
        i4.scale_for(-absmax if absmax else float("nan"))
    assert _lib.load().ina_scale_for_i4(1.0, None) == _lib.INA_EINVAL and b"null k_out" in _lib.load().ina_last_error_string()


def test_header_table_and_python_surface():
    import ina_amd
    from ina_amd import _lib as L, dist, i4
    inc = os.path.join(REPO, "include")
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "ina_i4.h")).read(), flags=re.S)
    decls = dict(re.findall(r"^int\s+(ina_\w+)\s*\(([^;]*)\);", code, flags=re.M))
    assert set(decls) == set(L.SIGNATURES_I4) and len(decls) == 5 and re.search(r"#ifndef INA_I8_SR_H\n#error", code)
    for name, args in L.SIGNATURES_I4.items():
        assert list(getattr(L.load(), name).argtypes) == args and len(decls[name].split(",")) == len(args), name
    hits = [h for h in os.listdir(inc) if re.search(r'^#include "ina_i4\.h"', open(os.path.join(inc, h)).read(), flags=re.M)]
    sr = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "ina_i8_sr.h")).read(), flags=re.S)
    assert hits == ["ina_i8_sr.h"] and re.search(r'\)\s*;\s*#include "ina_i4\.h"\s*#endif\s*$', sr) and ina_amd.i4 is i4
    cpu, kb, q = torch.zeros(64), torch.zeros(2, dtype=torch.int8), torch.zeros(32, dtype=torch.uint8)
    for call in (lambda: i4.block_scales([cpu], 32), lambda: i4.quantize(cpu, kb, 32, rotate=1),
                 lambda: i4.sum_slices([q]), lambda: i4.sum_slices_requant([q], 32)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    for kw, msg in ((dict(V=12), "V must be a power of two"), (dict(V=512), "V must be a power of two"),
                    (dict(gather="i4"), "gather must be 'i16' or 'i8', got 'i4'"), (dict(n=1000), "multiple of V")):
        with pytest.raises(ValueError, match=msg):
            dist.NibbleWireAggregator(**{"n": 1024, "V": 256, "device": "cpu", **kw})
    agg = dist.NibbleWireAggregator(1000, V=64, device="cpu", rotate=False, align=96)
    assert agg.plan.shard % 384 == 0 and agg.q4.numel() == agg.plan.padded // 2 and (agg.kblk == 127).all() and agg.gather == "i8"
