"""The requantised gather's surface and refusals (include/ina_i8_gather.h, ina_amd.i8, dist.ByteWireAggregator), with
no GPU: every refusal is INA_EINVAL by name, in the header's order, before any device work (no pointer here is ever
dereferenced); the header declares exactly _lib.SIGNATURES_I8G and only ina_i8.h includes it."""
import ctypes
import os
import re

import pytest
import torch

X, X1, KB, OUT, SH = (i << 20 for i in range(1, 6))                   # addresses that are never touched
SUM, DEQ = "ina_sum_i8_slices_requant", "ina_dequantize_i8_gather"
BOTH = (SUM, DEQ)


def _rc(name, x=X, x1=X1, kblk=KB, out=OUT, shift=SH + 1, n=512, V=32, G=2, e0=0, slices=True):
    from ina_amd import _lib
    p = ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0))
    args = {SUM: (_lib.ptr_array([x, x1]) if slices else None, G, V, out, shift, n, None),
            DEQ: (x, shift, kblk, V, out, n, p, None)}[name]
    lib = _lib.load()
    return getattr(lib, name)(*args), lib.ina_last_error_string()


G_MSG, V_MSG, N_MSG, AL_MSG, E0_MSG = b"G must be in [1, 64]", b"V must be a power of two in [8, 256]", b"n must be a multiple of V", b"16-byte aligned", b"e0 must be"
# each case breaks one rule and every rule the header checks AFTER it, so the message proves the order
REFUSALS = {"G=0": ((SUM,), dict(G=0, V=12, shift=None), G_MSG), "G=65": ((SUM,), dict(G=65, V=12), G_MSG),
            "null-slices": ((SUM,), dict(slices=False, V=12), G_MSG),
            "V=12": (BOTH, dict(V=12, n=50, shift=None, x=None), V_MSG), "V=4": (BOTH, dict(V=4, shift=None), V_MSG),
            "V=512": (BOTH, dict(V=512, n=500), V_MSG), "sum-null-shift": ((SUM,), dict(shift=None, n=500), b"null shift"),
            "n%V": (BOTH, dict(n=500, x=None, out=None), N_MSG),
            "null-slice": ((SUM,), dict(x1=None, out=None), b"null worker buffer"),
            "null-q8-out": ((SUM,), dict(out=None, x=X + 8), b"null q8"),
            "null-q8": ((DEQ,), dict(x=None, shift=None), b"null pointer"), "null-y": ((DEQ,), dict(out=None, shift=None), b"null pointer"),
            "null-kblk": ((DEQ,), dict(kblk=None, shift=None), b"null pointer"),
            "deq-null-shift": ((DEQ,), dict(shift=None, x=X + 8), b"null shift"),
            "misaligned-in": (BOTH, dict(x=X + 8, e0=64), AL_MSG), "misaligned-out": (BOTH, dict(out=OUT + 4, e0=64), AL_MSG),
            "e0%128": ((DEQ,), dict(e0=64), E0_MSG), "e0%V": ((DEQ,), dict(e0=128, V=256), E0_MSG)}


@pytest.mark.parametrize("name,case", [(n, c) for c, v in REFUSALS.items() for n in v[0]])
def test_refused_by_name_in_the_headers_order(name, case):
    from ina_amd import _lib
    _, kw, msg = REFUSALS[case]
    rc, err = _rc(name, **kw)
    assert rc == _lib.INA_EINVAL and msg in err, (name, case, rc, err)
    assert _rc(name, n=0)[0] == _lib.INA_OK                                # n == 0 is a no-op


def test_header_table_and_python_refusals():
    from ina_amd import _lib as L, dist, i8
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    text = open(os.path.join(inc, "ina_i8_gather.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M)) == set(L.SIGNATURES_I8G) == {SUM, DEQ}
    assert re.search(r"#ifndef INA_I8_H\n#error", code) and "Not here" in text
    hits = [h for h in os.listdir(inc) if re.search(r'^#include "ina_i8_gather\.h"', open(os.path.join(inc, h)).read(), flags=re.M)]
    assert hits == ["ina_i8.h"]
    for name, args in L.SIGNATURES_I8G.items():
        assert list(getattr(L.load(), name).argtypes) == args and getattr(L.load(), name).restype is ctypes.c_int
    q, sh, kb = torch.zeros(64, dtype=torch.int8), torch.zeros(2, dtype=torch.uint8), torch.zeros(2, dtype=torch.int8)
    for call in (lambda: i8.sum_slices_requant([q], 32), lambda: i8.dequantize_gather(q, sh, kb, 32, rotate=1)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="gather must be 'i16' or 'i8', got 'x'"):
        dist.ByteWireAggregator(1024, device="cpu", gather="x")
    agg = dist.ByteWireAggregator(1024, V=64, device="cpu", gather="i8")
    assert agg.gather_shift.numel() == 16 and agg.gather_bytes == 0 and not hasattr(agg, "s16_full")
    assert dist.ByteWireAggregator(1024, V=64, device="cpu").gather == "i16"
