"""The refusals of the byte wire's stochastic rounding (include/ina_i8_sr.h, ina_amd.i8, dist.ByteWireAggregator),
with no GPU: INA_EINVAL by name, in the header's order, before any device work (no pointer here is ever dereferenced);
the scale rule at its edges; the header against the signatures table."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.conftest import REPO

X, X1, KB, OUT, OVF, SH = (i << 20 for i in range(1, 7))               # addresses that are never touched
SCALES, QUANT, SUM = "ina_block_scales_i8_sr", "ina_quantize_sr_i8_wire", "ina_sum_i8_slices_requant_sr"
BLOCKS = (SCALES, QUANT)


def _rc(name, x=X, kblk=KB, out=OUT, sh=SH, n=512, V=32, t=0, W=2, e0=0, rot_e0=0, rnd=True, slices=True):
    from ina_amd import _lib
    rot, r = ctypes.byref(_lib.SrParams(0x1234, rot_e0, 0, 0)), ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0)) if rnd else None
    args = {SCALES: (_lib.ptr_array([x, X1]), t, W, n, V, kblk, rot, None),
            QUANT: (x, t, kblk, V, out, n, OVF, rot, r, None),
            SUM: (_lib.ptr_array([x, X1]) if slices else None, W, V, out, sh, n, r, None)}[name]
    return getattr(_lib.load(), name)(*args), _lib.load().ina_last_error_string()


# each case breaks one rule and every rule the header checks AFTER it, so the message proves the order
REFUSALS = {"xtype": (BLOCKS, dict(t=3, V=12, kblk=None), b"xtype must be"),
            "V=12": (BLOCKS, dict(V=12, n=50, kblk=None), b"V must be a power of two in [8, 256]"),
            "null-kblk": (BLOCKS, dict(kblk=None, n=500), b"null kblk"),
            "n%V": (BLOCKS, dict(n=500, x=None, W=0), b"n must be a multiple of V"),
            "W": ((SCALES,), dict(W=65, x=X + 8), b"W must be in [1, 64]"),
            "null-bucket": ((SCALES,), dict(x=None, rot_e0=64), b"null worker buffer"),
            "null-x": ((QUANT,), dict(x=None, out=OUT + 4), b"null pointer"),
            "null-q8": ((QUANT,), dict(out=None, rot_e0=64), b"null pointer"),
            "misaligned": (BLOCKS, dict(x=X + 8, rot_e0=64, rnd=False), b"16-byte aligned"),
            "rot-e0": (BLOCKS, dict(rot_e0=64, rnd=False), b"e0 must be a multiple of 128 and of V"),
            "null-rnd": ((QUANT, SUM), dict(rnd=False), b"null rnd"),
            "rnd-e0%4": ((QUANT,), dict(e0=6), b"rnd->e0 must be a multiple of 4"),
            "G": ((SUM,), dict(W=65, V=12), b"G must be in [1, 64]"), "null-slices": ((SUM,), dict(slices=False, V=12), b"G must be"),
            "sum-V": ((SUM,), dict(V=12, sh=None), b"V must be a power of two in [8, 256]"),
            "null-shift": ((SUM,), dict(sh=None, n=500), b"null shift"), "sum-n%V": ((SUM,), dict(n=500, x=None), b"n must be a multiple"),
            "null-slice": ((SUM,), dict(x=None, out=None), b"null worker buffer"), "sum-null-q8": ((SUM,), dict(out=None, x=X + 8), b"null q8"),
            "sum-misaligned": ((SUM,), dict(x=X + 8, rnd=False), b"16-byte aligned"), "rnd-e0%16": ((SUM,), dict(e0=8), b"rnd->e0 must be a multiple of 16")}


@pytest.mark.parametrize("name,case", [(n, c) for c, v in REFUSALS.items() for n in v[0]])
def test_refused_by_name_in_the_headers_order(name, case):
    from ina_amd import _lib
    rc, err = _rc(name, **REFUSALS[case][1])
    assert rc == _lib.INA_EINVAL and REFUSALS[case][2] in err, (name, case, rc, err)
    assert _rc(name, n=0, rnd=False)[0] == _lib.INA_OK                     # n == 0 is a no-op, before rnd is read


def test_scale_rule_at_its_edges():
    """The largest k with absmax * 2^k + 1 <= 127 in exact rationals: either side of 126 * 2^-k, the ends, zero."""
    from ina_amd import _lib, i8
    for a in (0.0, 126.0, 126.00001, 125.99999, 63.0, 63.000004, 126.5, 1e-30, 2.0 ** -149, 3e38, 126.0 * 2.0 ** -120):
        k, fits = i8.scale_for_sr(a), lambda j: Fraction(float(np.float32(a))) * Fraction(2) ** j + 1 <= 127
        assert -126 <= k <= 127 and (fits(k) or k == -126) and (k == 127 or not fits(k + 1)), (a, k)
    assert (i8.scale_for_sr(0.0), i8.scale_for_sr(126.0), i8.scale_for(126.5), i8.scale_for_sr(126.5)) == (127, 0, 0, -1)
    with pytest.raises(_lib.InaError, match="absmax must be finite"):
        i8.scale_for_sr(float("inf"))
    assert _lib.load().ina_scale_for_i8_sr(1.0, None) == _lib.INA_EINVAL and b"null k_out" in _lib.load().ina_last_error_string()


def test_header_and_python_surface():
    from ina_amd import _lib, dist, i8
    text = open(os.path.join(REPO, "include", "ina_i8_sr.h")).read()
    decls = dict(re.findall(r"^int (ina_\w+)\(([^;]*)\);", text[text.index("*/"):], re.M))
    assert set(decls) == set(_lib.SIGNATURES_I8_SR) and len(decls) == 4 and all(hasattr(_lib.load(), d) for d in decls)
    assert all(len(args.split(",")) == len(_lib.SIGNATURES_I8_SR[name]) for name, args in decls.items())
    x, kb, q = torch.zeros(64), torch.zeros(2, dtype=torch.int8), torch.zeros(64, dtype=torch.int8)
    for call in (lambda: i8.block_scales_sr([x], 32), lambda: i8.quantize_sr(x, kb, 32, 1, rotate=1),
                 lambda: i8.sum_slices_requant_sr([q], 32, 1)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="rounding must be 'nearest' or 'stochastic', got 'up'"):
        dist.ByteWireAggregator(1024, device="cpu", rounding="up")
    with pytest.raises(ValueError, match="rounding='stochastic' and error_feedback=True exclude each other"):
        dist.ByteWireAggregator(1024, device="cpu", rounding="stochastic", error_feedback=True)
