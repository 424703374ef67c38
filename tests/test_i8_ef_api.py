"""The refusals of the byte wire's error feedback (include/ina_i8_ef.h, ina_amd.i8, dist.ByteWireAggregator), with no
GPU: INA_EINVAL by name, in the header's order, before any device work (no pointer here is ever dereferenced)."""
import ctypes

import pytest
import torch

X, X1, R, R1, KB, OUT, OVF = (i << 20 for i in range(1, 8))           # addresses that are never touched
BOTH = SCALES, QUANT = "ina_block_scales_i8_ef", "ina_quantize_ef_i8_wire"


def _rc(name, x=X, r=R, r1=R1, kblk=KB, out=OUT, n=512, V=32, t=0, W=2, e0=0, resids=True):
    from ina_amd import _lib
    p = ctypes.byref(_lib.SrParams(0x1234, e0, 0, 0))
    args = {SCALES: (_lib.ptr_array([x, X1]), _lib.ptr_array([r, r1]) if resids else None, t, W, n, V, kblk, p, None),
            QUANT: (x, t, r, kblk, V, out, n, OVF, p, None)}[name]
    return getattr(_lib.load(), name)(*args), _lib.load().ina_last_error_string()


# each case breaks one rule and every rule the header checks AFTER it, so the message proves the order
REFUSALS = {"xtype": (BOTH, dict(t=3, V=12, kblk=None), b"xtype must be"),
            "V=12": (BOTH, dict(V=12, n=50, kblk=None), b"V must be a power of two in [8, 256]"),
            "null-kblk": (BOTH, dict(kblk=None, n=500), b"null kblk"),
            "n%V": (BOTH, dict(n=500, x=None, W=0), b"n must be a multiple of V"),
            "W": ((SCALES,), dict(W=65, r=None), b"W must be in [1, 64]"),
            "null-bucket": ((SCALES,), dict(x=None, r=None), b"null worker buffer"),
            "null-x": ((QUANT,), dict(x=None, r=None), b"null pointer"), "null-q8": ((QUANT,), dict(out=None, r=None), b"null pointer"),
            "null-resid": (BOTH, dict(r=None, x=X + 8, e0=64), b"null resid"),
            "null-resid-1": ((SCALES,), dict(r1=None, x=X + 8), b"null resid"),
            "null-resids": ((SCALES,), dict(resids=False, x=X + 8), b"null resid"),
            "misaligned-in": (BOTH, dict(x=X + 8, e0=64), b"16-byte aligned"),
            "misaligned-resid": (BOTH, dict(r=R + 8, e0=64), b"16-byte aligned"),
            "misaligned-out": ((QUANT,), dict(out=OUT + 4, e0=64), b"16-byte aligned"),
            "e0%128": (BOTH, dict(e0=64), b"e0 must be a multiple of 128 and of V"), "e0%V": (BOTH, dict(e0=128, V=256), b"e0 must be")}


@pytest.mark.parametrize("name,case", [(n, c) for c, v in REFUSALS.items() for n in v[0]])
def test_refused_by_name_in_the_headers_order(name, case):
    from ina_amd import _lib
    rc, err = _rc(name, **REFUSALS[case][1])
    assert rc == _lib.INA_EINVAL and REFUSALS[case][2] in err, (name, case, rc, err)
    assert _rc(name, n=0, r=None)[0] == _lib.INA_OK                        # n == 0 is a no-op


def test_python_surface():
    from ina_amd import dist, i8
    x, kb = torch.zeros(64), torch.zeros(2, dtype=torch.int8)
    for call in (lambda: i8.block_scales_ef([x], [x], 32), lambda: i8.quantize_ef(x, x, kb, 32, rotate=1)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    agg = dist.ByteWireAggregator(1000, V=64, device="cpu", rotate=False, error_feedback=True)
    assert agg.residual.shape == (1000,) and agg.residual.dtype == torch.float32 and not agg.residual.any()
    agg.residual.fill_(1.0)
    agg.reset_residual()
    assert not agg.residual.any()
    with pytest.raises(ValueError, match="error_feedback=False"):
        dist.ByteWireAggregator(1024, device="cpu").residual
