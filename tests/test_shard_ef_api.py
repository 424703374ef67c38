"""Error feedback on the sharded int16 wire: the surface and the argument checks (include/ina_shard_ef.h,
ina_amd.ef, ina_amd.dist), with no GPU.  The header declares exactly the two functions, refuses a lone
include and sits between ina_shard_blk.h and ina_ef.h; the names are in SIGNATURES_SHARD_EF and in no
other table or header, exported and bound, with the wire siblings' arguments and resid after x; the
checks come in the siblings' order with their messages before any device work and n == 0 is a no-op;
ina_amd.ef refuses CPU tensors, other dtypes and mismatched residuals by name; and the aggregators
refuse error feedback without a device (ShardedAggregator) or altogether (RangeAggregator)."""
import ctypes
import os
import re

import pytest
import torch

# aligned addresses that are never touched, far enough apart for any n used here
X, RESID, WIRE, KBLK = 1 << 20, 2 << 20, 3 << 20, 4 << 20
GLOBAL, BLK = "ina_quantize_ef_f32_i16_wire", "ina_quantize_ef_blk_f32_i16_wire"
NAMES = {GLOBAL, BLK}


def _calls(x=X, resid=RESID, wire=WIRE, kblk=KBLK, n=64, k=9, V=32):
    return {GLOBAL: (x, resid, wire, n, k, None), BLK: (x, resid, kblk, V, wire, n, None)}


def _rc(name, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    return getattr(lib, name)(*_calls(**kw)[name]), lib.ina_last_error_string()


def _einval(name, msg, **kw):
    from ina_amd import _lib
    rc, err = _rc(name, **kw)
    assert rc == _lib.INA_EINVAL and msg in err, (name, kw, rc, err)


def test_header_declares_the_two_and_they_are_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_shard_ef.h")).read()
    includes = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(inc, "ina.h")).read(), flags=re.M)
    assert includes.count("ina_shard_ef.h") == 1
    at = includes.index("ina_shard_ef.h")
    assert includes.index("ina_shard_blk.h") < at and includes[at + 1] == "ina_ef.h"
    assert "#ifndef INA_SHARD_BLK_H\n#error" in src                                        # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == NAMES == set(_lib.SIGNATURES_SHARD_EF) == set(_calls())
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16) | set(_lib.SIGNATURES_BLK) |
              set(_lib.SIGNATURES_PKT_BLK) | set(_lib.SIGNATURES_SWITCH_BLK) | set(_lib.SIGNATURES_SHARD_BLK) |
              set(_lib.SIGNATURES_BLK_X16) | set(_lib.SIGNATURES_EF))
    assert not declared & others
    for h in sorted(os.listdir(inc)):                                                      # declared nowhere else
        if h == "ina_shard_ef.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SIGNATURES_SHARD_EF[name] and fn.restype is ctypes.c_int, name
    # the wire siblings' arguments with resid after x
    for name, sib in ((GLOBAL, _lib.SIGNATURES["ina_quantize_f32_i16_wire"]),
                      (BLK, _lib.SIGNATURES_SHARD_BLK["ina_quantize_blk_f32_i16_wire"])):
        assert _lib.SIGNATURES_SHARD_EF[name] == sib[:1] + [ctypes.c_void_p] + sib[1:], name


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_shard_ef.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { return ina_quantize_ef_f32_i16_wire(0, 0, 0, 0, 1, 0) + '
                 'ina_quantize_ef_blk_f32_i16_wire(0, 0, 0, 1, 0, 0, 0); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_checks_come_in_the_siblings_order_with_their_messages():
    for k in (-127, 128, 500):
        _einval(GLOBAL, b"k out of range [-126,127]", k=k)
        _einval(GLOBAL, b"k out of range", k=k, n=0)                     # before the empty call's no-op
        _einval(GLOBAL, b"k out of range", k=k, x=None, resid=None)
    for V in (0, -1, -256):
        _einval(BLK, b"V must be >= 1", V=V)
        _einval(BLK, b"V must be >= 1", V=V, n=0)
        _einval(BLK, b"V must be >= 1", V=V, kblk=None, resid=None)
    for V in (32, 100, 1):
        _einval(BLK, b"null kblk", kblk=None, V=V)
        _einval(BLK, b"null kblk", kblk=None, x=None, resid=None, V=V)   # kblk is looked at first
    for name in NAMES:
        _einval(name, b"null pointer", x=None)
        _einval(name, b"null pointer", wire=None)
        _einval(name, b"null pointer", x=None, resid=None)               # the sibling's check first
        _einval(name, b"null resid", resid=None)


def test_resid_must_not_overlap_x_or_wire():
    from ina_amd import _lib
    n = 64
    for name in NAMES:
        for other in ("x", "wire"):
            base = {"x": X, "wire": WIRE}[other]
            for resid in (base, base + 4 * (n - 1), base - 4 * (n - 1)):
                _einval(name, b"resid overlaps x or wire", resid=resid, n=n)
    # (a residual right beside x shares no byte with it and is a launch: tests/test_gpu_shard_ef.py runs it)
    rc, err = _rc(GLOBAL, n=0, resid=X)                                   # an empty call looks at nothing
    assert rc == _lib.INA_OK, err


def test_empty_bucket_is_a_no_op():
    from ina_amd import _lib
    for name in NAMES:
        rc, err = _rc(name, n=0)
        assert rc == _lib.INA_OK, (name, err)
        rc, err = _rc(name, n=0, x=None, resid=None, wire=None, kblk=None)   # nothing is looked at
        assert rc == _lib.INA_OK, (name, err)


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind _req's device test are
    reached without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def _ef_calls(kb=None, V=32):
    from ina_amd import ef
    kb = _FakeDev(torch.zeros(2, dtype=torch.int8)) if kb is None else kb
    return [lambda x, r: ef.quantize_i16_wire(x, r, 9), lambda x, r: ef.quantize_i16_wire_blk(x, r, kb, V)]


def test_ef_wire_calls_refuse_by_name_before_any_device_call():
    x, r = torch.zeros(64), torch.zeros(64)
    for f in _ef_calls():
        with pytest.raises(ValueError, match="no CPU fallback"):
            f(x, r)
    dx, dr = _FakeDev(x), _FakeDev(r)
    for f in _ef_calls():
        with pytest.raises(ValueError, match="resid must be a device .* no CPU fallback"):
            f(dx, r)
        with pytest.raises(TypeError, match="x must be torch.float32"):
            f(_FakeDev(torch.zeros(64, dtype=torch.float64)), dr)
        with pytest.raises(TypeError, match="resid must be torch.float32"):
            f(dx, _FakeDev(torch.zeros(64, dtype=torch.bfloat16)))
        with pytest.raises(ValueError, match="resid holds 63 elements, the bucket 64"):
            f(dx, _FakeDev(torch.zeros(63)))
        for dt in (torch.bfloat16, torch.float16):
            with pytest.raises(ValueError, match=f"the sharded int16 wire takes fp32 buckets: x is {dt}"):
                f(_FakeDev(torch.zeros(64, dtype=dt)), dr)
    blk = lambda **kw: _ef_calls(**kw)[1](dx, dr)                          # noqa: E731
    with pytest.raises(ValueError, match="no CPU fallback"):
        blk(kb=torch.zeros(2, dtype=torch.int8))
    with pytest.raises(TypeError, match="kblk must be torch.int8"):
        blk(kb=_FakeDev(torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="kblk holds 1 elements, needs 2"):
        blk(kb=_FakeDev(torch.zeros(1, dtype=torch.int8)))
    with pytest.raises(ValueError, match="V must be >= 1"):
        blk(V=0)


def test_aggregators_and_error_feedback_without_a_device():
    import inspect
    from ina_amd.dist import RangeAggregator, ShardedAggregator
    assert inspect.signature(ShardedAggregator.__init__).parameters["error_feedback"].default is False
    assert "error_feedback" not in inspect.signature(RangeAggregator.__init__).parameters
    cpu = torch.device("cpu")
    for wire in ("i16", "i32"):
        for k in (9, "block"):
            with pytest.raises(ValueError, match="error_feedback=True keeps its residual on the GPU .* no CPU fallback"):
                ShardedAggregator(1000, k=k, wire=wire, V=32, device=cpu, error_feedback=True)
        with pytest.raises(TypeError, match="unexpected keyword argument 'error_feedback'"):
            RangeAggregator(1000, k=9, wire=wire, V=32, device=cpu, error_feedback=True)
    # the default: no residual, and nothing to reset
    agg = ShardedAggregator(1000, k=9, wire="i16", V=32, device=cpu)
    assert agg.error_feedback is False and agg.residual is None
    with pytest.raises(AttributeError, match="only with error_feedback=True"):
        agg.reset_residual()
    assert "residual" in RangeAggregator.__doc__ and "error feedback" in RangeAggregator.__doc__
