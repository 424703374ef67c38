"""bf16 / fp16 buckets on the sharded int16 wire: the surface and the argument checks
(include/ina_shard_x16.h, ina_amd.wire, ina_amd.dist), with no GPU.  The header declares exactly the four
functions, refuses a lone include and sits between ina_shard_blk.h and ina_shard_ef.h; the names are in
SIGNATURES_SHARD_X16 and in no other table or header, exported and bound, with the fp32 siblings'
arguments plus the type code after the 16-bit pointer; the checks come in the siblings' order with their
messages before any device work, the type code first, and n == 0 is a no-op; ina_amd.wire refuses CPU
tensors, other dtypes and wrong sizes by name; and the aggregators take out_dtype (float32 by default)
and refuse any other dtype for it."""
import ctypes
import os
import re

import pytest
import torch

# aligned addresses that are never touched, far enough apart for any n used here
X, WIRE, KBLK, OUT16, Y, OVF = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20
QG, QB = "ina_quantize_x16_i16_wire", "ina_quantize_blk_x16_i16_wire"
FG, FB = "ina_i16_wire_finish_x16", "ina_i16_wire_finish_blk_x16"
NAMES = {QG, QB, FG, FB}
BLOCK = {QB, FB}
BAD_TYPE = b"16-bit type must be INA_X16_BF16 (1) or INA_X16_F16 (2)"


def _calls(x=X, wire=WIRE, kblk=KBLK, out16=OUT16, y=Y, ovf=OVF, n=64, k=9, V=32, t=1):
    return {QG: (x, t, wire, n, k, None), QB: (x, t, kblk, V, wire, n, None),
            FG: (wire, n, k, V, out16, y, t, ovf, None), FB: (wire, n, kblk, V, out16, y, t, ovf, None)}


def _rc(name, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    return getattr(lib, name)(*_calls(**kw)[name]), lib.ina_last_error_string()


def _einval(name, msg, **kw):
    from ina_amd import _lib
    rc, err = _rc(name, **kw)
    assert rc == _lib.INA_EINVAL and msg in err, (name, kw, rc, err)


def test_header_declares_the_four_and_they_are_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_shard_x16.h")).read()
    includes = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(inc, "ina.h")).read(), flags=re.M)
    assert includes.count("ina_shard_x16.h") == 1
    at = includes.index("ina_shard_x16.h")
    assert includes[at - 1] == "ina_shard_blk.h" and includes[at + 1] == "ina_shard_ef.h"
    assert "#ifndef INA_SHARD_BLK_H\n#error" in src                                        # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == NAMES == set(_lib.SIGNATURES_SHARD_X16) == set(_calls())
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16) | set(_lib.SIGNATURES_BLK) |
              set(_lib.SIGNATURES_PKT_BLK) | set(_lib.SIGNATURES_SWITCH_BLK) | set(_lib.SIGNATURES_SHARD_BLK) |
              set(_lib.SIGNATURES_BLK_X16) | set(_lib.SIGNATURES_EF) | set(_lib.SIGNATURES_SHARD_EF))
    assert not declared & others
    for h in sorted(os.listdir(inc)):                                                      # declared nowhere else
        if h == "ina_shard_x16.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SIGNATURES_SHARD_X16[name] and fn.restype is ctypes.c_int, name
    # the fp32 siblings' arguments with the type code after the 16-bit pointer: x is argument 0 of a
    # quantiser, y argument 5 of a finish
    for name, sib, at in ((QG, _lib.SIGNATURES["ina_quantize_f32_i16_wire"], 1),
                          (QB, _lib.SIGNATURES_SHARD_BLK["ina_quantize_blk_f32_i16_wire"], 1),
                          (FG, _lib.SIGNATURES["ina_i16_wire_finish"], 6),
                          (FB, _lib.SIGNATURES_SHARD_BLK["ina_i16_wire_finish_blk"], 6)):
        assert _lib.SIGNATURES_SHARD_X16[name] == sib[:at] + [ctypes.c_int] + sib[at:], name


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_shard_x16.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { return ina_quantize_x16_i16_wire(0, INA_X16_BF16, 0, 0, 1, 0) + '
                 'ina_quantize_blk_x16_i16_wire(0, INA_X16_F16, 0, 1, 0, 0, 0) + '
                 'ina_i16_wire_finish_x16(0, 0, 1, 1, 0, 0, INA_X16_BF16, 0, 0) + '
                 'ina_i16_wire_finish_blk_x16(0, 0, 0, 1, 0, 0, INA_X16_F16, 0, 0); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_type_code_is_checked_first():
    """Where include/ina_x16.h's functions put it: before k, V, the empty call's no-op and the pointers."""
    for t in (0, 3, -1, 16):
        for name in NAMES:
            _einval(name, BAD_TYPE, t=t)
            _einval(name, BAD_TYPE, t=t, n=0)
            _einval(name, BAD_TYPE, t=t, k=500, V=0, x=None, wire=None, kblk=None, y=None)
    for t in (1, 2):
        for name in NAMES:
            rc, err = _rc(name, t=t, n=0)
            from ina_amd import _lib
            assert rc == _lib.INA_OK, (name, err)


def test_checks_come_in_the_siblings_order_with_their_messages():
    for k in (-127, 128, 500):
        for name in (QG, FG):
            _einval(name, b"k out of range [-126,127]", k=k)
            _einval(name, b"k out of range", k=k, n=0)                   # before the empty call's no-op
            _einval(name, b"k out of range", k=k, x=None, wire=None)
        _einval(FG, b"k out of range", k=k, V=0)                         # k before V
    for V in (0, -1, -256):
        _einval(FG, b"V must be > 0", V=V)
        _einval(FG, b"V must be > 0", V=V, n=0)
        _einval(FG, b"V must be > 0", V=V, wire=None)
        for name in BLOCK:
            _einval(name, b"V must be >= 1", V=V)
            _einval(name, b"V must be >= 1", V=V, n=0)
            _einval(name, b"V must be >= 1", V=V, kblk=None, x=None, wire=None)
    for V in (32, 100, 1):
        for name in BLOCK:
            _einval(name, b"null kblk", kblk=None, V=V)
            _einval(name, b"null kblk", kblk=None, x=None, wire=None, V=V)   # kblk is looked at first
    for name in (QG, QB):
        _einval(name, b"null pointer", x=None)
        _einval(name, b"null pointer", wire=None)
        _einval(name, b"null pointer", x=None, wire=None)
        _einval(name, b"16-bit buffers must be 2-byte aligned", x=X + 1)
        _einval(name, b"null pointer", x=X + 1, wire=None)               # the sibling's checks first
    for name in (FG, FB):
        _einval(name, b"null pointer", wire=None)
        _einval(name, b"null pointer", wire=None, out16=None, y=None, ovf=None)
        _einval(name, b"16-bit buffers must be 2-byte aligned", y=Y + 1)
        _einval(name, b"null pointer", wire=None, y=Y + 1)


def test_empty_bucket_is_a_no_op():
    from ina_amd import _lib
    for name in NAMES:
        for t in (1, 2):
            rc, err = _rc(name, n=0, t=t)
            assert rc == _lib.INA_OK, (name, err)
            rc, err = _rc(name, n=0, t=t, x=None, wire=None, kblk=None, out16=None, y=None, ovf=None)
            assert rc == _lib.INA_OK, (name, err)                         # nothing is looked at
            rc, err = _rc(name, n=0, t=t, x=X + 1, y=Y + 1)
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


X16 = (torch.bfloat16, torch.float16)


def test_wire_quantisers_refuse_by_name_before_any_device_call():
    from ina_amd import wire
    kb = _FakeDev(torch.zeros(2, dtype=torch.int8))
    calls = [lambda x, **kw: wire.quantize(x, 9, **kw), lambda x, **kw: wire.quantize_blk(x, kb, 32, **kw)]
    for dt in X16 + (torch.float32,):
        x = torch.zeros(64, dtype=dt)
        for f in calls:
            with pytest.raises(ValueError, match="x must be a device .* no CPU fallback"):
                f(x)
    for f in calls:
        with pytest.raises(TypeError, match="x must be torch.float32"):           # any other dtype: the fp32 path's refusal
            f(_FakeDev(torch.zeros(64, dtype=torch.float64)))
        with pytest.raises(TypeError, match="x must be a torch.Tensor"):
            f([0.0] * 64)
    for dt in X16:
        dx = _FakeDev(torch.zeros(64, dtype=dt))
        for f in calls:
            with pytest.raises(ValueError, match="out must be a device .* no CPU fallback"):
                f(dx, out=torch.zeros(64, dtype=torch.int32))
            with pytest.raises(TypeError, match="out must be torch.int32"):
                f(dx, out=_FakeDev(torch.zeros(64, dtype=torch.int16)))
            with pytest.raises(ValueError, match="out holds 63 elements, needs 64"):
                f(dx, out=_FakeDev(torch.zeros(63, dtype=torch.int32)))
            with pytest.raises(ValueError, match="x must be contiguous"):
                f(_FakeDev(torch.zeros(128, dtype=dt)[::2]))
        with pytest.raises(ValueError, match="kblk must be a device .* no CPU fallback"):
            wire.quantize_blk(dx, torch.zeros(2, dtype=torch.int8), 32)
        with pytest.raises(TypeError, match="kblk must be torch.int8"):
            wire.quantize_blk(dx, _FakeDev(torch.zeros(2, dtype=torch.int32)), 32)
        with pytest.raises(ValueError, match="kblk holds 1 elements, needs 2"):
            wire.quantize_blk(dx, _FakeDev(torch.zeros(1, dtype=torch.int8)), 32)
        with pytest.raises(ValueError, match="V must be >= 1"):
            wire.quantize_blk(dx, kb, 0)


def test_wire_finishes_refuse_by_name_before_any_device_call():
    from ina_amd import wire
    kb = _FakeDev(torch.zeros(2, dtype=torch.int8))
    # (want_out16=False: the outputs are checked in the order out16, y, overflow, and an out16 the
    # call allocated itself would be a real CPU tensor here)
    calls = [lambda w, **kw: wire.finish(w, 9, 32, want_out16=False, **kw),
             lambda w, **kw: wire.finish_blk(w, kb, 32, want_out16=False, **kw)]
    dw = _FakeDev(torch.zeros(64, dtype=torch.int32))
    for f in calls:
        for bad in (torch.float64, torch.int16):
            with pytest.raises(TypeError, match="dtype must be float32, bfloat16 or float16"):
                f(dw, dtype=bad)
            with pytest.raises(TypeError, match="y must be float32, bfloat16 or float16"):
                f(dw, y=_FakeDev(torch.zeros(64, dtype=bad)))
        for dt in X16:
            with pytest.raises(ValueError, match="wire_sum must be a device .* no CPU fallback"):
                f(torch.zeros(64, dtype=torch.int32), y=_FakeDev(torch.zeros(64, dtype=dt)))
            with pytest.raises(TypeError, match="wire_sum must be torch.int32"):
                f(_FakeDev(torch.zeros(64, dtype=torch.int64)), y=_FakeDev(torch.zeros(64, dtype=dt)))
            with pytest.raises(ValueError, match="y must be a device .* no CPU fallback"):
                f(dw, y=torch.zeros(64, dtype=dt))
            with pytest.raises(ValueError, match="y holds 63 elements, needs 64"):
                f(dw, y=_FakeDev(torch.zeros(63, dtype=dt)))
            y = _FakeDev(torch.zeros(64, dtype=dt))
            with pytest.raises(TypeError, match="out16 must be torch.int16"):
                f(dw, y=y, out16=_FakeDev(torch.zeros(64, dtype=torch.int32)))
            with pytest.raises(ValueError, match="out16 holds 10 elements, needs 64"):
                f(dw, y=y, out16=_FakeDev(torch.zeros(10, dtype=torch.int16)))
            with pytest.raises(TypeError, match="overflow must be torch.uint8"):
                f(dw, y=y, out16=_FakeDev(torch.zeros(64, dtype=torch.int16)),
                  overflow=_FakeDev(torch.zeros(2, dtype=torch.int8)))
            with pytest.raises(ValueError, match="overflow holds 1 elements, needs 2"):
                f(dw, y=y, out16=_FakeDev(torch.zeros(64, dtype=torch.int16)),
                  overflow=_FakeDev(torch.zeros(1, dtype=torch.uint8)))
    for dt in X16:
        y = _FakeDev(torch.zeros(64, dtype=dt))
        with pytest.raises(ValueError, match="V must be > 0"):
            wire.finish(dw, 9, 0, y=y, want_out16=False)
        with pytest.raises(ValueError, match="V must be >= 1"):
            wire.finish_blk(dw, kb, 0, y=y, want_out16=False)
        with pytest.raises(ValueError, match="kblk must be a device .* no CPU fallback"):
            wire.finish_blk(dw, torch.zeros(2, dtype=torch.int8), 32, y=y, want_out16=False)
        with pytest.raises(ValueError, match="kblk holds 1 elements, needs 2"):
            wire.finish_blk(dw, _FakeDev(torch.zeros(1, dtype=torch.int8)), 32, y=y, want_out16=False)


def test_ops_and_ef_wire_calls_still_refuse_16_bit_tensors():
    from ina_amd import ef, ops
    kb = _FakeDev(torch.zeros(2, dtype=torch.int8))
    r = _FakeDev(torch.zeros(64))
    for dt in X16:
        x = _FakeDev(torch.zeros(64, dtype=dt))
        with pytest.raises(TypeError, match="quantize_i16_wire takes float32 only"):
            ops.quantize_i16_wire(x, 9)
        with pytest.raises(ValueError, match=f"block scales take fp32 buckets: x is {dt}"):
            ops.quantize_i16_wire_blk(x, kb, 32)
        with pytest.raises(ValueError, match=f"block scales take fp32 buckets: y is {dt}"):
            ops.i16_wire_finish_blk(_FakeDev(torch.zeros(64, dtype=torch.int32)), kb, 32, y=x)
        with pytest.raises(TypeError, match="y must be torch.float32"):
            ops.i16_wire_finish(_FakeDev(torch.zeros(64, dtype=torch.int32)), 9, 32, y=x, want_out16=False)
        for f in (lambda: ef.quantize_i16_wire(x, r, 9), lambda: ef.quantize_i16_wire_blk(x, r, kb, 32)):
            with pytest.raises(ValueError, match=f"the sharded int16 wire takes fp32 buckets: x is {dt}"):
                f()


def test_aggregators_take_out_dtype_and_refuse_any_other():
    import inspect
    from ina_amd.dist import RangeAggregator, ShardedAggregator
    cpu = torch.device("cpu")
    for cls in (ShardedAggregator, RangeAggregator):
        assert inspect.signature(cls.__init__).parameters["out_dtype"].default is torch.float32
        for bad in (torch.float64, torch.int16, torch.int32, "bf16", None):
            with pytest.raises(ValueError, match="out_dtype must be torch.float32, torch.bfloat16 or torch.float16"):
                cls(1000, k=9, wire="i16", V=32, device=cpu, out_dtype=bad)
        for wire in ("i16", "i32"):
            for k in (9, "block"):
                agg = cls(1000, k=k, wire=wire, V=32, device=cpu)
                assert agg.out_dtype is torch.float32 and agg.full.dtype == torch.float32
                assert agg.f_shard.dtype == torch.float32
                for dt in X16:
                    agg = cls(1000, k=k, wire=wire, V=32, device=cpu, out_dtype=dt)
                    assert agg.out_dtype is dt and agg.full.dtype == dt and agg.f_shard.dtype == dt
                    assert agg.gather_bytes == 0                              # one rank: nothing gathered
