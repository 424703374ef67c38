"""Error feedback for the quantiser: the surface and the argument checks (include/ina_ef.h, ina_amd.ef),
with no GPU.  The header declares exactly the nine functions, refuses a lone include and sits right
before ina_x16_blk.h, which stays ina.h's last include; the names are in SIGNATURES_EF and in no other
table or header, exported and bound; a null resid, k out of range, a bad mode, a bad type code and a
degree that fails ina_scale_for's rule come back as INA_EINVAL before any device work and n == 0 is a
no-op; ina_amd.ef refuses CPU tensors, other dtypes and mismatched residuals by name."""
import ctypes
import os
import re

import pytest
import torch

FAKE = 1 << 20            # an aligned address that is never touched

GLOBAL = ("ina_quantize_ef_f32_i32", "ina_quantize_ef_f32_i16_sat")
X16 = ("ina_quantize_ef_x16_i32", "ina_quantize_ef_x16_i16_sat")
SCALES = "ina_block_scales_ef_f32"
BLK = ("ina_quantize_ef_blk_f32_i32", "ina_quantize_ef_blk_f32_i16_sat")
PACK, PACK_BLK = "ina_quantize_pack_nga_multi_split_ef", "ina_quantize_pack_nga_multi_split_ef_blk"
NAMES = set(GLOBAL + X16 + BLK + (SCALES, PACK, PACK_BLK))


def _calls(n=64, k=10, V=32, W=2, degree=2, bits=32, mode=1, xtype=1, kblk=FAKE, resid=FAKE, x=FAKE):
    """name -> argument tuple over fake aligned pointers, for every entry point."""
    from ina_amd import _lib
    nw = max(W, 1)
    xs = _lib.ptr_array([x] * nw)
    rs = _lib.ptr_array([resid] * nw) if resid is not None else None
    rows = _lib.ptr_array([FAKE] * nw)
    prm = (_lib.NgaParams * nw)(*[_lib.NgaParams(1, 2, 0, 1, 0, 1, 16384, V)] * nw)
    return {
        "ina_quantize_ef_f32_i32": (x, None, resid, FAKE, n, k, None),
        "ina_quantize_ef_f32_i16_sat": (x, None, resid, FAKE, n, k, V, None, None),
        "ina_quantize_ef_x16_i32": (x, xtype, None, resid, FAKE, n, k, None),
        "ina_quantize_ef_x16_i16_sat": (x, xtype, None, resid, FAKE, n, k, V, None, None),
        SCALES: (xs, rs, W, None, n, V, degree, bits, kblk, None),
        "ina_quantize_ef_blk_f32_i32": (x, None, resid, kblk, mode, degree, V, FAKE, n, None),
        "ina_quantize_ef_blk_f32_i16_sat": (x, None, resid, kblk, mode, degree, V, FAKE, n, None, None),
        PACK: (xs, rs, W, None, n, k, prm, rows, rows, None, None),
        PACK_BLK: (xs, rs, W, None, n, kblk, mode, degree, prm, rows, rows, None, None),
    }


def _einval(name, msg, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    assert getattr(lib, name)(*_calls(**kw)[name]) == _lib.INA_EINVAL, (name, kw)
    assert msg in lib.ina_last_error_string(), (name, kw, lib.ina_last_error_string())


def test_header_declares_the_nine_and_they_are_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_ef.h")).read()
    includes = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(inc, "ina.h")).read(), flags=re.M)
    assert includes[-2:] == ["ina_ef.h", "ina_x16_blk.h"] and includes.count("ina_ef.h") == 1
    assert re.search(r"#ifndef INA_\w+_H\n#error", src)                                    # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert len(NAMES) == 9 and declared == NAMES == set(_lib.SIGNATURES_EF) == set(_calls())
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16) | set(_lib.SIGNATURES_BLK) |
              set(_lib.SIGNATURES_PKT_BLK) | set(_lib.SIGNATURES_SWITCH_BLK) | set(_lib.SIGNATURES_SHARD_BLK) |
              set(_lib.SIGNATURES_BLK_X16))
    assert not declared & others
    for h in sorted(os.listdir(inc)):                                                      # declared nowhere else
        if h == "ina_ef.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SIGNATURES_EF[name] and fn.restype is ctypes.c_int, name
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    S = _lib.SIGNATURES_EF
    # (x, base, resid, q, n, k[, V, overflow], stream), the 16-bit ones with xtype after x
    assert S["ina_quantize_ef_f32_i32"] == [vp, vp, vp, vp, sz, i, vp]
    assert S["ina_quantize_ef_f32_i16_sat"] == [vp, vp, vp, vp, sz, i, i, vp, vp]
    assert S["ina_quantize_ef_x16_i32"] == [vp, i, vp, vp, vp, sz, i, vp]
    assert S["ina_quantize_ef_x16_i16_sat"] == [vp, i, vp, vp, vp, sz, i, i, vp, vp]
    # (xs, resids, W, base, n, V, degree, bits, kblk, stream)
    assert S[SCALES] == [vp, vp, i, vp, sz, i, i, i, vp, vp]
    # (x, base, resid, kblk, mode, degree, V, q, n[, overflow], stream)
    assert S["ina_quantize_ef_blk_f32_i32"] == [vp, vp, vp, vp, i, i, i, vp, sz, vp]
    assert S["ina_quantize_ef_blk_f32_i16_sat"] == [vp, vp, vp, vp, i, i, i, vp, sz, vp, vp]
    # the siblings' arguments with the W residual pointers after the buckets
    for name, sib in ((PACK, _lib.SIGNATURES["ina_quantize_pack_nga_multi_split"]),
                      (PACK_BLK, _lib.SIGNATURES_PKT_BLK["ina_quantize_pack_nga_multi_split_blk"])):
        assert S[name] == sib[:1] + [vp] + sib[1:], name
    assert lib.ina_version() == b"ina-mi355x 0.2 (gfx950)"


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_ef.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { return ina_quantize_ef_f32_i32(0, 0, 0, 0, 0, 1, 0); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_resid_is_einval():
    for name in NAMES:
        for mode in (0, 1):
            _einval(name, b"null resid", resid=None, mode=mode)
    # a null entry of the residual array, and a misaligned one on the packs
    from ina_amd import _lib
    lib = _lib.load()
    for name in (SCALES, PACK, PACK_BLK):
        args = list(_calls()[name])
        args[1] = _lib.ptr_array([FAKE, None])
        assert getattr(lib, name)(*args) == _lib.INA_EINVAL, name
        assert b"null" in lib.ina_last_error_string()
    for name in (PACK, PACK_BLK):
        args = list(_calls()[name])
        args[1] = _lib.ptr_array([FAKE, FAKE + 4])
        assert getattr(lib, name)(*args) == _lib.INA_EINVAL, name
        assert b"16-byte aligned" in lib.ina_last_error_string()


@pytest.mark.parametrize("k", [-127, 128, 500])
def test_k_out_of_range_is_einval(k):
    for name in GLOBAL + X16 + (PACK,):
        _einval(name, b"k out of range", k=k)
        _einval(name, b"k out of range", k=k, n=0)                      # before the empty call's no-op


def test_bad_mode_type_code_v_and_w_are_einval():
    for mode in (2, -1, 7):
        for name in BLK + (PACK_BLK,):
            _einval(name, b"mode", mode=mode)
    for xtype in (0, 3):
        for name in X16:
            _einval(name, b"INA_X16_BF16 (1) or INA_X16_F16 (2)", xtype=xtype)
            _einval(name, b"INA_X16_BF16", xtype=xtype, n=0)
    for V in (0, -1):
        for name in ("ina_quantize_ef_f32_i16_sat", "ina_quantize_ef_x16_i16_sat", SCALES) + BLK:
            _einval(name, b"V must be", V=V)
        for name in (PACK, PACK_BLK):
            _einval(name, b"V a multiple of 4", V=V)
    for W in (0, -1, 65):
        _einval(SCALES, b"W must be", W=W)
        for name in (PACK, PACK_BLK):
            _einval(name, b"W in [1, 64]", W=W)
    _einval("ina_quantize_ef_x16_i32", b"2-byte aligned", x=FAKE + 1)


def test_degree_follows_ina_scale_for():
    for degree in (0, -3):
        for name in BLK + (SCALES, PACK_BLK):
            _einval(name, b"degree", degree=degree, mode=1)
    # too many summands for 16 bits: 32767 / degree - 1/2 <= 0
    for degree in (65534, 70000):
        _einval(SCALES, b"degree", degree=degree, bits=16)
        _einval("ina_quantize_ef_blk_f32_i16_sat", b"degree", degree=degree, mode=1)
    for bits in (0, 8, 31, 64):
        _einval(SCALES, b"bits", bits=bits)
    # given scales: degree is ignored
    from ina_amd import _lib
    lib = _lib.load()
    for name in BLK + (PACK_BLK,):
        assert getattr(lib, name)(*_calls(degree=0, mode=0, n=0)[name]) == _lib.INA_OK, name


def test_null_scales_and_buffers_are_einval():
    for name in BLK + (SCALES, PACK_BLK):
        for mode in (0, 1):
            _einval(name, b"null", kblk=None, mode=mode)
    for name in NAMES:
        _einval(name, b"null", x=None)


def test_empty_bucket_is_a_no_op():
    from ina_amd import _lib
    lib = _lib.load()
    for name, args in _calls(n=0).items():
        assert getattr(lib, name)(*args) == _lib.INA_OK, name
    for name, args in _calls(n=0, resid=None, x=None).items():          # nothing is looked at
        assert getattr(lib, name)(*args) == _lib.INA_OK, name


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind _req's device test are
    reached without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def _ef_calls():
    from ina_amd import ef
    kb = _FakeDev(torch.zeros(2, dtype=torch.int8))
    return [
        lambda x, r: ef.quantize(x, r, 10),
        lambda x, r: ef.quantize_i16(x, r, 10, 32),
        lambda x, r: ef.block_scales([x], [r], 32),
        lambda x, r: ef.quantize_blk(x, r, 32),
        lambda x, r: ef.quantize_i16_blk(x, r, 32, kblk=kb),
        lambda x, r: ef.quantize_pack_nga_multi_split([x, x], [r, r], 10, 32, [1, 2], 2, 1, 1),
        lambda x, r: ef.quantize_pack_nga_multi_split([x, x], [r, r], None, 32, [1, 2], 2, 1, 1),
    ]


def test_ef_is_exported_and_refuses_by_name_before_any_device_call():
    import ina_amd
    from ina_amd import ef
    assert ina_amd.ef is ef
    x, r = torch.zeros(64), torch.zeros(64)
    for f in _ef_calls():
        with pytest.raises(ValueError, match="no CPU fallback"):
            f(x, r)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ef.new_residual(x)
    dx, dr = _FakeDev(x), _FakeDev(r)
    for f in _ef_calls():
        with pytest.raises(TypeError, match="must be torch.float32"):
            f(_FakeDev(torch.zeros(64, dtype=torch.float64)), dr)
        with pytest.raises(TypeError, match="resid.* must be torch.float32"):
            f(dx, _FakeDev(torch.zeros(64, dtype=torch.bfloat16)))
        with pytest.raises(ValueError, match="resid.* holds 63 elements"):
            f(dx, _FakeDev(torch.zeros(63)))
    # 16-bit buckets: the global-k quantisers take them, the block-scaled calls and the packs say no
    for dt in (torch.bfloat16, torch.float16):
        h = _FakeDev(torch.zeros(64, dtype=dt))
        for f in _ef_calls()[2:]:
            with pytest.raises(ValueError, match=f"takes fp32 buckets: .* is {dt}"):
                f(h, dr)
        with pytest.raises(TypeError, match="base must be torch.float32"):
            ef.quantize(h, dr, 10, base=h)
    with pytest.raises(ValueError, match="one residual per bucket"):
        ef.block_scales([dx, dx], [dr], 32)
    with pytest.raises(ValueError, match="V must be"):
        ef.block_scales([dx], [dr], 0)
    with pytest.raises(ValueError, match="degree"):
        ef.block_scales([dx], [dr], 32, bits=16, degree=65534)
    with pytest.raises(TypeError, match="k must be an int"):
        ef.quantize_pack_nga_multi_split([dx], [dr], 1.5, 32, [1], 1, 1, 1)


def test_loopback_defaults_keep_error_feedback_off():
    import inspect
    from ina_amd import loopback
    assert inspect.signature(loopback.worker_send).parameters["residual"].default is None
    assert inspect.signature(loopback.worker_serve).parameters["error_feedback"].default is False
