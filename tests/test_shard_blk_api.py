"""The block-scaled int16 wire's surface and argument checks (include/ina_shard_blk.h), with no GPU:
the header declares exactly the two functions, refuses a lone include and is included by ina.h after
ina_switch_blk.h; the names are in SIGNATURES_SHARD_BLK and in no other table or header, exported and
bound; null kblk, null buffers and V <= 0 come back as INA_EINVAL with their messages before any
device work and n == 0 is a no-op; the ops wrappers refuse CPU tensors, 16-bit buckets, non-int8 and
short scale arrays; and the aggregators refuse chunks > 1 with k="block" and an unknown string for k
before they touch a device or a process group."""
import ctypes
import os
import re

import pytest
import torch

FAKE = 1 << 20            # an aligned address that is never touched
NAMES = {"ina_quantize_blk_f32_i16_wire", "ina_i16_wire_finish_blk"}


def _quant(x=FAKE, kblk=FAKE, V=32, wire=FAKE, n=64):
    from ina_amd import _lib
    lib = _lib.load()
    return lib.ina_quantize_blk_f32_i16_wire(x, kblk, V, wire, n, None), lib.ina_last_error_string()


def _finish(wsum=FAKE, n=64, kblk=FAKE, V=32, out16=FAKE, y=FAKE, ovf=FAKE):
    from ina_amd import _lib
    lib = _lib.load()
    return lib.ina_i16_wire_finish_blk(wsum, n, kblk, V, out16, y, ovf, None), lib.ina_last_error_string()


def _einval(call, msg, **kw):
    from ina_amd import _lib
    rc, err = call(**kw)
    assert rc == _lib.INA_EINVAL and msg in err, (call.__name__, kw, rc, err)


def test_header_declares_the_two_and_they_are_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    inc = os.path.join(REPO, "include")
    src = open(os.path.join(inc, "ina_shard_blk.h")).read()
    ina_h = open(os.path.join(inc, "ina.h")).read()
    assert ina_h.index('#include "ina_switch_blk.h"') < ina_h.index('#include "ina_shard_blk.h"')
    assert "#ifndef INA_SWITCH_BLK_H\n#error" in src                      # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == NAMES == set(_lib.SIGNATURES_SHARD_BLK)
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16) | set(_lib.SIGNATURES_BLK) |
              set(_lib.SIGNATURES_PKT_BLK) | set(_lib.SIGNATURES_SWITCH_BLK))
    assert not declared & others
    for h in sorted(os.listdir(inc)):                                     # declared nowhere else
        if h == "ina_shard_blk.h":
            continue
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
        for name in NAMES:
            assert not re.search(rf"\b{name}\s*\(", other), (h, name)
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SIGNATURES_SHARD_BLK[name] and fn.restype is ctypes.c_int, name
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    # (x, kblk, V, wire, n, stream) and (wire_sum, n, kblk, V, out16, y, overflow_per_slot, stream)
    assert _lib.SIGNATURES_SHARD_BLK["ina_quantize_blk_f32_i16_wire"] == [vp, vp, i, vp, sz, vp]
    assert _lib.SIGNATURES_SHARD_BLK["ina_i16_wire_finish_blk"] == [vp, sz, vp, i, vp, vp, vp, vp]


def test_lone_include_is_refused_by_the_preprocessor(tmp_path):
    import shutil
    import subprocess
    from tests.conftest import REPO
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    c = tmp_path / "lone.c"
    c.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "ina_shard_blk.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode != 0 and "include ina.h" in r.stderr
    c.write_text('#include "ina.h"\nint main(void) { return ina_i16_wire_finish_blk(0, 0, 0, 1, 0, 0, 0, 0); }\n')
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("V", [0, -1, -256])
def test_v_below_one_is_einval(V):
    _einval(_quant, b"V must be >= 1", V=V)
    _einval(_finish, b"V must be >= 1", V=V)
    _einval(_quant, b"V must be >= 1", V=V, n=0)                         # before the empty call's no-op
    _einval(_finish, b"V must be >= 1", V=V, n=0)


@pytest.mark.parametrize("V", [32, 100, 1])
def test_null_kblk_and_null_buffers_are_einval_before_any_device_work(V):
    _einval(_quant, b"null kblk", kblk=None, V=V)
    _einval(_finish, b"null kblk", kblk=None, V=V)
    _einval(_quant, b"null kblk", kblk=None, x=None, V=V)                # kblk is looked at first
    _einval(_quant, b"null pointer", x=None, V=V)
    _einval(_quant, b"null pointer", wire=None, V=V)
    _einval(_finish, b"null pointer", wsum=None, V=V)


def test_empty_call_is_a_no_op_even_with_null_pointers():
    from ina_amd import _lib
    for V in (32, 100):
        rc, err = _quant(x=None, kblk=None, wire=None, n=0, V=V)
        assert rc == _lib.INA_OK, err
        rc, err = _finish(wsum=None, kblk=None, out16=None, y=None, ovf=None, n=0, V=V)
        assert rc == _lib.INA_OK, err


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind _req's device test are
    reached without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def _wrappers(x, w, k, V=32):
    from ina_amd import ops
    return [lambda: ops.quantize_i16_wire_blk(x, k, V), lambda: ops.i16_wire_finish_blk(w, k, V)]


def test_ops_refuse_cpu_tensors_bad_scales_and_16bit_buckets():
    from ina_amd import ops
    V = 32
    n = 3 * V + 5                                                         # 4 blocks
    x, w = _FakeDev(torch.zeros(n)), _FakeDev(torch.zeros(n, dtype=torch.int32))
    good = _FakeDev(torch.zeros(4, dtype=torch.int8))
    for f in _wrappers(torch.zeros(n), torch.zeros(n, dtype=torch.int32), good):       # CPU buckets
        with pytest.raises(ValueError, match="no CPU fallback"):
            f()
    for f in _wrappers(x, w, torch.zeros(4, dtype=torch.int8)):                        # CPU scales
        with pytest.raises(ValueError, match="no CPU fallback"):
            f()
    for f in _wrappers(x, w, _FakeDev(torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(TypeError, match="kblk must be torch.int8"):
            f()
    for f in _wrappers(x, w, _FakeDev(torch.zeros(3, dtype=torch.int8))):
        with pytest.raises(ValueError, match="kblk holds 3 elements, needs 4"):
            f()
    for f in _wrappers(x, w, good, V=0):
        with pytest.raises(ValueError, match="V must be >= 1"):
            f()
    for dt in (torch.bfloat16, torch.float16):
        x16 = _FakeDev(torch.zeros(n, dtype=dt))
        with pytest.raises(ValueError, match="block scales take fp32 buckets"):
            ops.quantize_i16_wire_blk(x16, good, V)
        with pytest.raises(ValueError, match="block scales take fp32 buckets"):
            ops.i16_wire_finish_blk(w, good, V, y=x16)
        with pytest.raises(ValueError, match="block scales take fp32 buckets"):
            ops.i16_wire_finish_blk(x16, good, V)


def test_aggregators_refuse_chunks_and_unknown_k_before_any_device_or_group_use():
    from ina_amd.dist import RangeAggregator, ShardedAggregator
    dev = torch.device("cpu")                  # never reached: the refusals come first
    for wire in ("i16", "i32"):
        with pytest.raises(ValueError, match="whole bucket's MIN"):
            ShardedAggregator(1000, k="block", chunks=2, wire=wire, V=32, device=dev)
        for k in ("blocks", "auto", ""):
            with pytest.raises(ValueError, match="k must be an integer or 'block'"):
                ShardedAggregator(1000, k=k, wire=wire, V=32, device=dev)
            with pytest.raises(ValueError, match="k must be an integer or 'block'"):
                RangeAggregator(1000, k=k, wire=wire, V=32, device=dev)


def test_agree_block_scales_is_the_identity_on_one_rank_and_takes_int8_only():
    from ina_amd.dist import agree_block_scales
    kb = torch.tensor([-126, 0, 5, 127], dtype=torch.int8)
    assert agree_block_scales(kb) is kb and kb.tolist() == [-126, 0, 5, 127]
    with pytest.raises(TypeError, match="torch.int8"):
        agree_block_scales(torch.zeros(4, dtype=torch.int32))
