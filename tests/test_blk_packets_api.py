"""The block-scaled packet entry points' surface and argument checks (include/ina_pkt_blk.h), with
no GPU: the header declares exactly the three functions, they are exported and bound, null
pointers, a bad mode, a bad degree and a V the sibling refuses come back as INA_EINVAL with their
message before any device work, n == 0 is a no-op, the Python layer refuses CPU tensors, 16-bit
dtypes and short or non-int8 scale arrays, and loopback.agree_block_scales returns the element-wise
MIN to every peer."""
import ctypes
import os
import re
import socket
import threading

import pytest
import torch

FAKE = 1 << 20            # an aligned address that is never touched

NAMES = {"ina_quantize_pack_nga_blk_desc", "ina_quantize_pack_nga_multi_split_blk", "ina_apply_completed_nga_blk"}


def _calls(n=64, V=32, W=2, degree=2, mode=1, kblk=FAKE, bufs=FAKE, rows=FAKE, pay=FAKE, num_slots=16384,
           stride=None, prm=True):
    """name -> argument tuple over fake aligned pointers, for the three entry points."""
    from ina_amd import _lib
    arr = _lib.ptr_array([bufs] * max(W, 1))
    out = _lib.ptr_array([rows] * max(W, 1))
    one = _lib.NgaParams(1, W & 0xFF, 0, 1, 0, 1, num_slots, V)
    many = (_lib.NgaParams * max(W, 1))(*[_lib.NgaParams(w + 1, W & 0xFF, 0, 1, 0, 1, num_slots, V)
                                          for w in range(max(W, 1))])
    stride = (15 + 4 * max(V, 0) + 15) // 16 * 16 if stride is None else stride
    return {
        "ina_quantize_pack_nga_blk_desc": (bufs, None, n, kblk, ctypes.byref(one) if prm else None, rows, stride,
                                           None, None),
        "ina_quantize_pack_nga_multi_split_blk": (arr, W, None, n, kblk, mode, degree, many if prm else None, out,
                                                  out, None, None),
        "ina_apply_completed_nga_blk": (rows, None, 4, V, stride, FAKE, 1, bufs, kblk, 0.5, FAKE, n, None, 0, None),
        "ina_apply_completed_nga_blk/split": (rows, pay, 4, V, 16, FAKE, 1, bufs, kblk, 0.5, FAKE, n, None, 0, None),
    }


def _einval(name, msg, **kw):
    from ina_amd import _lib
    lib = _lib.load()
    assert getattr(lib, name.split("/")[0])(*_calls(**kw)[name]) == _lib.INA_EINVAL, (name, kw)
    assert msg in lib.ina_last_error_string(), (name, kw, lib.ina_last_error_string())


def test_header_declares_the_three_and_they_are_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    src = open(os.path.join(REPO, "include", "ina_pkt_blk.h")).read()
    ina_h = open(os.path.join(REPO, "include", "ina.h")).read()
    assert ina_h.index('#include "ina_blk.h"') < ina_h.index('#include "ina_pkt_blk.h"')
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == NAMES == set(_lib.SIGNATURES_PKT_BLK)
    assert not set(_lib.SIGNATURES_PKT_BLK) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16) | set(_lib.SIGNATURES_BLK))
    lib = _lib.load()
    for n in declared:
        fn = getattr(lib, n)
        assert list(fn.argtypes) == _lib.SIGNATURES_PKT_BLK[n] and fn.restype is ctypes.c_int, n


def test_null_pointers_are_einval():
    _einval("ina_quantize_pack_nga_blk_desc", b"null pointer", bufs=None)
    _einval("ina_quantize_pack_nga_blk_desc", b"null pointer", kblk=None)
    _einval("ina_quantize_pack_nga_blk_desc", b"null pointer", rows=None)
    _einval("ina_quantize_pack_nga_blk_desc", b"bad nga params", prm=False)
    for mode in (0, 1):
        _einval("ina_quantize_pack_nga_multi_split_blk", b"null kblk", kblk=None, mode=mode)
        _einval("ina_quantize_pack_nga_multi_split_blk", b"null worker buffer", bufs=None, mode=mode)
        _einval("ina_quantize_pack_nga_multi_split_blk", b"null worker buffer", rows=None, mode=mode)
        _einval("ina_quantize_pack_nga_multi_split_blk", b"non-null", prm=False, mode=mode)
    for name in ("ina_apply_completed_nga_blk", "ina_apply_completed_nga_blk/split"):
        _einval(name, b"null pointer", kblk=None)
        _einval(name, b"null pointer", bufs=None)            # local
    _einval("ina_apply_completed_nga_blk", b"null pointer", rows=None)


@pytest.mark.parametrize("mode", [2, -1, 7])
def test_bad_mode_is_einval(mode):
    _einval("ina_quantize_pack_nga_multi_split_blk", b"mode must be", mode=mode)


def test_bad_degree_is_einval_under_scale_fors_rule():
    from ina_amd import _lib
    for degree in (0, -3):
        _einval("ina_quantize_pack_nga_multi_split_blk", b"degree", degree=degree)
    # 2147483647 / degree - 1/2 <= 0 from degree = 2^32 on; an int reaches 2^31 - 1, which passes
    k = ctypes.c_int(0)
    assert _lib.load().ina_scale_for(1.0, 2147483647, 32, ctypes.byref(k)) == _lib.INA_OK
    # a given scale array ignores degree
    lib = _lib.load()
    assert lib.ina_quantize_pack_nga_multi_split_blk(*_calls(n=0, mode=0, degree=0)[
        "ina_quantize_pack_nga_multi_split_blk"]) == _lib.INA_OK


@pytest.mark.parametrize("V", [0, -4, 6, 260])
def test_v_the_sibling_refuses_is_einval(V):
    _einval("ina_quantize_pack_nga_multi_split_blk", b"split rows need V", V=V)
    _einval("ina_apply_completed_nga_blk", b"V must be a multiple of 4", V=V, stride=2048)
    _einval("ina_apply_completed_nga_blk/split", b"V must be a multiple of 4", V=V)
    if V <= 0:
        _einval("ina_quantize_pack_nga_blk_desc", b"bad nga params", V=V)


def test_geometry_the_siblings_refuse_is_einval():
    _einval("ina_quantize_pack_nga_blk_desc", b"stride < 15 + 4V", stride=64)
    _einval("ina_quantize_pack_nga_blk_desc", b"bad nga params", num_slots=0)
    _einval("ina_apply_completed_nga_blk", b"stride", stride=150)
    _einval("ina_apply_completed_nga_blk", b"stride", stride=64)
    _einval("ina_apply_completed_nga_blk/split", b"split rows", rows=FAKE + 4)
    for W in (0, -1, 65):
        _einval("ina_quantize_pack_nga_multi_split_blk", b"W in [1, 64]", W=W)


def test_empty_bucket_is_a_no_op():
    from ina_amd import _lib
    lib = _lib.load()
    for kw in (dict(n=0), dict(n=0, kblk=None, bufs=None, rows=None)):
        for name, args in _calls(**kw).items():
            if name == "ina_quantize_pack_nga_multi_split_blk" and kw.get("rows", FAKE) is None:
                continue                                               # its pointer arrays hold the nulls
            assert getattr(lib, name.split("/")[0])(*args) == _lib.INA_OK, (name, kw, lib.ina_last_error_string())


def test_ops_refuse_cpu_tensors_16bit_dtypes_and_bad_scales():
    from ina_amd import ops
    V = 32
    x = torch.zeros(64)
    kb = torch.zeros(2, dtype=torch.int8)
    pk = torch.zeros((2, 144), dtype=torch.uint8)
    act = torch.zeros(2, dtype=torch.uint8)
    calls = [
        lambda t, k: ops.quantize_pack_nga_blk(t, k, V, 1, 2, 1, 1),
        lambda t, k: ops.quantize_pack_nga_blk(_FakeDev(torch.zeros(64)), k, V, 1, 2, 1, 1, base=t),
        lambda t, k: ops.quantize_pack_nga_multi_split_blk([t, t], V, [1, 2], 2, 1, 1, kblk=k),
        lambda t, k: ops.quantize_pack_nga_multi_split_blk([t, t], V, [1, 2], 2, 1, 1),
    ]
    for f in calls:
        with pytest.raises(ValueError, match="no CPU fallback"):
            f(x, kb)
        for dt in (torch.bfloat16, torch.float16):
            with pytest.raises(ValueError, match="block scales take fp32 buckets"):
                f(x.to(dt), kb)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.apply_completed_blk(pk, act, V, 1, x, kb, 0.5)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match="block scales take fp32 buckets"):
            ops.apply_completed_blk(_FakeDev(pk), _FakeDev(act), V, 1, x.to(dt), kb, 0.5)
    with pytest.raises(ValueError, match="V must be"):
        ops.quantize_pack_nga_blk(x, kb, 0, 1, 2, 1, 1)
    with pytest.raises(ValueError, match="degree"):
        ops.quantize_pack_nga_multi_split_blk([_FakeDev(x)], V, [1], 1, 1, 1, degree=0)


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind _req's device test are
    reached without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def test_ops_refuse_short_and_non_int8_scales():
    from ina_amd import ops
    V = 32
    x = _FakeDev(torch.zeros(3 * V + 5))                              # 4 packets
    pk, act = _FakeDev(torch.zeros((8, 144), dtype=torch.uint8)), _FakeDev(torch.zeros(8, dtype=torch.uint8))
    short, wrong = _FakeDev(torch.zeros(3, dtype=torch.int8)), _FakeDev(torch.zeros(4, dtype=torch.int32))
    for f in (lambda k: ops.quantize_pack_nga_blk(x, k, V, 1, 2, 1, 1),
              lambda k: ops.quantize_pack_nga_multi_split_blk([x, x], V, [1, 2], 2, 1, 1, kblk=k),
              lambda k: ops.quantize_pack_nga_multi_split_blk([x, x], V, [1, 2], 2, 1, 1, kblk_out=k),
              lambda k: ops.apply_completed_blk(pk, act, V, 1, x, k, 0.5, out=_FakeDev(torch.zeros(3 * V + 5)))):
        with pytest.raises(ValueError, match="kblk holds 3 elements, needs 4"):
            f(short)
        with pytest.raises(TypeError, match="kblk must be torch.int8"):
            f(wrong)
    # the size checks of _check_apply: a short actions array, out of another size, too few ack rows
    kb = _FakeDev(torch.zeros(4, dtype=torch.int8))
    with pytest.raises(ValueError, match="actions must hold one byte per packet"):
        ops.apply_completed_blk(pk, _FakeDev(torch.zeros(7, dtype=torch.uint8)), V, 1, x, kb, 0.5)
    with pytest.raises(ValueError, match="out must have local's size"):
        ops.apply_completed_blk(pk, act, V, 1, x, kb, 0.5, out=_FakeDev(torch.zeros(3 * V + 9)))
    with pytest.raises(ValueError, match="one row per slot"):
        ops.apply_completed_blk(pk, act, V, 1, x, kb, 0.5, acks=_FakeDev(torch.zeros((3, 16), dtype=torch.uint8)))
    with pytest.raises(ValueError, match="shorter than 15"):
        ops.apply_completed_blk(_FakeDev(torch.zeros((8, 128), dtype=torch.uint8)), act, V, 1, x, kb, 0.5)
    with pytest.raises(ValueError, match="pay must be a contiguous uint8"):
        ops.apply_completed_blk(_FakeDev(torch.zeros((8, 16), dtype=torch.uint8)), act, V, 1, x, kb, 0.5,
                                pay=_FakeDev(torch.zeros((7, 4 * V), dtype=torch.uint8)))


def test_agree_block_scales_returns_the_min_to_every_peer():
    from ina_amd import loopback
    W, nblk = 3, 37
    g = torch.Generator().manual_seed(5)
    mine = [torch.randint(-126, 128, (nblk,), generator=g, dtype=torch.int32).to(torch.int8) for _ in range(W)]
    pairs = [socket.socketpair() for _ in range(W)]
    for a, b in pairs:
        a.settimeout(20)
        b.settimeout(20)
    got, errs = [None] * W, []

    def worker(w):
        try:
            got[w] = loopback.agree_block_scales(pairs[w][1], mine[w])
        except Exception as e:          # noqa: BLE001 -- reported below
            errs.append(e)

    ths = [threading.Thread(target=worker, args=(w,), daemon=True) for w in range(W)]
    for t in ths:
        t.start()
    try:
        agreed = loopback.agree_block_scales([a for a, _ in pairs])
        for t in ths:
            t.join(20)
        assert not errs and not any(t.is_alive() for t in ths), errs
    finally:
        for a, b in pairs:
            a.close()
            b.close()
    want = torch.stack(mine).amin(dim=0)
    assert agreed.dtype == torch.int8 and torch.equal(agreed, want)
    for w in range(W):
        assert got[w].dtype == torch.int8 and torch.equal(got[w], want), w
