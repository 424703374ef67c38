"""The block-scaled fused switch + PS step's surface and argument checks (include/ina_switch_blk.h),
with no GPU: the header declares exactly the one function, ina.h includes it after ina_pkt_blk.h, the
symbol is exported and bound, its table is disjoint from the other four, every refusal ina_switch
makes for a PS step (and a null ps or kblk) comes back as INA_EINVAL with its message before any
device work, an empty batch is a no-op, a run alone with no sort recorded is refused, and the Python
layer refuses CPU tensors, non-int8 and short scale arrays and 16-bit buckets."""
import ctypes
import os
import re

import pytest
import torch

FAKE = 1 << 20            # an aligned address that is never touched


def _call(batch=True, ps=True, kblk=FAKE, phase=0, V=32, npkts=4, split=False, ack_stride=0, local=FAKE,
          acks=None, ack_desc=None, stride=144):
    from ina_amd import _lib
    lib = _lib.load()
    st = _lib.SwitchState(16384, V, 1, 0, FAKE, FAKE, FAKE)
    b = _lib.SwitchBatch(FAKE, FAKE if split else None, npkts, stride, None, FAKE, FAKE)
    p = _lib.SwitchPs(1, 0, 0.5, local, FAKE, 4 * 32, acks, ack_stride, ack_desc, 1)
    rc = lib.ina_switch_blk(ctypes.byref(st), ctypes.byref(b) if batch else None, ctypes.byref(p) if ps else None,
                            kblk, phase, None)
    return rc, lib.ina_last_error_string()


def _einval(msg, **kw):
    from ina_amd import _lib
    rc, err = _call(**kw)
    assert rc == _lib.INA_EINVAL and msg in err, (kw, rc, err)


def test_header_declares_the_one_and_it_is_exported_and_bound():
    from ina_amd import _lib
    from tests.conftest import REPO
    src = open(os.path.join(REPO, "include", "ina_switch_blk.h")).read()
    ina_h = open(os.path.join(REPO, "include", "ina.h")).read()
    assert ina_h.index('#include "ina_pkt_blk.h"') < ina_h.index('#include "ina_switch_blk.h"')
    assert "#ifndef INA_PKT_BLK_H\n#error" in src                       # not on its own
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(ina_\w+)\s*\(", code, flags=re.M))
    assert declared == {"ina_switch_blk"} == set(_lib.SIGNATURES_SWITCH_BLK)
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_X16) | set(_lib.SIGNATURES_BLK) | set(_lib.SIGNATURES_PKT_BLK)
    assert not declared & others
    for h in ("ina.h", "ina_x16.h", "ina_blk.h", "ina_pkt_blk.h"):         # declared nowhere else
        other = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", h)).read(), flags=re.S)
        assert not re.search(r"\bina_switch_blk\s*\(", other), h
    fn = getattr(_lib.load(), "ina_switch_blk")
    assert list(fn.argtypes) == _lib.SIGNATURES_SWITCH_BLK["ina_switch_blk"] and fn.restype is ctypes.c_int
    # ina_switch_ps_t keeps its layout
    assert [f[0] for f in _lib.SwitchPs._fields_] == ["seq0", "k", "weight_step", "local", "out", "n", "acks",
                                                      "ack_stride", "ack_desc", "keep_forwarded"]


@pytest.mark.parametrize("phase", [0, 1, 2])
def test_null_batch_ps_and_kblk_are_einval_in_every_phase(phase):
    _einval(b"null batch", batch=False, phase=phase)
    _einval(b"null ps", ps=False, phase=phase)
    _einval(b"null kblk", kblk=None, phase=phase)
    _einval(b"null ps", ps=False, phase=phase, npkts=0)               # before the empty batch's no-op
    _einval(b"null kblk", kblk=None, phase=phase, npkts=0)


@pytest.mark.parametrize("phase", [3, -1, 7])
def test_bad_phase_is_einval(phase):
    _einval(b"phase must be", phase=phase)


def test_what_ina_switch_refuses_for_a_ps_step_is_refused():
    _einval(b"split rows: the ack rows are header rows", split=True, ack_stride=32, acks=FAKE)
    _einval(b"split rows: the ack rows are header rows", split=True, ack_stride=8)
    for V in (6, 30):
        _einval(b"the PS step needs V % 4 == 0", V=V, stride=16 * 10)
    _einval(b"local/out must be 16-byte aligned", local=FAKE + 4)
    _einval(b"ack descriptors need ack rows", ack_desc=FAKE)
    _einval(b"ack rows must be 16-byte aligned", acks=FAKE, ack_stride=24)
    _einval(b"null pointer", local=None)


def test_empty_batch_is_a_no_op():
    from ina_amd import _lib
    for phase in (0, 1, 2):
        for split in (False, True):
            rc, err = _call(npkts=0, phase=phase, split=split)
            assert rc == _lib.INA_OK, (phase, split, err)


def test_run_alone_with_no_sort_recorded_is_einval():
    _einval(b"run alone: no sort of this batch", phase=2)
    _einval(b"run alone: no sort of this batch", phase=2, split=True, stride=16)


class _FakeDev(torch.Tensor):
    """A CPU tensor that says it is on the device, so the checks behind _req's device test are
    reached without a GPU.  Nothing is ever launched on it: every use below ends in an error."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


class _NoState:
    """Switch's methods over a bare object: no device state is made, and no call gets as far as it."""
    V, num_slots = 32, 16384


def _methods(local, k):
    from ina_amd import ops
    V = 32
    pk = _FakeDev(torch.zeros((8, 144), dtype=torch.uint8))
    act = _FakeDev(torch.zeros(8, dtype=torch.uint8))
    hdr, pay = _FakeDev(torch.zeros((8, 16), dtype=torch.uint8)), _FakeDev(torch.zeros((8, 4 * V), dtype=torch.uint8))
    sw = _NoState()
    sw._ps_scale = lambda loc, kk: ops.Switch._ps_scale(sw, loc, kk)
    return [lambda: ops.Switch.process_apply(sw, pk, 1, local, k, 0.5),
            lambda: ops.Switch.process_apply_split(sw, hdr, pay, 1, local, k, 0.5),
            lambda: ops.Switch.run_apply(sw, pk, act, 1, local, k, 0.5)]


def test_ops_refuse_cpu_tensors_bad_scales_and_16bit_buckets():
    V = 32
    n = 3 * V + 5                                                     # 4 slots
    x = _FakeDev(torch.zeros(n))
    good = _FakeDev(torch.zeros(4, dtype=torch.int8))
    for f in _methods(torch.zeros(n), good):                          # a CPU bucket
        with pytest.raises(ValueError, match="no CPU fallback"):
            f()
    for f in _methods(x, torch.zeros(4, dtype=torch.int8)):           # CPU scales
        with pytest.raises(ValueError, match="no CPU fallback"):
            f()
    for f in _methods(x, _FakeDev(torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(TypeError, match="kblk must be torch.int8"):
            f()
    for f in _methods(x, _FakeDev(torch.zeros(3, dtype=torch.int8))):
        with pytest.raises(ValueError, match="kblk holds 3 elements, needs 4"):
            f()
    for dt in (torch.bfloat16, torch.float16):
        for f in _methods(_FakeDev(torch.zeros(n, dtype=dt)), good):
            with pytest.raises(ValueError, match="block scales take fp32 buckets"):
                f()
