"""Shared pieces of tests/test_gpu_scratch_reuse.py, and -- run as a program -- its child
process: the stale-flag case of the switch's sort scratch under known epochs.

The switch (csrc/ina_switch.hip) tags its control words and per-wave key flags with the call's
epoch instead of clearing them; epochs count 1, 2, 3, ... per process, one per call past the
one-workgroup paths.  The child makes no switch call before its loop, so call j runs under
epoch j.  Before every call it fills every 32-bit word of the scratch with F: call F meets key
flags, control words and key arrays that all equal its own epoch.  Usage:
    python tests/_scratch_reuse.py F packed|split
"""
import os
import sys

import numpy as np
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
for _p in (TESTS, REPO, os.path.join(REPO, "distributed-training-ina_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import oracle as orc                                    # noqa: E402
from test_gpu_local import rr_batch, split_of                       # noqa: E402
from test_gpu_runs import runs_batch, worker_major                  # noqa: E402

DEV = "cuda:0"
W = 8
# bulk kinds (any size past one workgroup) and the two one-workgroup kinds
BULK = ("in_order", "runs", "runs_acks", "near40", "near1500", "shuffled", "digits")
ONE_WG, TINY = 90, 12          # slots' worth: 720 packets (<= 768), 96 packets (<= key 15's 128)


def ops():
    from ina_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def make_batch(rng, kind, V, per, seq0, num_slots, stride):
    """W = 8 senders x `per` slots from seq0 on, arriving as `kind` says."""
    if kind in ("runs", "runs_acks"):
        return runs_batch(rng, V, worker_major(W, per, seq0, acks=kind == "runs_acks"), W, stride,
                          num_slots=num_slots)
    J = {"in_order": 0, "near40": 40, "near1500": 1500, "shuffled": 1 << 30, "digits": 1 << 30,
         "one_wg": 40, "tiny": 40}[kind]
    return rr_batch(rng, V, W, per, seq0, num_slots, stride, J)


def expected_paths(pk, num_slots, kind, per, seq0):
    """The paths a batch may take, from the batch alone (ina_switch.hip's definitions): None for
    the one-workgroup paths (they write no control words), "sorted" under the digit passes, no
    descent of the slot keys = "in_order", else at most kRunsMax = 64 breaks = "runs", else the
    lists or the sort.  Jitter 40 over at least 1,000 slots that do not wrap the pool is the shape
    whose path the jitter tests of test_gpu_local.py assert as "local"."""
    if len(pk) <= 768:
        return None
    if kind == "digits":
        return {"sorted"}
    idx = pk[:, 6:10].astype(np.int64)
    idx = (idx[:, 0] << 24) | (idx[:, 1] << 16) | (idx[:, 2] << 8) | idx[:, 3]
    mine = pk[:, 10] == 1
    ack = (pk[:, 5] & orc.FLAG_ACK) != 0
    key = np.where(mine, idx % num_slots, num_slots)
    if not (key[1:] < key[:-1]).any():
        return {"in_order"}
    brk = 1 + int((~mine[1:] | (key[:-1] + 1 != key[1:]) | (ack[1:] != ack[:-1])).sum())
    if brk <= 64:
        return {"runs"}
    if kind == "near40" and per >= 1000 and seq0 + per <= num_slots:
        return {"local"}
    return {"local", "sorted"}


def reg_views(ref):
    """The oracle's registers without the copy orc.Switch.registers() makes (2^20 x 32 words)."""
    import ctypes as C
    st = ref._st
    cnt = np.ctypeslib.as_array(C.cast(st.count, C.POINTER(C.c_uint8)), (ref.num_slots,))
    frag = np.ctypeslib.as_array(C.cast(st.frag, C.POINTER(C.c_uint32)), (ref.num_slots,))
    regs = np.ctypeslib.as_array(C.cast(st.regs, C.POINTER(C.c_uint32)), (ref.num_slots, ref.V))
    return cnt, frag, regs


def run_batch(o, sw, pk, V, mode, side=None):
    """One batch through the device switch in `mode`; returns (actions, rows) on the host."""
    d = dev(pk)
    desc = None if mode == "packed_nodesc" else o.nga_descriptors(d)
    if mode == "split":
        hdr, pay = split_of(d, V)
        act = sw.process_split(hdr, pay, desc=desc)
        d[:, :15] = hdr[:, :15]
        d[:, 15:15 + 4 * V] = pay
    elif mode == "two_phase":
        act = torch.empty(len(pk), dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            sw.sort(d, desc, actions=act)
        sw.run(d, act)
    else:
        act = sw.process(d, desc=desc)
    return host(act), host(d)


def check_rows(got_act, got_pk, want_act, want_pk, write_dropped, tag):
    assert np.array_equal(got_act, want_act), tag
    rows = slice(None) if write_dropped else want_act != orc.ACT_DROP
    assert np.array_equal(got_pk[rows], want_pk[rows]), tag


def check_regs(sw, want, hi, tag):
    """count, frag and regs of slots [0, hi) against the oracle's (cnt, frag, regs)."""
    cnt, frag, regs = want
    assert np.array_equal(host(sw.count[:hi]), cnt[:hi]), tag
    assert np.array_equal(host(sw.frag[:hi]).view(np.uint32), frag[:hi]), tag
    assert np.array_equal(host(sw.regs[:hi]).view(np.uint32), regs[:hi]), tag


def main():
    F, split = int(sys.argv[1]), sys.argv[2] == "split"
    o = ops()
    V, num_slots = 32, 1 << 17
    assert 0 < F < num_slots          # a key read from unwritten scratch is then a valid slot
    stride = o.nga_stride(V)
    rng = np.random.default_rng(300 + F)
    sw = o.Switch(V, num_slots=num_slots, switch_id=1, device=DEV, write_dropped=not split)
    ref = orc.Switch(V, num_slots=num_slots, switch_id=1)
    need = o.load().ina_switch_scratch_bytes(W * 2000, num_slots)
    words = torch.empty((need + 3) // 4, dtype=torch.int32, device=DEV)
    sw._scratch = words.view(torch.uint8)
    local = 0
    for j in range(1, 17):                                  # call j runs under epoch j
        per = 1000 + 60 * j                                 # 1,060 .. 1,960 slots
        J = 40 if j % 2 else 1500
        pk = rr_batch(rng, V, W, per, 1 + 7 * j, num_slots, stride, J)
        want_pk, want_act = ref.run(pk, stride=stride)
        words.fill_(F)
        # Batches this small take 1,024-packet sort chunks, i.e. units of 512 packets, and jitter
        # 1500 then makes every unit's window 512 + 1,500 packets: past the lists' scan budget
        # (kLocBeta = 3 x the batch), so the batch would sort.  4,096-packet chunks (tuning key 13;
        # no switch call, no epoch) give units of 2,048: windows of 1.7 x, the lists.  A detection
        # wave then covers 256 packets = 32 slots + the jitter's 187: past kKeysSpanMin, it stores.
        if J == 1500:
            o.set_tuning(switch_sort_rounds=16)
        try:
            got_act, got_pk = run_batch(o, sw, pk, V, "split" if split else "packed")
        finally:
            o.set_tuning(switch_sort_rounds=0)
        assert sw._scratch.data_ptr() == words.data_ptr()
        path = sw.batch_path(len(pk))
        print(f"call {j}: {len(pk)} packets, path {path}", flush=True)
        assert path == "local", (j, path)
        local += 1
        check_rows(got_act, got_pk, want_act, want_pk, not split, j)
        check_regs(sw, reg_views(ref), num_slots, j)
    assert local == 16
    print(f"scratch reuse child ok: F={F} {'split' if split else 'packed'} local 16/16")


if __name__ == "__main__":
    main()
