"""GPU parity of the switch over a REUSED sort scratch (csrc/ina_switch.hip).  ina.h promises
that one scratch sized for the largest batch serves every batch and that its contents on entry
are arbitrary: the kernels tag control words, the run table, the near-sorted verdict and the
per-wave key flags with the call's epoch instead of clearing them, and the arrays inside the
scratch sit at offsets that move with the batch size, so a smaller batch's tags land in whatever
a larger batch left there (sorted slot keys, histograms, run starts, packet ids).

1. seeded sequences of batches of changing kind and size over ONE scratch allocation;
2. one batch over a scratch the test pre-fills (zeros, ones, 0x01 bytes, random bytes, the
   leavings of a 72,000-packet shuffled batch);
3. in a child process, where call j runs under epoch j: every scratch word preset to F, so call
   F meets flags and control words equal to its own epoch.

Every expectation is the CPU oracle's P4 restatement with state carried from batch to batch:
actions, rewritten rows, count / frag / regs, and the path each batch took.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc

from _scratch_reuse import (BULK, DEV, ONE_WG, REPO, TINY, W, check_regs, check_rows, dev, expected_paths,
                            host, make_batch, reg_views, run_batch)
from test_gpu_local import rr_batch, split_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ina_amd import ops  # noqa: F401  (fails loudly if libina.so is missing)


def ops():
    from ina_amd import ops as o
    return o


# ---- 1. sequences over one scratch ----------------------------------------------------------
READERS = {"near": ("near40", "near1500"), "in_order": ("in_order",), "runs": ("runs", "runs_acks")}
LARGE, SMALL = (2500, 9000), (100, 1000)          # slots' worth per sender, W = 8 senders


def reader_of(kind):
    return next((r for r, ks in READERS.items() if kind in ks), None)


def build_sequence(seed):
    """[(kind, per)]: first the largest batch (it sizes the scratch) and a shuffled one of 72,000
    packets (sorted keys and packet ids all over the scratch), then every ordered pair
    (bulk kind A, large) -> (B, small) for B among the three paths that read epoch-tagged words
    -- the near-sorted lists, the in-order run, the run table -- in seeded order; each small
    batch is followed by the next pair's large one, so every kind also grows.  A one-workgroup
    and a tiny batch sit between pairs.  Sizes: 8 x {100, 1000} small, 8 x {2500, 9000} large."""
    rng = np.random.default_rng(seed)
    pairs = [(a, b) for a in BULK for b in READERS]
    rng.shuffle(pairs)
    seq = [("runs_acks", 9000), ("shuffled", 9000)]     # 81,000 packets (acks in front): the largest
    extras = {int(x): k for x, k in zip(rng.choice(len(pairs) - 1, 3, replace=False) + 1,
                                        ("one_wg", "tiny", "one_wg"))}
    for i, (a, b) in enumerate(pairs):
        if i in extras:
            seq.append((extras[i], ONE_WG if extras[i] == "one_wg" else TINY))
        bk = READERS[b][int(rng.integers(len(READERS[b])))]
        seq.append((a, LARGE[1] if i % 7 == 3 else LARGE[0]))
        seq.append((bk, SMALL[i % 2]))
    return seq


def check_coverage(seq):
    """The pairs the sequence must hold, asserted so that an edit cannot drop one silently."""
    big = lambda per: per >= LARGE[0]                                   # noqa: E731
    small = lambda per: ONE_WG < per <= SMALL[1]                        # noqa: E731
    pairs = {(a, reader_of(b)) for (a, pa), (b, pb) in zip(seq, seq[1:]) if big(pa) and small(pb)}
    assert pairs >= {(a, b) for a in BULK for b in READERS}, sorted(pairs)
    grows = {b for (a, pa), (b, pb) in zip(seq, seq[1:]) if pa <= SMALL[1] and big(pb)}
    assert grows >= set(BULK), sorted(grows)
    assert {"one_wg", "tiny"} <= {k for k, _ in seq}
    assert {per for _, per in seq} >= set(LARGE) | set(SMALL)
    assert len(seq) >= 12 and seq[0] == ("runs_acks", max(per for _, per in seq))


_SEQ = {}


def sequence_reference(num_slots, V):
    """The sequence's batches and the oracle's results, computed once per (pool, V) and shared by
    the four modes: per batch (kind, per, seq0, rows, want rows, want actions, the oracle's
    registers of slots [0, hi) after it); the oracle itself keeps the final state."""
    key = (num_slots, V)
    if key not in _SEQ:
        _SEQ.clear()                                     # one (pool, V) at a time
        o = ops()
        stride = o.nga_stride(V)
        seq = build_sequence(1000 + num_slots % 991 + V)
        check_coverage(seq)
        rng = np.random.default_rng(7 + num_slots % 977 + V)
        ref = orc.Switch(V, num_slots=num_slots, switch_id=1)
        hi = min(num_slots, 1 << 14)                     # every slot a batch can touch is below it
        steps = []
        for kind, per in seq:
            seq0 = 1 + int(rng.integers(0, 300))
            assert hi == num_slots or seq0 + per <= hi
            pk = make_batch(rng, kind, V, per, seq0, num_slots, stride)
            want_pk, want_act = ref.run(pk, stride=stride)
            regs = tuple(x[:hi].copy() for x in reg_views(ref))
            steps.append((kind, per, seq0, pk, want_pk, want_act, regs))
        _SEQ[key] = (steps, ref, hi)
    return _SEQ[key]


@pytest.mark.parametrize("mode", ["packed", "packed_nodesc", "split", "two_phase"])
@pytest.mark.parametrize("num_slots,V", [(1000, 32), (1 << 17, 32), (1 << 20, 32), (1 << 17, 8)])
def test_sequence_over_one_scratch(num_slots, V, mode):
    """One Switch, one scratch allocation (its pointer asserted after every batch), 47 batches:
    in slot order, dense runs with and without acks in front, near-sorted (jitter 40 / 1500),
    shuffled, the digit passes (tuning key 12 = 3), one-workgroup and tiny batches, 96 to 81,000
    packets, every large -> small pair in front of the three paths that read tagged words.  Packed
    rows with and without descriptors, split rows, and two phases (sort() on a side stream, then
    run(), alternating with one-call batches).  Pools of 1,000, 2^17 and 2^20 slots (one-digit,
    two-digit and wide keys; the 1,000-slot pool wraps under the larger batches) and V = 8."""
    o = ops()
    steps, ref, hi = sequence_reference(num_slots, V)
    wd = mode != "split"
    sw = o.Switch(V, num_slots=num_slots, switch_id=1, device=DEV, write_dropped=wd)
    side = torch.cuda.Stream(DEV) if mode == "two_phase" else None
    ptr = None
    for i, (kind, per, seq0, pk, want_pk, want_act, regs) in enumerate(steps):
        tag = (i, kind, per)
        m = mode if mode != "two_phase" or i % 2 == 0 else "packed"
        if kind == "digits":
            o.set_tuning(switch_sort=3)
        try:
            got_act, got_pk = run_batch(o, sw, pk, V, m, side)
        finally:
            if kind == "digits":
                o.set_tuning(switch_sort=0)
        if ptr is None:
            ptr = sw._scratch.data_ptr()                 # sized by the largest batch, the first
        assert sw._scratch.data_ptr() == ptr, tag
        check_rows(got_act, got_pk, want_act, want_pk, wd, tag)
        want = expected_paths(pk, num_slots, kind, per, seq0)
        if want is not None:
            path = sw.batch_path(len(pk))
            assert path in want, (tag, path, want)
        check_regs(sw, regs, hi, tag)
    check_regs(sw, reg_views(ref), num_slots, "final")   # and nothing outside those slots


@pytest.mark.parametrize("split", [False, True])
def test_fused_ps_steps_over_one_scratch(split):
    """The fused PS step (process_apply / process_apply_split) over one scratch, three steps of
    different n (7,000, 900, 3,000 slots: large, small, large), the steady-state batch (acks in
    front, jitter 500): actions and registers are the oracle's; out, the ack rows and the ack
    descriptors equal the switch followed by apply_completed on a second device switch whose
    scratch is fresh at every step."""
    o = ops()
    V, num_slots = 32, 1 << 20
    stride = o.nga_stride(V)
    rng = np.random.default_rng(55 + split)
    sw = o.Switch(V, num_slots=num_slots, switch_id=1, device=DEV)
    two = o.Switch(V, num_slots=num_slots, switch_id=1, device=DEV)
    ref = orc.Switch(V, num_slots=num_slots, switch_id=1)
    ptr = None
    for step, per in enumerate((7000, 900, 3000)):
        pk = rr_batch(rng, V, W, per, 1, num_slots, stride, 500, acks=True, collide=0, degree_mix=0)
        n = per * V - 5
        local = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
        _, want_act = ref.run(pk, stride=stride)
        # the two-step reference
        d2 = dev(pk)
        two._scratch = None
        act2 = two.process(d2, desc=o.nga_descriptors(d2))
        out2 = torch.full_like(local, float("nan"))
        acks2 = torch.zeros((per, stride), dtype=torch.uint8, device=DEV)
        o.apply_completed(d2, act2, V, 1, local, 16, 1 / 9, out=out2, acks=acks2)
        # fused, over the reused scratch
        d = dev(pk)
        desc = o.nga_descriptors(d)
        out = torch.full_like(local, float("nan"))
        acks = torch.zeros((per, 16 if split else stride), dtype=torch.uint8, device=DEV)
        ad = torch.zeros(per, dtype=torch.int64, device=DEV)
        if split:
            hdr, pay = split_of(d, V)
            act, _ = sw.process_apply_split(hdr, pay, 1, local, 16, 1 / 9, out=out, ack_hdr=acks, ack_desc=ad,
                                            desc=desc)
        else:
            act, _ = sw.process_apply(d, 1, local, 16, 1 / 9, out=out, acks=acks, ack_desc=ad, desc=desc)
        if ptr is None:
            ptr = sw._scratch.data_ptr()
        assert sw._scratch.data_ptr() == ptr, step
        assert np.array_equal(host(act), want_act), step
        assert np.array_equal(host(act2), want_act), step
        assert int((want_act == orc.ACT_FWD_AGG).sum()) > 0
        assert sw.batch_path(len(pk)) in ("local", "sorted"), step
        assert np.array_equal(host(out).view(np.uint32), host(out2).view(np.uint32)), step
        assert np.array_equal(host(acks)[:, :15], host(acks2)[:, :15]), step
        assert np.array_equal(host(ad), host(o.nga_descriptors(acks2))), step
        check_regs(sw, reg_views(ref), 1 << 14, step)
    check_regs(sw, reg_views(ref), num_slots, "final")


# ---- 2. results do not depend on what the scratch held --------------------------------------
FILLS = ("zeros", "ones", "bytes01", "random", "left_by_72000_shuffled")
_LEFT = {}


def left_scratch(o, num_slots):
    """The scratch as a 72,000-packet shuffled batch over slots 0..8999 leaves it."""
    if num_slots not in _LEFT:
        V, stride = 32, o.nga_stride(32)
        sw = o.Switch(V, num_slots=num_slots, switch_id=1, device=DEV)
        pk = rr_batch(np.random.default_rng(72), V, W, 9000, 0, num_slots, stride, 1 << 30)
        d = dev(pk)
        sw.process(d, desc=o.nga_descriptors(d))
        assert sw.batch_path(len(pk)) == "sorted"
        _LEFT[num_slots] = sw._scratch.clone()
    return _LEFT[num_slots]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("num_slots", [1 << 17, 1 << 20])
@pytest.mark.parametrize("kind", ["in_order", "runs", "near40", "near1500", "shuffled"])
def test_prefilled_scratch(kind, num_slots, split):
    """One batch of 8 x 2,000 NGA-32 packets from a fresh state over a scratch holding 0x00, 0xFF,
    0x01 bytes, seeded random bytes, or what a 72,000-packet shuffled batch left: the oracle's
    results and the same path under every fill."""
    o = ops()
    V, per, seq0 = 32, 2000, 1
    stride = o.nga_stride(V)
    rng = np.random.default_rng(len(kind) + num_slots % 97 + 3 * split)
    pk = make_batch(rng, kind, V, per, seq0, num_slots, stride)
    ref = orc.Switch(V, num_slots=num_slots, switch_id=1)
    want_pk, want_act = ref.run(pk, stride=stride)
    want_paths = expected_paths(pk, num_slots, kind, per, seq0)
    left = left_scratch(o, num_slots)
    nbytes = left.numel()
    assert nbytes >= o.load().ina_switch_scratch_bytes(len(pk), num_slots)
    paths = []
    for fill in FILLS:
        if fill == "left_by_72000_shuffled":
            buf = left.clone()
        elif fill == "random":
            g = torch.Generator(device=DEV).manual_seed(9)
            buf = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=DEV, generator=g)
        else:
            buf = torch.full((nbytes,), {"zeros": 0, "ones": 255, "bytes01": 1}[fill], dtype=torch.uint8,
                             device=DEV)
        sw = o.Switch(V, num_slots=num_slots, switch_id=1, device=DEV, write_dropped=not split)
        sw._scratch = buf
        got_act, got_pk = run_batch(o, sw, pk, V, "split" if split else "packed")
        assert sw._scratch.data_ptr() == buf.data_ptr(), fill
        check_rows(got_act, got_pk, want_act, want_pk, not split, fill)
        path = sw.batch_path(len(pk))
        assert path in want_paths, (fill, path, want_paths)
        paths.append(path)
        check_regs(sw, reg_views(ref), 1 << 12, fill)
        assert np.array_equal(host(sw.count), reg_views(ref)[0]), fill
    assert len(set(paths)) == 1, paths


# ---- 3. the stale-flag case under known epochs ----------------------------------------------
@pytest.mark.parametrize("F,rows", [(8, "packed"), (9, "split")])
def test_stale_flags_equal_to_the_epoch(F, rows):
    """A fresh process, where call j of the switch runs under epoch j: 16 near-sorted batches
    (W = 8, 1,060-1,960 slots, V = 32, pool 2^17, descriptors, one call; jitter 40 on odd calls,
    1500 on even ones, those with 4,096-packet sort chunks: with the 1,024-packet chunks of so
    small a batch jitter 1500 exceeds the lists' scan budget and sorts), every scratch word preset to F before each call, each batch against the
    oracle and its path "local" -- tests/_scratch_reuse.py.  Call F meets key flags equal to its
    own epoch.  Before the detection pass wrote every wave's flag (k_sort_chunks: it used to
    write a flag only where the wave stored its keys, i.e. found a descent over a span of more
    than kKeysSpanMin = 128 slots) this could not pass: under jitter 40 (F = 9) no wave spans
    128 slots, so no flag and no key was written, k_local_lists found every flag of every unit's
    window equal to the epoch, took 'the stored keys throughout' and read F for every packet;
    under jitter 1500 (F = 8) the waves that did not store left the same."""
    cmd = [sys.executable, os.path.join(REPO, "tests", "_scratch_reuse.py"), str(F), rows]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert f"scratch reuse child ok: F={F} {rows} local 16/16" in r.stdout
    assert r.stdout.count("path local") == 16
