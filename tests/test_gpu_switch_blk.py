"""GPU parity of the fused switch + PS step with per-block scales (include/ina_switch_blk.h;
Switch.process_apply / process_apply_split / run_apply with an int8 tensor for k), bit for bit.

The yardstick is never the code under test: oracle.Switch.run gives actions, registers and the
rewritten rows, _blk_ref.ps_apply of the oracle's integer sums gives `out` on the completed slots
of the bucket.  `out` is sentinel-filled and a few elements longer than the result: slots that did
not complete, and the tail, stay untouched.  Ack rows and their descriptors do not depend on k, so
they equal what the global-k call writes for the same batch.  Equality with process[_split]()
followed by apply_completed_blk() is a second check.

Scales: _blk_ref.kblk_ref of the bucket (magnitude-varied blocks, so neighbouring slots differ and a
wrong slot index shows) with the first three slots forced to 127, -128 (read as -126) and -126.
Every batch carries n = V * per - 3 (a ragged last slot: the value-by-value tail), packets whose
frag id lies past the bucket (completed, forwarded, not consumed), and -- where the path under test
allows them -- collisions, other degrees and foreign packets at tests/test_gpu_local.rr_batch's rates.
The shapes are the smallest that reach each PS site, taken from the tests that pin those paths."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _blk_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0xA5
SENT_F = np.float32(-777.5)
PAST = 3                    # slots packed past the PS's bucket
WRAP = 0xFFFFFFFE           # the sequence numbers wrap inside the bucket


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ina_amd import ops  # noqa: F401


def ops():
    from ina_amd import ops as o
    return o


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sentinel(shape, dtype=torch.uint8):
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((int(np.prod(shape)) * size,), SENT, dtype=torch.uint8, device=DEV).view(dtype).reshape(shape)


class Case:
    """One batch, its scales and what the oracle says of it (computed once, never changed)."""

    def __init__(self, V, W, per, order, pool, seq0, seed, **kw):
        # two completions of one PS slot in one batch (a collision's frag id on a packet that
        # completes by its own degree) leave `out` to chance on every path, the two-call form
        # included: such a draw is not a case, the next seed is
        while not self._build(V, W, per, order, pool, seq0, seed, **kw):
            seed += 1000

    def _build(self, V, W, per, order, pool, seq0, seed, jitter=0, acks=False, noise=True):
        o = ops()
        self.V, self.W, self.per, self.pool, self.seq0 = V, W, per, pool, seq0
        self.n = n = V * per - 3
        self.stride = stride = o.nga_stride(V)
        rng = np.random.default_rng(seed)
        nbig = (per + PAST) * V
        xs = R.bucket(rng, W, nbig, V)
        self.local = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        kbig = R.kblk_ref(xs, V, W, 32)
        kbig[:3] = (127, -128, -126)
        self.kblk = kbig[:per].copy()
        rows = []
        if acks:        # last step's acks in front of each slot's packets (the steady state)
            rows.append(orc.pack_nga(np.zeros(nbig, np.int32), V, 0, W, 1, seq0, flags=orc.FLAG_ACK, num_slots=pool,
                                     stride=stride))
        for w in range(W):
            rows.append(orc.pack_nga(R.quantize_i32(xs[w], kbig, V), V, w + 1, W, 1, seq0, num_slots=pool,
                                     stride=stride))
        K, npk = len(rows), per + PAST
        if order == "worker_major":
            pk = np.concatenate(rows)
        else:                                               # slot-major: slot s, then sender
            pk = np.stack(rows, 1).reshape(K * npk, stride)
            if order == "shuffled":
                pk = pk[rng.permutation(len(pk))]
            elif order == "jitter":
                pk = pk[np.argsort(np.arange(len(pk)) + rng.integers(0, jitter, len(pk)), kind="stable")]
        pk = pk.copy()
        if noise:
            m = len(pk)
            for i in np.flatnonzero(rng.random(m) < 0.02):                     # collisions
                f = int.from_bytes(pk[i, 11:15].tobytes(), "big") + 1
                pk[i, 11:15] = np.frombuffer((f & 0xFFFFFFFF).to_bytes(4, "big"), np.uint8)
            for i in np.flatnonzero(rng.random(m) < 0.02):                     # another degree
                pk[i, 4] = int(rng.choice([1, 2]))
            # foreign packets (another switch id) sort behind every slot: each one breaks an in-order
            # or dense-run batch, so only the shuffled batches carry them
            for i in np.flatnonzero(rng.random(m) < (0.01 if order == "shuffled" else 0.0)):
                pk[i, 10] = 2
        self.pk = np.ascontiguousarray(pk)
        ref = orc.Switch(V, num_slots=pool, switch_id=1)
        self.rew, self.act = ref.run(self.pk, stride=stride)
        self.regs = ref.registers()
        done = self.act == orc.ACT_FWD_AGG
        f, vals = orc.unpack_nga(self.rew[done], V, stride)
        slot = (f["frag_id"].astype(np.int64) - seq0) & 0xFFFFFFFF
        take = slot < per
        if len(np.unique(slot[take])) != int(take.sum()):
            return False
        assert take.any() and not take.all()                   # consumed ones, and ones past the bucket
        self.consumed = np.zeros(len(pk), bool)
        self.consumed[np.flatnonzero(done)[take]] = True
        sums = np.zeros(per * V, np.int32)
        hit = np.zeros(per * V, bool)
        idx = (slot[take][:, None] * V + np.arange(V)[None, :]).ravel()
        sums[idx] = vals.reshape(-1, V)[take].ravel()
        hit[idx] = True
        self.hit, self.sums = hit[:n], sums[:n]
        return True

    ws = 1.0 / 9

    def want_out(self, kblk, untouched=SENT_F):
        return np.where(self.hit, R.ps_apply(self.local, self.sums, kblk, self.V, self.ws), untouched)


def split_of(pk, V):
    hdr = np.zeros((len(pk), 16), np.uint8)
    hdr[:, :15] = pk[:, :15]
    return hdr, np.ascontiguousarray(pk[:, 15:15 + 4 * V])


def fused(c, split, k, keep_forwarded=True, write_dropped=False, two_phase=False, sw=None):
    """One fused call over a fresh switch (k: an int or the int8 scales); everything it wrote."""
    o, V, per = ops(), c.V, c.per
    sw = sw or o.Switch(V, num_slots=c.pool, switch_id=1, device=DEV, write_dropped=write_dropped)
    d = dev(c.pk)
    desc = o.nga_descriptors(d)
    buf = torch.full((c.n + 5,), float(SENT_F), device=DEV)
    acks = sentinel((per + 2, 16 if split else c.stride))
    ad = sentinel((per + 2,), torch.int64)
    local = dev(c.local)
    if split:
        assert not two_phase
        hd, pa = split_of(c.pk, V)
        hdr, pay = dev(hd), dev(pa)
        act, _ = sw.process_apply_split(hdr, pay, c.seq0, local, k, c.ws, out=buf[:c.n], ack_hdr=acks, ack_desc=ad,
                                        keep_forwarded=keep_forwarded, desc=desc)
        rows = np.concatenate([host(hdr)[:, :15], host(pay)], 1)
    else:
        if two_phase:
            act = sw.sort(d, desc)
            sw.run_apply(d, act, c.seq0, local, k, c.ws, out=buf[:c.n], acks=acks, keep_forwarded=keep_forwarded,
                         ack_desc=ad)
        else:
            act, _ = sw.process_apply(d, c.seq0, local, k, c.ws, out=buf[:c.n], acks=acks, ack_desc=ad,
                                      keep_forwarded=keep_forwarded, desc=desc)
        rows = host(d)[:, :15 + 4 * V]
    path = sw.batch_path(len(c.pk)) if len(c.pk) > 768 else None
    return dict(act=host(act), out=host(buf), acks=host(acks), ad=host(ad), rows=rows, path=path,
                count=host(sw.count), frag=host(sw.frag).view(np.uint32), regs=host(sw.regs).view(np.uint32))


def two_calls(c, split, kblk, write_dropped=False):
    """What a caller wrote before: the switch, then apply_completed_blk."""
    o, V = ops(), c.V
    sw = o.Switch(V, num_slots=c.pool, switch_id=1, device=DEV, write_dropped=write_dropped)
    buf = torch.full((c.n + 5,), float(SENT_F), device=DEV)
    acks = sentinel((c.per + 2, 16 if split else c.stride))
    if split:
        hd, pa = split_of(c.pk, V)
        hdr, pay = dev(hd), dev(pa)
        act = sw.process_split(hdr, pay)
        o.apply_completed_blk(hdr, act, V, c.seq0, dev(c.local), kblk, c.ws, out=buf[:c.n], acks=acks, pay=pay)
    else:
        d = dev(c.pk)
        act = sw.process(d)
        o.apply_completed_blk(d, act, V, c.seq0, dev(c.local), kblk, c.ws, out=buf[:c.n], acks=acks)
    return host(buf), host(acks)


def check_registers(got, c, tag):
    cnt, frag, regs = c.regs
    assert np.array_equal(got["count"], cnt), tag
    assert np.array_equal(got["frag"], frag), tag
    assert np.array_equal(got["regs"], regs), tag


def check_case(c, split, want_paths=None, write_dropped=False, two_call=True):
    V, n = c.V, c.n
    kblk = dev(c.kblk)
    want = c.want_out(c.kblk)
    glob = fused(c, split, 16, write_dropped=write_dropped)               # the acks' reference: they ignore k
    assert (glob["acks"] != SENT).any() and (glob["ad"].view(np.uint8) != SENT).any()
    wide = 15 + 4 * V
    for keep in (True, False):
        tag = (V, c.W, c.per, split, keep, write_dropped)
        got = fused(c, split, kblk, keep_forwarded=keep, write_dropped=write_dropped)
        if want_paths is not None:
            assert got["path"] in want_paths, (tag, got["path"])
        assert np.array_equal(got["act"], c.act), tag
        assert np.array_equal(got["out"][:n].view(np.uint32), want.view(np.uint32)), tag
        assert (got["out"][n:] == SENT_F).all(), tag
        check_registers(got, c, tag)
        assert np.array_equal(got["acks"], glob["acks"]) and np.array_equal(got["ad"], glob["ad"]), tag
        # rows: the oracle's where the switch writes them; a consumed packet's stay as they arrived
        written = (c.act != orc.ACT_DROP) if not write_dropped else np.ones(len(c.pk), bool)
        if not keep:
            written &= ~c.consumed
            assert np.array_equal(got["rows"][c.consumed], c.pk[c.consumed][:, :wide]), tag
        assert np.array_equal(got["rows"][written], c.rew[written][:, :wide]), tag
    if two_call:
        out2, acks2 = two_calls(c, split, kblk, write_dropped)
        assert np.array_equal(got["out"].view(np.uint32), out2.view(np.uint32))
        if split:
            assert np.array_equal(got["acks"], acks2)
        else:                    # (the apply's packed ack row is the 16 header bytes)
            assert np.array_equal(got["acks"][:, :15], acks2[:, :15])


# ---- the one-launch tiny path (kLat) ----------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("V", [4, 12, 32, 256])
def test_tiny_batches(V, split):
    check_case(Case(V, 3, 30, "shuffled", 16384, WRAP, seed=V + split), split)


# ---- in-order / run table / bucket sort ---------------------------------------------------------------
ORDERS = [("round_robin", 1, {"in_order", "runs"}), ("worker_major", WRAP, {"runs"}), ("shuffled", WRAP, {"sorted"})]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("order,seq0,paths", ORDERS)
@pytest.mark.parametrize("V,W,per", [(256, 8, 700), (64, 4, 300)])
def test_wide_rows(V, W, per, order, seq0, paths, split):
    """run_segment in the wide run kernel."""
    check_case(Case(V, W, per, order, 16384, seq0, seed=V + W + len(order)), split, paths)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("order,seq0,paths", ORDERS)
@pytest.mark.parametrize("V,W,per,pool", [(32, 8, 3000, 1 << 13), (8, 8, 1000, 16384)])
def test_narrow_rows(V, W, per, pool, order, seq0, paths, split):
    """The narrow drivers (window_slots_narrow, runs_slots_narrow), their group_packet and the whole
    segments of seg8_fast."""
    check_case(Case(V, W, per, order, pool, seq0, seed=V + W + len(order)), split, paths)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("V,W,per,pool,order", [(256, 8, 700, 16384, "shuffled"), (32, 8, 3000, 1 << 13, "round_robin")])
def test_write_dropped(V, W, per, pool, order, split):
    check_case(Case(V, W, per, order, pool, 1, seed=3 * V + W), split, write_dropped=True, two_call=False)


# ---- near-sorted lists ---------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_near_sorted_lists(split):
    """tests/test_gpu_local.test_local_ps_fused_equals_sorted's batch (acks in front, jitter 500, 2^20
    slots): the per-slot lists' update, and the same call with the lists off (the bucket sort)."""
    o = ops()
    c = Case(32, 8, 7000, "jitter", 1 << 20, 1, seed=77 + split, jitter=500, acks=True, noise=False)
    check_case(c, split, {"local"})
    try:
        o.set_tuning(switch_local=False)
        srt = fused(c, split, dev(c.kblk))
    finally:
        o.set_tuning(switch_local=True)
    loc = fused(c, split, dev(c.kblk))
    assert srt["path"] == "sorted" and loc["path"] == "local"
    for key in ("act", "out", "acks", "ad", "rows", "count", "frag", "regs"):
        assert np.array_equal(srt[key], loc[key]), key


# ---- sort, then run ----------------------------------------------------------------------------------
@pytest.mark.parametrize("V,W,per,pool", [(256, 8, 700, 16384), (32, 8, 3000, 1 << 13), (32, 3, 30, 16384)])
def test_sort_then_run_apply_gives_the_one_call_result(V, W, per, pool):
    c = Case(V, W, per, "shuffled", pool, WRAP, seed=V + per)
    one = fused(c, False, dev(c.kblk), keep_forwarded=False)
    two = fused(c, False, dev(c.kblk), keep_forwarded=False, two_phase=True)
    assert np.array_equal(one["out"][:c.n].view(np.uint32), c.want_out(c.kblk).view(np.uint32))
    for key in ("act", "out", "acks", "ad", "rows", "count", "frag", "regs"):
        assert np.array_equal(one[key], two[key]), key


def test_run_apply_after_a_sort_of_another_batch_is_refused():
    o = ops()
    c = Case(32, 8, 200, "shuffled", 16384, 1, seed=5)
    sw = o.Switch(32, num_slots=16384, switch_id=1, device=DEV)
    d, other = dev(c.pk), dev(c.pk)
    act = sw.sort(other, o.nga_descriptors(other))
    with pytest.raises(ValueError, match="must follow sort"):
        sw.run_apply(d, act, 1, dev(c.local), dev(c.kblk), c.ws)
    torch.cuda.synchronize()


# ---- all-16 scales are the global-k step -----------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("V,W,per,pool", [(256, 8, 700, 16384), (32, 8, 3000, 1 << 13), (32, 3, 30, 16384)])
def test_all_16_scales_give_the_global_k_call(V, W, per, pool, split):
    c = Case(V, W, per, "round_robin", pool, 1, seed=V + per + 1)
    k16 = torch.full((per,), 16, dtype=torch.int8, device=DEV)
    a, b = fused(c, split, k16), fused(c, split, 16)
    for key in ("act", "out", "acks", "ad", "rows", "count", "frag", "regs"):
        assert np.array_equal(a[key], b[key]), key
    assert (a["out"][:c.n] != SENT_F).any()


# ---- three steady-state steps --------------------------------------------------------------------------
@pytest.mark.parametrize("V,W,per", [(256, 8, 700), (32, 8, 3000), (64, 4, 200), (256, 3, 30)])
def test_steady_state_steps(V, W, per):
    """tests/test_gpu_split.test_process_apply_split_equals_packed's steps with block scales: the
    AUTO multi-worker split pack feeds process_apply_split(k=kblk), the acks of step t in front of
    step t+1's packets.  Per step, against the oracle chain on the very bytes the switch was given:
    actions, the update on completed slots (_blk_ref.ps_apply of the oracle's sums with the pack's
    scales), ack rows and descriptors (the completing packet's header with the ack flag)."""
    o = ops()
    rng = np.random.default_rng(V + W + per)
    n = V * per - 3
    npk = -(-n // V)
    slots = 1 << 13
    xs = [dev(x) for x in R.bucket(rng, W, n, V, lo=-6.0, hi=0.0)]
    glob = dev((rng.standard_normal(n) * 1e-2).astype(np.float32))
    upd = torch.full((n + 5,), float(SENT_F), device=DEV)
    acts = torch.empty((W + 1) * npk, dtype=torch.uint8, device=DEV)
    desc = torch.zeros((W + 1) * npk, dtype=torch.int64, device=DEV)
    hdr = torch.zeros(((W + 1) * npk, 16), dtype=torch.uint8, device=DEV)
    pay = torch.zeros(((W + 1) * npk, 4 * V), dtype=torch.uint8, device=DEV)
    hw, pw = hdr[npk:].view(W, npk, 16), pay[npk:].view(W, npk, 4 * V)
    kblk = torch.empty(npk, dtype=torch.int8, device=DEV)
    sw = o.Switch(V, num_slots=slots, switch_id=1, device=DEV)
    ref = orc.Switch(V, num_slots=slots, switch_id=1)
    stride = 15 + 4 * V
    ws = 1.0 / (W + 1)
    for step in range(3):
        o.quantize_pack_nga_multi_split_blk(xs, V, list(range(1, W + 1)), W, 1, 1, base=glob, num_slots=slots,
                                            hdrs=list(hw.unbind(0)), pays=list(pw.unbind(0)),
                                            descs=list(desc[npk:].view(W, npk).unbind(0)), kblk_out=kblk)
        if step == 0:
            o.nga_descriptors(hdr[:npk], out=desc[:npk])
        given = np.concatenate([host(hdr)[:, :15], host(pay)], 1)
        local, kb = host(glob).copy(), host(kblk).copy()
        sw.process_apply_split(hdr, pay, 1, glob, kblk, ws, out=upd[:n], ack_hdr=hdr[:npk], ack_desc=desc[:npk],
                               keep_forwarded=False, actions=acts, desc=desc)
        rew, act = ref.run(given, stride=stride)
        assert np.array_equal(host(acts), act), step
        done = act == orc.ACT_FWD_AGG
        assert int(done.sum()) == npk, step
        f, vals = orc.unpack_nga(rew[done], V, stride)
        sums = np.zeros(npk * V, np.int32)
        slot = f["frag_id"].astype(np.int64) - 1
        sums[(slot[:, None] * V + np.arange(V)[None, :]).ravel()] = vals
        got = host(upd)
        assert np.array_equal(got[:n].view(np.uint32), R.ps_apply(local, sums[:n], kb, V, ws).view(np.uint32)), step
        assert (got[n:] == SENT_F).all()
        want_ack = np.zeros((npk, 16), np.uint8)
        want_ack[slot, :15] = given[done][:, :15]
        want_ack[:, 5] = orc.FLAG_ACK
        assert np.array_equal(host(hdr[:npk]), want_ack), step
        assert np.array_equal(host(desc[:npk]), np.ascontiguousarray(want_ack[:, 4:12]).view(np.int64).ravel()), step
        glob.copy_(upd[:n])
    cnt, frag, regs = ref.registers()
    assert np.array_equal(host(sw.count), cnt) and np.array_equal(host(sw.frag).view(np.uint32), frag)
    assert np.array_equal(host(sw.regs).view(np.uint32), regs)
