"""GPU parity of the block-scaled packet entry points (include/ina_pkt_blk.h) against the CPU
oracle, bit for bit.  The yardstick is never the code under test: payload values are
_blk_ref.quantize_i32 of the fp32 deltas, row bytes oracle.pack_nga (split rows: its first 15 bytes
plus a zero byte, and its payload bytes), scales _blk_ref.kblk_ref, the update _blk_ref.ps_apply of
the oracle switch's integer sums.  Outputs are sentinel-filled and a few elements longer than the
result; what lies past the result must stay untouched."""
import os
import socket
import tempfile
import threading

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import _blk_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0xA5
NUM_SLOTS = 16384
VS = [8, 32, 128, 256, 12]            # 12: no vector AUTO layout
NS = ["3V+5", "V-3", "4V"]            # a ragged short last packet, one short packet, whole packets


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


def n_of(kind, V):
    return {"3V+5": 3 * V + 5, "V-3": V - 3, "4V": 4 * V}[kind]


def sentinel(shape, dtype=torch.uint8):
    """A device tensor whose every byte is SENT."""
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((int(np.prod(shape)) * size,), SENT, dtype=torch.uint8, device=DEV).view(dtype).reshape(shape)


def given_scales(rng, xs, base, V, W):
    """Neighbouring packets with very different scales: 127, one given as -128 (packs as -126), -126,
    then what the data asks for."""
    k = R.kblk_ref(xs, V, W, 32, base=base)
    for i, v in enumerate((127, -128, -126)):
        if i < k.size - 1:
            k[i] = v
    return k


def ref_rows(x, base, kblk, V, bitmap, count, seq0, stride=None, switch_id=1):
    d = (np.asarray(x, np.float32) - base).astype(np.float32) if base is not None else x
    return orc.pack_nga(R.quantize_i32(d, kblk, V), V, bitmap, count, switch_id, seq0, num_slots=NUM_SLOTS,
                        stride=stride)


def split_of(rows, V):
    hdr = np.zeros((len(rows), 16), np.uint8)
    hdr[:, :15] = rows[:, :15]
    return hdr, np.ascontiguousarray(rows[:, 15:15 + 4 * V])


def desc_of(rows):
    return np.ascontiguousarray(rows[:, 4:12]).view(np.int64).ravel()


def bucket(seed, W, n, V):
    rng = np.random.default_rng(seed)
    xs = R.bucket(rng, W, n, V)
    base = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    return rng, xs, base


# ---- packs, scales given ----------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["aligned", "odd-stride", "unaligned-x"])
@pytest.mark.parametrize("kind", NS)
@pytest.mark.parametrize("V", VS)
def test_packed_pack_given(V, kind, layout):
    o, n = ops(), n_of(kind, V)
    rng, xs, base = bucket(V * 7 + len(kind), 1, n, V)
    kblk = given_scales(rng, xs, base, V, 1)
    npk = kblk.size
    stride = 15 + 4 * V if layout == "odd-stride" else o.nga_stride(V)
    seq0 = 0xFFFFFFFE                                   # the sequence numbers wrap inside the bucket
    if layout == "unaligned-x":
        x = torch.empty(n + 1, dtype=torch.float32, device=DEV)[1:]
        x.copy_(dev(xs[0]))
        assert x.data_ptr() % 16 == 4
    else:
        x = dev(xs[0])
    for b in (None, base):
        out, d = sentinel((npk + 2, stride)), sentinel((npk + 3,), torch.int64)
        got, gd = o.quantize_pack_nga_blk(x, dev(kblk), V, 3, 5, 1, seq0, base=None if b is None else dev(b),
                                          num_slots=NUM_SLOTS, stride=stride, out=out, desc=d)
        want = ref_rows(xs[0], b, kblk, V, 3, 5, seq0, stride)
        got, gd = host(got), host(gd)
        assert np.array_equal(got[:npk], want), (V, kind, layout)
        assert (got[npk:] == SENT).all()
        assert np.array_equal(gd[:npk], desc_of(want)) and (gd[npk:].view(np.uint8) == SENT).all()
    # a scale given as -128 / -127 packs as -126
    if npk >= 4:
        k2 = kblk.copy()
        k2[1] = -127
        assert np.array_equal(host(o.quantize_pack_nga_blk(x, dev(k2), V, 3, 5, 1, seq0, num_slots=NUM_SLOTS,
                                                           stride=stride)),
                              ref_rows(xs[0], None, kblk, V, 3, 5, seq0, stride))


def _multi_split(o, xs, base, V, W, seq0, **kw):
    npk = -(-xs.shape[1] // V)
    hdrs = [sentinel((npk + 2, 16)) for _ in range(W)]
    pays = [sentinel((npk + 2, 4 * V)) for _ in range(W)]
    descs = [sentinel((npk + 3,), torch.int64) for _ in range(W)]
    r = o.quantize_pack_nga_multi_split_blk([dev(x) for x in xs], V, list(range(1, W + 1)), W, 1, seq0,
                                            base=dev(base), num_slots=NUM_SLOTS, hdrs=hdrs, pays=pays, descs=descs,
                                            **kw)
    return [[host(t) for t in r[i]] for i in range(3)], r[3]


def _check_split(got, xs, base, kblk, V, W, seq0):
    npk = kblk.size
    for w in range(W):
        want = ref_rows(xs[w], base, kblk, V, w + 1, W, seq0)
        wh, wp = split_of(want, V)
        h, p, d = got[0][w], got[1][w], got[2][w]
        assert np.array_equal(h[:npk], wh) and (h[npk:] == SENT).all(), w
        assert np.array_equal(p[:npk], wp) and (p[npk:] == SENT).all(), w
        assert np.array_equal(d[:npk], desc_of(want)) and (d[npk:].view(np.uint8) == SENT).all(), w


@pytest.mark.parametrize("W", [1, 3, 8, 9])             # 9 crosses a pack group
@pytest.mark.parametrize("kind", NS)
@pytest.mark.parametrize("V", VS)
def test_multi_split_pack_given(V, kind, W):
    o, n = ops(), n_of(kind, V)
    rng, xs, base = bucket(V * 11 + W, W, n, V)
    kblk = given_scales(rng, xs, base, V, W)
    got, k = _multi_split(o, xs, base, V, W, 7, kblk=dev(kblk))
    assert np.array_equal(host(k), kblk)                 # a given array is read, never written
    _check_split(got, xs, base, kblk, V, W, 7)


# ---- packs, scales computed ---------------------------------------------------------------------
def special_packets(xs, base, V):
    """Packet 0 all-zero deltas (-> 127), packet 1 holds inf (-> -126), packet 2 holds a NaN (ignored),
    packet 3 subnormal deltas only -- where the bucket has them."""
    n = xs.shape[1]
    xs[:, :min(V, n)] = base[:min(V, n)]
    if n > V + 1:
        xs[0, V + 1] = np.inf
    if n > 2 * V + 3:
        xs[-1, 2 * V + 3] = np.nan
    if n > 3 * V:
        base[3 * V:4 * V] = 0
        xs[:, 3 * V:4 * V] = np.float32(1e-40) * np.arange(1, xs[:, 3 * V:4 * V].shape[1] + 1, dtype=np.float32)


@pytest.mark.parametrize("deg", ["W", 16])
@pytest.mark.parametrize("W", [1, 3, 8, 9])
@pytest.mark.parametrize("kind", NS)
@pytest.mark.parametrize("V", VS)
def test_multi_split_pack_auto(V, kind, W, deg):
    o, n = ops(), n_of(kind, V)
    degree = W if deg == "W" else 16
    rng, xs, base = bucket(V * 13 + W, W, n, V)
    special_packets(xs, base, V)
    with np.errstate(invalid="ignore"):
        want_k = R.kblk_ref(xs, V, degree, 32, base=base)
    npk = want_k.size
    if npk >= 4:
        assert want_k[0] == 127 and want_k[1] == -126 and want_k[3] > 100
    kout = sentinel((npk + 3,), torch.int8)
    got, k = _multi_split(o, xs, base, V, W, 7, degree=degree, kblk_out=kout)
    k = host(k)
    assert np.array_equal(k[:npk], want_k), (k[:npk], want_k)
    assert (k[npk:].view(np.uint8) == SENT).all()
    with np.errstate(invalid="ignore"):
        _check_split(got, xs, base, want_k, V, W, 7)


def test_auto_refuses_a_bad_degree_with_nothing_written():
    from ina_amd import _lib
    o, V, W, n = ops(), 32, 2, 100
    xs = [torch.ones(n, device=DEV) for _ in range(W)]
    for degree in (0, -2):
        with pytest.raises(ValueError, match="degree"):
            o.quantize_pack_nga_multi_split_blk(xs, V, [1, 2], W, 1, 1, degree=degree)
        kb, hd, pa = sentinel((4,), torch.int8), sentinel((4, 16)), sentinel((4, 4 * V))
        prm = (_lib.NgaParams * W)(*[_lib.NgaParams(w + 1, W, 0, 1, 0, 1, NUM_SLOTS, V) for w in range(W)])
        rc = _lib.load().ina_quantize_pack_nga_multi_split_blk(
            _lib.ptr_array([x.data_ptr() for x in xs]), W, None, n, kb.data_ptr(), _lib.BLK_AUTO, degree, prm,
            _lib.ptr_array([hd.data_ptr()] * W), _lib.ptr_array([pa.data_ptr()] * W), None, None)
        assert rc == _lib.INA_EINVAL and b"degree" in _lib.load().ina_last_error_string()
        for t in (kb, hd, pa):
            assert (host(t).view(np.uint8) == SENT).all()


# ---- the PS apply ---------------------------------------------------------------------------------
def apply_case(V, order, seed, slots=5, extra=7, W=3, past=2):
    """A W-worker batch for a bucket of n = slots * V + extra values (a short last slot), packed for
    `past` more slots than the PS's bucket holds, worker W-1's packet of slot 1 missing (the slot never
    completes) and two foreign packets (another switch id) in between."""
    n, nbig = slots * V + extra, (slots + 1 + past) * V
    rng, xs, base = bucket(seed, W, nbig, V)
    kblk = R.kblk_ref(xs, V, W, 32, base=base)
    seq0 = 0xFFFFFFFD                                    # wraps inside the bucket
    stride = ops().nga_stride(V)
    rows = [ref_rows(xs[w], base, kblk, V, 1 << w, W, seq0, stride) for w in range(W)]
    foreign = ref_rows(xs[0], base, kblk, V, 1, W, seq0, stride, switch_id=9)[:2]
    npk = len(rows[0])
    pk = [rows[w][p] for p in range(npk) for w in range(W) if not (p == 1 and w == W - 1)]
    pk[4:4] = list(foreign)
    pk = np.stack(pk)
    if order == "shuffled":
        pk = pk[rng.permutation(len(pk))]
    return n, base[:n].copy(), kblk[:slots + 1].copy(), seq0, stride, np.ascontiguousarray(pk)


def expected_apply(pk, V, stride, seq0, local, kblk, ws, n, untouched):
    """(actions, out) from the oracle switch's sums: completed slots inside the bucket get
    _blk_ref.ps_apply, everything else keeps `untouched`."""
    from ina_amd import _lib
    rew, act = orc.Switch(V, NUM_SLOTS, 1).run(pk, stride)
    done = rew[act == _lib.ACT_FWD_AGG]
    f, vals = orc.unpack_nga(done, V, stride)
    nslots = -(-n // V)
    sums = np.zeros(nslots * V, np.int32)
    hit = np.zeros(nslots * V, bool)
    for i, frag in enumerate(f["frag_id"]):
        slot = (int(frag) - seq0) & 0xFFFFFFFF
        if slot < nslots:
            sums[slot * V:(slot + 1) * V] = vals[i * V:(i + 1) * V]
            hit[slot * V:(slot + 1) * V] = True
    assert hit.any() and not hit[:n].all() and len(done) > hit.sum() // V      # completed, missing and past slots
    out = np.where(hit[:n], R.ps_apply(local, sums[:n], kblk, V, ws), untouched)
    return act, out.astype(np.float32), done


@pytest.mark.parametrize("with_acks", [True, False])
@pytest.mark.parametrize("order", ["round-robin", "shuffled"])
@pytest.mark.parametrize("V", [32, 256])
def test_apply_completed_blk_packed_and_split(V, order, with_acks):
    o, ws = ops(), 1.0 / 3
    n, local, kblk, seq0, stride, pk = apply_case(V, order, V + len(order))
    nslots = kblk.size
    sent_f = np.float32(-777.5)
    want_act, want_out, done = expected_apply(pk, V, stride, seq0, local, kblk, ws, n, sent_f)
    # packed rows through Switch.process
    dpk = dev(pk)
    act = o.Switch(V, NUM_SLOTS, 1, DEV).process(dpk)
    assert np.array_equal(host(act), want_act)
    buf = torch.full((n + 5,), float(sent_f), device=DEV)
    acks = sentinel((nslots + 2, 32)) if with_acks else None
    o.apply_completed_blk(dpk, act, V, seq0, dev(local), dev(kblk), ws, out=buf[:n], acks=acks)
    got = host(buf)
    assert np.array_equal(got[:n].view(np.uint32), want_out.view(np.uint32))
    assert (got[n:] == sent_f).all()
    # the sibling on the same batch writes the same ack rows
    sib = sentinel((nslots + 2, 32)) if with_acks else None
    o.apply_completed(dpk, act, V, seq0, dev(local), 16, ws, acks=sib)
    if with_acks:
        acks, sib = host(acks), host(sib)
        assert np.array_equal(acks, sib) and (acks[nslots:] == SENT).all() and (acks[:, 16:] == SENT).all()
        assert (acks[:, :16] != SENT).any()
    # out aliasing local (the sibling allows it): slots that did not complete keep local
    loc = torch.full((n + 5,), float(sent_f), device=DEV)
    loc[:n] = dev(local)
    o.apply_completed_blk(dpk, act, V, seq0, loc[:n], dev(kblk), ws, out=loc[:n])
    want_alias = np.where(want_out == sent_f, local, want_out)
    assert np.array_equal(host(loc)[:n].view(np.uint32), want_alias.view(np.uint32)) and (host(loc)[n:] == sent_f).all()
    # split rows through Switch.process_split
    hd, pa = split_of(pk, V)
    dh, dp = dev(hd), dev(pa)
    act2 = o.Switch(V, NUM_SLOTS, 1, DEV).process_split(dh, dp)
    assert np.array_equal(host(act2), want_act)
    buf2 = torch.full((n + 5,), float(sent_f), device=DEV)
    acks2 = sentinel((nslots + 2, 32)) if with_acks else None
    o.apply_completed_blk(dh, act2, V, seq0, dev(local), dev(kblk), ws, out=buf2[:n], acks=acks2, pay=dp)
    got2 = host(buf2)
    assert np.array_equal(got2[:n].view(np.uint32), want_out.view(np.uint32)) and (got2[n:] == sent_f).all()
    if with_acks:
        acks2 = host(acks2)
        wrote = acks[:, 0] != SENT
        assert np.array_equal(acks2[:, :15], acks[:, :15]) and (acks2[wrote, 15] == 0).all()
        assert (acks2[~wrote] == SENT).all() and (acks2[:, 16:] == SENT).all()


# ---- every new grid-stride loop past its first pass ----------------------------------------------
def test_grid_stride_loops_run_four_passes_and_more():
    """ops.set_tuning(max_blocks=1): one 256-thread workgroup, so the block-scaled launches (which all
    honour that cap) stride -- the multi split pack over 1061 chunks (5 passes of 256, the last of 37),
    the packed pack over its flat chunk stream (V = 32: 133 packets x 9 chunks), its wave-per-packet
    V = 256 kernel (18 packets, 4 a pass) and its byte path, the apply over 1054 packets (256 a pass)."""
    o = ops()
    o.set_tuning(max_blocks=1)
    try:
        V, W = 32, 3
        n = 4 * 1061 - 2
        rng, xs, base = bucket(99, W, n, V)
        kblk = R.kblk_ref(xs, V, W, 32, base=base)
        got, k = _multi_split(o, xs, base, V, W, 7)
        assert np.array_equal(host(k)[:kblk.size], kblk)
        _check_split(got, xs, base, kblk, V, W, 7)
        got, _ = _multi_split(o, xs, base, V, W, 7, kblk=dev(kblk))
        _check_split(got, xs, base, kblk, V, W, 7)
        for V1, n1, stride in ((32, 133 * 32 - 3, None), (256, 17 * 256 + 5, None), (32, 40 * 32 + 1, 15 + 4 * 32)):
            rng, x1, b1 = bucket(V1 + n1, 1, n1, V1)
            k1 = R.kblk_ref(x1, V1, 1, 32, base=b1)
            r = o.quantize_pack_nga_blk(dev(x1[0]), dev(k1), V1, 1, 1, 1, 5, base=dev(b1), num_slots=NUM_SLOTS,
                                        stride=stride)
            assert np.array_equal(host(r), ref_rows(x1[0], b1, k1, V1, 1, 1, 5, stride or o.nga_stride(V1)))
        n, local, kblk, seq0, stride, pk = apply_case(V, "shuffled", 5, slots=348, extra=23)
        assert len(pk) >= 4 * 256 + 1 and len(pk) % 256
        want_act, want_out, _ = expected_apply(pk, V, stride, seq0, local, kblk, 0.25, n, np.float32(3.0))
        for split in (False, True):
            if split:
                hd, pa = split_of(pk, V)
                rows, pay = dev(hd), dev(pa)
                act = o.Switch(V, NUM_SLOTS, 1, DEV).process_split(rows, pay)
            else:
                rows, pay = dev(pk), None
                act = o.Switch(V, NUM_SLOTS, 1, DEV).process(rows)
            out = torch.full((n,), 3.0, device=DEV)
            o.apply_completed_blk(rows, act, V, seq0, dev(local), dev(kblk), 0.25, out=out, pay=pay)
            assert np.array_equal(host(out).view(np.uint32), want_out.view(np.uint32)), split
    finally:
        o.set_tuning(max_blocks=16384)


# ---- the point of the feature ----------------------------------------------------------------------
def test_block_scales_keep_small_blocks_that_one_global_scale_zeroes():
    """W = 4 workers, V = 256, 96 packets with block magnitudes 1e-9 .. 1e3, AUTO pack -> switch ->
    apply_completed_blk with local = 0 and weight_step = 1, against the float64 sum of the inputs.

    The bound, per element of block s with k = kblk[s], is not tuned.  AUTO picks k so that no summand
    saturates (amax * 2^k <= (2^31 - 1) / W - 1/2), so each summand is rounded to the nearest integer:
    an error of at most half a unit, 2^-(k+1), per summand, W * 2^-(k+1) in all.  The switch adds the
    integers exactly.  float(sum) is one fp32 rounding: at most |sum| * 2^-24, times 2^-k.  The
    multiplications by 2^-k and by weight_step = 1 and the addition of local = 0 are exact.
        bound = W * 2^-(k+1) + |sum| * 2^-24 * 2^-k
    At the one global k that scale_for_workers gives for the bucket's largest block, the same path
    returns whole blocks of zeros: the count is computed from the CPU oracle first and asserted as is."""
    o, W, V, npk = ops(), 4, 256, 96
    n = npk * V
    xs = R.bucket(np.random.default_rng(2024), W, n, V)
    dx = [dev(x) for x in xs]
    zero = torch.zeros(n, device=DEV)
    exact = xs.astype(np.float64).sum(0)
    # per-block scales
    hdrs, pays, kblk = o.quantize_pack_nga_multi_split_blk(dx, V, [1 << w for w in range(W)], W, 1, 1)
    kb = host(kblk)
    assert np.array_equal(kb, R.kblk_ref(xs, V, W, 32))
    hd = torch.stack(hdrs, 1).reshape(W * npk, 16).contiguous()          # round-robin arrival
    pa = torch.stack(pays, 1).reshape(W * npk, 4 * V).contiguous()
    act = o.Switch(V, NUM_SLOTS, 1, DEV).process_split(hd, pa)
    got = host(o.apply_completed_blk(hd, act, V, 1, zero, kblk, 1.0, pay=pa)).astype(np.float64)
    sums = R.quantize_reduce_i32(list(xs), kb, V).astype(np.float64)
    inv = np.repeat(np.ldexp(1.0, -kb.astype(np.int64)), V)
    bound = W * inv / 2 + np.abs(sums) * 2.0 ** -24 * inv
    err = np.abs(got - exact)
    print("worst err / bound per block:", (err / bound).reshape(npk, V).max(1).max())
    assert (err <= bound).all()
    assert (np.abs(got).reshape(npk, V).max(1) > 0).all()                # no block is lost
    # one global scale
    kg = o.scale_for_workers(dx)
    want_zero = int((orc.quantize_reduce_i32(list(xs), kg).reshape(npk, V) == 0).all(1).sum())
    rows = o.quantize_pack_nga_multi(dx, kg, V, [1 << w for w in range(W)], W, 1, 1)
    pk = torch.stack(rows, 1).reshape(W * npk, -1).contiguous()
    act = o.Switch(V, NUM_SLOTS, 1, DEV).process(pk)
    glob = host(o.apply_completed(pk, act, V, 1, zero, kg, 1.0))
    got_zero = int((glob.reshape(npk, V) == 0).all(1).sum())
    print(f"global k = {kg}: {got_zero} of {npk} blocks all zero (oracle: {want_zero})")
    # one unit at the global k (17 for a 4e3 maximum and 4 summands) is 7.6e-6: the blocks below ~1e-6,
    # a quarter of 12 log-uniform decades, round to nothing
    assert want_zero >= npk // 8
    assert got_zero == want_zero


# ---- the whole flow in one process -----------------------------------------------------------------
def _noise(idx, epoch, n):
    g = torch.Generator().manual_seed(1000 * idx + epoch)
    mag = torch.logspace(-7, 1, -(-n // 32)).repeat_interleave(32)[:n]
    return (torch.randn(n, generator=g) * mag).numpy().astype(np.float32)


def _train_step(model, idx, epoch):
    with torch.no_grad():
        v = torch.nn.utils.parameters_to_vector(model.parameters())
        v += torch.from_numpy(_noise(idx, epoch, v.numel())).to(v.device)
        torch.nn.utils.vector_to_parameters(v, model.parameters())


def _make_model():
    torch.manual_seed(3)
    return torch.nn.Linear(40, 70)                       # 2870 parameters: 90 NGA-32 packets, the last short


def _run_flow(k, W=2, V=32, epochs=2):
    from ina_amd.loopback import ps_serve, worker_serve
    model = _make_model().to(DEV)
    local0 = torch.nn.utils.parameters_to_vector(model.parameters()).detach().cpu().numpy()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    seen, errs, listening = [], [], threading.Event()
    # the data path has its receive timeout (timeout_ms); the threads are daemons and joined with a
    # timeout, so a peer that dies ends the test instead of hanging it
    try:
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "switch.sock")

            def guarded(fn, *a, **kw):
                try:
                    fn(*a, **kw)
                except Exception as e:      # noqa: BLE001 -- reported below
                    errs.append(e)
                    listening.set()

            th = [threading.Thread(target=guarded, args=(ps_serve, model, W, epochs, port, path), daemon=True,
                                   kwargs=dict(k=k, V=V, timeout_ms=30000, on_listen=listening.set,
                                               on_epoch=lambda e, v, ta, tt: seen.append(v.cpu().numpy().copy())))]
            th[0].start()
            assert listening.wait(30) and not errs, errs
            th += [threading.Thread(target=guarded, args=(worker_serve, i, W, port, path, _make_model, _train_step),
                                    kwargs=dict(device=DEV), daemon=True) for i in range(W)]
            for t in th[1:]:
                t.start()
            for t in th:
                t.join(60)
            assert not errs, errs
            assert not any(t.is_alive() for t in th)
    finally:
        listening.set()
    assert len(seen) == epochs
    return local0, seen


def test_loopback_flow_with_block_scales_equals_the_cpu_replay():
    W, V, epochs = 2, 32, 2
    local, seen = _run_flow("block", W, V, epochs)
    for e in range(epochs):
        paras = [(local + _noise(i, e, local.size)).astype(np.float32) for i in range(W)]
        kmin = np.minimum.reduce([R.kblk_ref([p], V, W, 32, base=local) for p in paras])
        assert kmin.max() - kmin.min() >= 16             # the blocks really carry different scales
        q = [R.quantize_i32((p - local).astype(np.float32), kmin, V) for p in paras]
        local = R.ps_apply(local, orc.sum_reduce_i32(q), kmin, V, 1.0 / (W + 1))
        assert np.array_equal(seen[e].view(np.uint32), local.view(np.uint32)), e


def test_loopback_flow_with_an_integer_k_is_todays():
    W, V, epochs, K = 2, 32, 2, 16
    local, seen = _run_flow(K, W, V, epochs)
    for e in range(epochs):
        paras = [(local + _noise(i, e, local.size)).astype(np.float32) for i in range(W)]
        local = orc.ps_combine_ina_f32(local, paras, K, 1.0 / (W + 1))
        assert np.array_equal(seen[e].view(np.uint32), local.view(np.uint32)), e
