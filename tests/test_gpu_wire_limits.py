"""The newer wires at the limits their own tests leave out, bit for bit against the numpy yardsticks
(tests/_wire_limits.py states the inputs): the requantised byte gather (include/ina_i8_gather.h), error feedback and
stochastic rounding on the byte wire (ina_i8_ef.h, ina_i8_sr.h) and the nibble wire (ina_i4.h) -- every compile-time
slice count and remainder of the run-time loop, every ragged tail of the nibble sums, every block width with the
block's maximum in the first, the last and a middle lane of its group, the quantisers on the planted bucket of
tests/_rot_limits.py, sign keys whose Philox counter is odd or needs its high word, slices against the whole,
views of one receive buffer, and the refusals.

Every device output is 0xA5-filled, PAD elements longer than the result and 16 bytes past a 256-byte boundary
(scales, flags and shifts: 1 or 3 bytes into a larger buffer); the bytes before and after the result must still
hold the fill.  No comparison has a tolerance."""
import numpy as np
import pytest
import torch

from tests import _i4_ref as r4
from tests import _rot_limits as R
from tests import _wire_limits as L
from tests._limits import dev, dev_rows, sent
from tests._rot_limits import NBLK, SEED, STEP, SUB, key, out16, same_out, untouched
from tests.test_gpu_rot import grid_cap
from tests.test_gpu_rot_limits import BOTH_CAPS, rows, scales_at

pytestmark = pytest.mark.gpu
CASES = pytest.mark.parametrize("V,W,src", R.CASES, ids=lambda v: str(v))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def shifts_at(nblk):
    """Shift bytes at an odd address."""
    sh = sent(nblk, torch.uint8, 1)
    assert sh.data_ptr() % 2 == 1
    return sh


def run_sum(kind, bufs, V, n):
    """One sum into placed outputs: (int16 sums,) or (bytes, shifts)."""
    from ina_amd import i4, i8
    if kind in ("i8.sum", "i4.sum"):
        out = out16(n, torch.int16)
        (i8 if kind == "i8.sum" else i4).sum_slices(bufs, out=out)
        return (out,)
    q, sh = out16(n, torch.int8), shifts_at(n // V)
    if kind == "i8.rq":
        i8.sum_slices_requant(bufs, V, out=q, shift=sh)
    elif kind == "i8.rq_sr":
        i8.sum_slices_requant_sr(bufs, V, SEED, out=q, shift=sh, **L.RND)
    else:
        i4.sum_slices_requant(bufs, V, out=q, shift=sh)
    return q, sh


def check_sum(kind, parts, want, V, caps=(None,), what=""):
    bufs = dev_rows(parts.copy())
    n = want[0].size
    for cap in caps:
        with grid_cap(cap):
            got = run_sum(kind, bufs, V, n)
        for g, w, name in zip(got, want, ("values", "shifts")):
            same_out(g, w, f"{kind} {what} cap={cap} {name}")
        if kind in L.REQUANT:
            assert int(got[0][:n].min()) >= -127, f"{kind} {what}: -128 written"


# ---- 1 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", L.G_STATIC + L.G_LOOP)
@pytest.mark.parametrize("kind", L.SUMS)
def test_every_compile_time_slice_count_and_loop_remainder(kind, G):
    """G = 4 and 16 are template instances of their own (16 of the byte sums: two batches of 8 loads); 5, 15, 31 and
    63 leave the run-time loops' remainders.  Columns at both extremes in every slice, and random slices."""
    for fill in ("extreme", "random"):
        parts, want = L.g_case(kind, G, fill)
        check_sum(kind, parts, want, L.G_V, BOTH_CAPS, f"G={G} {fill}")


# ---- 2 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", L.RAG_G)
def test_every_ragged_tail_of_the_nibble_sums(G):
    """The lane after the whole chunks holds 1, 2 or 3 dwords: the exact sum at 2 (the existing cases are 1 and 3),
    the requantiser at each of them with and without a whole chunk in front, the last block holding the largest sum."""
    for n in L.RAG_SUM_N:
        parts, want = L.rag_sum_case(G, n)
        check_sum("i4.sum", parts, want, 0, what=f"G={G} n={n}")
    for V, nblk in L.RAG_RQ:
        parts, want = L.rag_rq_case(G, V, nblk)
        check_sum("i4.rq", parts, want, V, BOTH_CAPS, f"G={G} V={V} nblk={nblk}")


# ---- 3 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", L.V_G)
@pytest.mark.parametrize("V", L.ALL_V)
@pytest.mark.parametrize("kind", L.REQUANT)
def test_every_block_width_of_the_requantisers(kind, V, G):
    """41 blocks whose largest sum sits in the first, the last or a middle lane of the block's lane group, under
    targets that ask for every shift: a step of the group maximum left out gives a block a smaller shift."""
    parts, want, _ = L.v_case(kind, V, G)
    check_sum(kind, parts, want, V, BOTH_CAPS, f"V={V} G={G}")


# ---- 4 -------------------------------------------------------------------------------------------------------
def check_nibbles(V, W, src, e0=0, caps=(None,), rots=(False, True)):
    from ina_amd import i4
    bufs, n = rows(V, W, src, e0), NBLK * V
    for rot_on in rots:
        want_kb, given, want = L.q4_case(V, W, src, e0, rot_on)
        rotate, kb = SEED if rot_on else None, scales_at(given)
        for cap in caps:
            what = f"V={V} W={W} {src} rot={rot_on} e0={e0:#x} cap={cap}"
            out = scales_at(None, 3)
            with grid_cap(cap):
                i4.block_scales(bufs, V, rotate, out=out, **key(e0))
            same_out(out, want_kb, "i4.block_scales " + what)
            for w, (q, flags) in want.items():
                o, fl = out16(n // 2, torch.uint8), sent(NBLK, torch.uint8, 3)
                with grid_cap(cap):
                    i4.quantize(bufs[w], kb[:NBLK], V, rotate, out=o, overflow=fl, **key(e0))
                same_out(o, q, f"i4.quantize worker {w} " + what)
                same_out(fl, flags, f"i4.quantize flags worker {w} " + what)
                assert r4.unpack(o[:n // 2].cpu().numpy()).min() >= -7, what + ": -8 written"
        same_out(kb, given, "i4.quantize wrote to its scales")


@CASES
def test_nibble_scales_and_quantiser_on_the_planted_bucket(V, W, src):
    """i4.block_scales over the W buckets and i4.quantize of the workers that hold the plants, plain and rotated,
    under scales of which one is -128 and one 8 too large: nibbles, flags, -8 never written."""
    check_nibbles(V, W, src, caps=BOTH_CAPS)


@CASES
def test_stochastic_byte_quantiser_on_the_planted_bucket(V, W, src):
    from ina_amd import i8
    bufs, n = rows(V, W, src), NBLK * V
    for rot_on in (False, True):
        want_kb, given, want = L.sr_case(V, W, src, rot_on)
        rotate, kb = SEED if rot_on else None, scales_at(given)
        for cap in BOTH_CAPS:
            what = f"V={V} W={W} {src} rot={rot_on} cap={cap}"
            out = scales_at(None, 3)
            with grid_cap(cap):
                i8.block_scales_sr(bufs, V, rotate, out=out, **key())
            same_out(out, want_kb, "i8.block_scales_sr " + what)
            for w, (q, flags) in want.items():
                o, fl = out16(n, torch.int8), sent(NBLK, torch.uint8, 3)
                with grid_cap(cap):
                    i8.quantize_sr(bufs[w], kb[:NBLK], V, L.SR_SEED, rotate, step=STEP, rot_sub=SUB, out=o, overflow=fl,
                                   **L.SR_KEY)
                same_out(o, q, f"i8.quantize_sr worker {w} " + what)
                same_out(fl, flags, f"i8.quantize_sr flags worker {w} " + what)
                assert int(o[:n].min()) >= -127, what + ": -128 written"
        same_out(kb, given, "i8.quantize_sr wrote to its scales")


@CASES
def test_error_feedback_byte_quantiser_on_the_planted_bucket(V, W, src):
    """The residual is read from and rewritten in a placed buffer of its own: its bits, and the fill around it."""
    from ina_amd import i8
    bufs, n = rows(V, W, src), NBLK * V
    res = dev_rows(L.residuals(V, W).copy())
    for rot_on in (False, True):
        want_kb, given, want = L.ef_case(V, W, src, rot_on)
        rotate, kb = SEED if rot_on else None, scales_at(given)
        for cap in BOTH_CAPS:
            what = f"V={V} W={W} {src} rot={rot_on} cap={cap}"
            out = scales_at(None, 3)
            with grid_cap(cap):
                i8.block_scales_ef(bufs, res, V, rotate, out=out, **key())
            same_out(out, want_kb, "i8.block_scales_ef " + what)
            for w, (q, flags, after) in want.items():
                o, fl, r = out16(n, torch.int8), sent(NBLK, torch.uint8, 3), out16(n, torch.float32)
                r[:n].copy_(res[w])
                with grid_cap(cap):
                    i8.quantize_ef(bufs[w], r[:n], kb[:NBLK], V, rotate, out=o, overflow=fl, **key())
                same_out(o, q, f"i8.quantize_ef worker {w} " + what)
                same_out(fl, flags, f"i8.quantize_ef flags worker {w} " + what)
                same_out(r, after, f"i8.quantize_ef residual worker {w} " + what)
                assert int(o[:n].min()) >= -127, what + ": -128 written"
        same_out(kb, given, "i8.quantize_ef wrote to its scales")
    for w, r in enumerate(res):                                            # block_scales_ef only reads
        assert np.array_equal(r.cpu().numpy().view(np.uint32), L.residuals(V, W)[w].view(np.uint32)), w


# ---- 5 and 6 ----------------------------------------------------------------------------------------------------
def run_gather(q8, sh, kb, V, e0):
    from ina_amd import i8
    y = out16(q8.numel(), torch.float32)
    i8.dequantize_gather(q8, sh, kb, V, SEED, out=y, **key(e0))
    return y


def gather_inputs(V):
    """The bytes 16 bytes past a 16-byte boundary, the shifts and the scales at odd addresses."""
    q8, sh, kb, _ = L.gather_case(V)
    return dev(q8.copy(), 16), dev(sh.copy(), 1), dev(kb.copy(), 3)


@pytest.mark.parametrize("V,e0", [(V, e0) for V in (32, 128, 256) for e0 in R.e0s(V)], ids=lambda v: f"{v:#x}")
def test_sign_keys_with_an_odd_counter_and_a_high_word(V, e0):
    """The rotated nibble quantiser and the rotated decode of the requantised gather at e0 >> 7 odd, at the carry
    into the counter's high word, and past 32 bits."""
    check_nibbles(V, 4, "f32", e0, rots=(True,))
    same_out(run_gather(*gather_inputs(V), V, e0), L.gather_case(V, e0)[3], f"i8.dequantize_gather V={V} e0={e0:#x}")


@pytest.mark.parametrize("V,src", [(16, "f32"), (32, "f16"), (128, "f32"), (256, "bf16")])
def test_a_slice_with_e0_at_its_start_is_that_slice_of_the_whole(V, src):
    """Calls on the views [lo, hi) with e0 = lo against [lo, hi) of the whole-bucket call with e0 = 0: device against
    device, and both against the replay."""
    from ina_amd import i4
    W, n = 4, NBLK * V
    lo, hi = R.slice_lo(V)
    b0, b1 = lo // V, hi // V
    bufs = rows(V, W, src)
    _, given, want = L.q4_case(V, W, src, 0, True)
    kb = scales_at(given)
    for w, (q, flags) in want.items():
        outs = []
        for buf, e0, m, k in ((bufs[w], 0, n, kb[:NBLK]), (bufs[w][lo:hi], lo, hi - lo, kb[b0:b1])):
            o, fl = out16(m // 2, torch.uint8), sent(m // V, torch.uint8, 3)
            i4.quantize(buf, k, V, SEED, out=o, overflow=fl, **key(e0))
            outs.append((o, fl))
        same_out(outs[0][0], q, f"i4.quantize whole V={V} worker {w}")
        same_out(outs[1][0], q[lo // 2:hi // 2], f"i4.quantize slice V={V} worker {w}")
        same_out(outs[1][1], flags[b0:b1], f"i4.quantize slice flags V={V} worker {w}")
        assert torch.equal(outs[1][0][:(hi - lo) // 2], outs[0][0][lo // 2:hi // 2])
        assert torch.equal(outs[1][1][:b1 - b0], outs[0][1][b0:b1])
    q8, sh, kbd = gather_inputs(V)
    y = L.gather_case(V)[3]
    whole, piece = run_gather(q8, sh, kbd, V, 0), run_gather(q8[lo:hi], sh[b0:b1], kbd[b0:b1], V, lo)
    same_out(whole, y, f"i8.dequantize_gather whole V={V}")
    same_out(piece, y[lo:hi], f"i8.dequantize_gather slice V={V}")
    assert np.array_equal(R.canon(piece[:hi - lo].cpu().numpy()), R.canon(whole[lo:hi].cpu().numpy()))


# ---- 7 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", L.V_G)
@pytest.mark.parametrize("kind", ("i4.sum", "i4.rq", "i8.rq", "i8.rq_sr"))
def test_sums_over_views_of_one_receive_buffer(kind, G):
    """G views of one allocation, as the aggregators pass them: nibble slices shard / 2 = 192 bytes apart (odd
    multiples of 64 bytes among them), byte slices 384 bytes apart."""
    recv, n, want = L.view_case(kind, G)
    pitch = recv.shape[1]
    d = dev(recv.reshape(-1).copy(), 16)
    held = n // 2 if L.nibble(kind) else n
    views = [d[g * pitch:g * pitch + held] for g in range(G)]
    assert (views[1].data_ptr() - views[0].data_ptr()) % 128 == (64 if L.nibble(kind) else 0)
    got = run_sum(kind, views, L.VIEW_V, n)
    for g, w, name in zip(got, want, ("values", "shifts")):
        same_out(g, w, f"{kind} views G={G} {name}")


# ---- 8 -------------------------------------------------------------------------------------------------------
def test_a_buffer_off_a_16_byte_boundary_is_refused_by_name():
    """Once per entry point of the four sources: an input 4 bytes past a 16-byte boundary, and every output (and the
    residual) stays untouched.  The shift pointer is exempt: every requantiser call of this module writes its
    shifts at an odd address, and one more does so here."""
    from ina_amd import i4, i8
    from ina_amd._lib import InaError
    V, W = 32, 2
    n = NBLK * V
    bad = dev_rows(R.bucket(V, 4)[1][:W].copy(), 1)
    good = rows(V, 4)[:W]
    res = [out16(n, torch.float32)[:n] for _ in range(W)]
    kb, fl, sh = scales_at(None), sent(NBLK, torch.uint8, 3), shifts_at(NBLK)
    o16, o8, o4, of = out16(n, torch.int16), out16(n, torch.int8), out16(n // 2, torch.uint8), out16(n, torch.float32)
    bytes_ = dev(np.zeros(n + 4, np.int8))[4:]
    nibs = dev(np.zeros(n // 2 + 4, np.uint8))[4:]
    given = scales_at(np.zeros(NBLK, np.int8))[:NBLK]
    shifts = dev(np.zeros(NBLK, np.uint8), 1)
    assert all(t.data_ptr() % 16 == 4 for t in (bad[0], bad[1], bytes_, nibs)) and good[0].data_ptr() % 16 == 0
    calls = (lambda: i8.sum_slices_requant([bytes_, bytes_], V, out=o8, shift=sh),
             lambda: i8.dequantize_gather(bytes_, shifts, given, V, SEED, out=of),
             lambda: i8.block_scales_ef(bad, res, V, SEED, out=kb),
             lambda: i8.quantize_ef(bad[0], res[0], given, V, SEED, out=o8, overflow=fl),
             lambda: i8.block_scales_sr(bad, V, SEED, out=kb),
             lambda: i8.quantize_sr(bad[0], given, V, L.SR_SEED, SEED, out=o8, overflow=fl),
             lambda: i8.sum_slices_requant_sr([bytes_, bytes_], V, SEED, out=o8, shift=sh, **L.RND),
             lambda: i4.block_scales(bad, V, SEED, out=kb),
             lambda: i4.quantize(bad[0], given, V, SEED, out=o4, overflow=fl),
             lambda: i4.sum_slices([nibs, nibs], out=o16),
             lambda: i4.sum_slices_requant([nibs, nibs], V, out=o8[:n], shift=sh))
    assert len(calls) == 11
    for call in calls:
        with pytest.raises(InaError, match="16-byte aligned"):
            call()
        untouched(kb, fl, sh, o16, o8, o4, of, *res)
    zeros = dev(np.zeros(n, np.int8), 16)
    i8.sum_slices_requant([zeros, zeros], V, out=o8, shift=sh)           # an odd shift address is accepted
    same_out(sh, np.zeros(NBLK, np.uint8), "shifts at an odd address")
    same_out(o8, np.zeros(n, np.int8), "bytes beside them")


def test_more_than_64_buffers_or_slices_are_refused_by_name():
    from ina_amd import i4, i8
    V = 32
    x, r = dev(np.zeros(V, np.float32)), dev(np.zeros(V, np.float32))
    b, nb = dev(np.zeros(V, np.int8)), dev(np.zeros(V // 2, np.uint8))
    kb, sh, o8, o16 = sent(1, torch.int8), shifts_at(1), sent(V, torch.int8), sent(V, torch.int16)
    for call in (lambda: i8.block_scales_ef([x] * 65, [r] * 65, V, SEED, out=kb),
                 lambda: i8.block_scales_sr([x] * 65, V, SEED, out=kb),
                 lambda: i4.block_scales([x] * 65, V, SEED, out=kb)):
        with pytest.raises(ValueError, match=r"1\.\.64 worker buffers, got 65"):
            call()
    for call in (lambda: i8.sum_slices_requant([b] * 65, V, out=o8, shift=sh),
                 lambda: i8.sum_slices_requant_sr([b] * 65, V, SEED, out=o8, shift=sh, **L.RND),
                 lambda: i4.sum_slices([nb] * 65, out=o16),
                 lambda: i4.sum_slices_requant([nb] * 65, V, out=o8, shift=sh)):
        with pytest.raises(ValueError, match=r"1\.\.64 slices, got 65"):
            call()
    untouched(kb, sh, o8, o16)
