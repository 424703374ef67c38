"""The rotation (include/ina_rot.h, ina_amd.rot) and the byte wire (include/ina_i8.h, ina_amd.i8) at their
stated limits, bit for bit against tests/_rot_ref.py, tests/_i8_ref.py and tests/_blk_ref.py: every block size
on a bucket of planted edge values (tests/_rot_limits.py), run-time worker counts up to 64, sign keys whose
Philox counter is odd or needs its high word, slices against the whole bucket, and placed buffers.

Every device output is 0xA5-filled, PAD elements longer than the result and 16 bytes past a 256-byte
boundary (scales and flags: 1 and 3 bytes into a larger buffer); the bytes before and after the result must
still hold the fill.  Floats compare through their bits, a NaN matching any NaN."""
import numpy as np
import pytest
import torch

from tests import _i8_ref as iref
from tests import _rot_limits as R
from tests._limits import dev, dev_rows, sent
from tests._rot_limits import NBLK, SEED, key, out16, same_out, untouched
from tests.test_gpu_rot import grid_cap

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("V,W,src", R.CASES, ids=lambda v: str(v))
BOTH_CAPS = (None, 1)                       # the default grid, and one workgroup striding over the bucket
_ROWS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rows(V, W, src="f32", e0=0):
    """The planted bucket's W rows on the device, each 16 bytes past a 16-byte boundary; never written to."""
    if (V, W, src, e0) not in _ROWS:
        got = R.bucket(V, W, src, e0)[0]
        got = torch.from_numpy(got.copy()) if isinstance(got, np.ndarray) else got
        _ROWS[V, W, src, e0] = dev_rows(got, 16 // got.element_size())
    return _ROWS[V, W, src, e0]


def scales_at(want, off=1):
    """An int8 scale array `off` bytes into a filled buffer, holding `want` when given."""
    kb = sent(NBLK, torch.int8, off)
    if want is not None:
        kb[:NBLK].copy_(torch.from_numpy(np.array(want)))
    return kb


def run_fused(bufs, V, nbits, given, e0, n, nblk=NBLK):
    """One fused reduce and its decode into placed outputs: (q, flags or None, kblk, y)."""
    from ina_amd import rot
    out = out16(n, torch.int32 if nbits == 32 else torch.int16)
    kb = sent(nblk, torch.int8, 1)
    if given is not None:
        kb[:nblk].copy_(given)
    args = dict(kblk=kb) if given is not None else dict(kblk_out=kb)
    fl = None
    if nbits == 32:
        rot.quantize_reduce(bufs, V, SEED, out=out, **args, **key(e0))
    else:
        fl = sent(nblk, torch.uint8, 3)
        rot.quantize_reduce_i16(bufs, V, SEED, out=out, overflow=fl, **args, **key(e0))
    y = out16(n, torch.float32)
    rot.dequantize(out[:n], kb[:nblk], V, SEED, out=y, **key(e0))
    return out, fl, kb, y


def check_fused(V, W, src, e0=0, caps=(None,), modes=("auto", "given"), widths=(32, 16)):
    bufs, n = rows(V, W, src, e0), NBLK * V
    for nbits in widths:
        for mode in modes:
            q, flags, kb, y = R.fused(V, W, src, e0, nbits, mode)
            for cap in caps:
                what = f"V={V} W={W} {src} e0={e0:#x} int{nbits} {mode} cap={cap}"
                with grid_cap(cap):
                    got = run_fused(bufs, V, nbits, torch.from_numpy(kb.copy()).to(bufs[0].device) if mode == "given"
                                    else None, e0, n)
                same_out(got[2], kb, what + " kblk")
                same_out(got[0], q, what + " q")
                if nbits == 16:
                    same_out(got[1], flags, what + " flags")
                same_out(got[3], y, what + " decode")


@CASES
def test_fused_reduces_on_the_planted_bucket(V, W, src):
    """rot.quantize_reduce and rot.quantize_reduce_i16 under AUTO and GIVEN scales: q, flags, kblk and the
    decode of each -- every V, and W in {6, 17, 33, 63, 64} with the integer-side plants."""
    check_fused(V, W, src, caps=BOTH_CAPS)


@CASES
def test_block_scales_on_the_planted_bucket(V, W, src):
    """rot.block_scales at 16 and 32 bits and i8.block_scales, plain and rotated: the group maximum at every
    group width, and the two-in-flight worker loop at even and odd W."""
    from ina_amd import i8, rot
    bufs = rows(V, W, src)
    for cap in BOTH_CAPS:
        with grid_cap(cap):
            for nbits in (16, 32):
                out = scales_at(None)
                rot.block_scales(bufs, V, SEED, bits=nbits, out=out, **key())
                same_out(out, R.fused(V, W, src, 0, nbits, "auto")[2], f"rot.block_scales bits={nbits} cap={cap}")
            for rot_on in (False, True):
                out = scales_at(None, 3)
                i8.block_scales(bufs, V, SEED if rot_on else None, out=out, **key())
                same_out(out, R.i8_case(V, W, src, 0, rot_on)[0], f"i8.block_scales rot={rot_on} cap={cap}")


def check_bytes(V, W, src, e0=0, caps=(None,), rots=(False, True)):
    from ina_amd import i8
    bufs, n = rows(V, W, src, e0), NBLK * V
    for rot_on in rots:
        _, given, want = R.i8_case(V, W, src, e0, rot_on)
        kb = scales_at(given)
        for cap in caps:
            for w, (q, flags) in want.items():
                out, fl = out16(n, torch.int8), sent(NBLK, torch.uint8, 3)
                with grid_cap(cap):
                    i8.quantize(bufs[w], kb[:NBLK], V, SEED if rot_on else None, out=out, overflow=fl, **key(e0))
                what = f"i8.quantize V={V} {src} worker {w} of {W} rot={rot_on} e0={e0:#x} cap={cap}"
                same_out(out, q, what)
                same_out(fl, flags, what + " flags")
                assert int(out[:n].min()) >= -127, what + ": -128 written"
        same_out(kb, given, "i8.quantize wrote to its scales")


@CASES
def test_byte_quantiser_on_the_planted_bucket(V, W, src):
    """i8.quantize, plain and rotated, of the workers that hold the plants: bytes, flags, -128 never written."""
    check_bytes(V, W, src, caps=BOTH_CAPS)


@pytest.mark.parametrize("alias", (False, True), ids=("out", "in-place"))
@pytest.mark.parametrize("V", (32, 256))
def test_ps_combine_at_the_worker_limit(V, alias):
    """rot.ps_combine_ina at W = 64 is the replay of the deltas -> decode -> local + xhat * float32(ws)."""
    from ina_amd import rot
    W, n, ws = 64, NBLK * V, 0.37 / 65
    local, _, kb, want = R.ps_case(V, W, ws)
    paras = rows(V, W)
    lbuf = out16(n, torch.float32)
    lbuf[:n].copy_(torch.from_numpy(local))
    out, kbd = lbuf if alias else out16(n, torch.float32), scales_at(None)
    got = rot.ps_combine_ina(lbuf[:n], paras, V, ws, SEED, out=out, kblk_out=kbd, **key())
    assert got.data_ptr() == out.data_ptr() and (out.data_ptr() == lbuf.data_ptr()) == alias
    same_out(out, want, f"ps_combine_ina V={V} alias={alias}")
    same_out(kbd, kb, f"ps_combine_ina V={V} kblk_out")
    if not alias:
        same_out(lbuf, local, "ps_combine_ina wrote to local")


def test_more_than_64_workers_are_refused_by_name():
    from ina_amd import i8, rot
    V = 32
    x = dev(np.zeros(V, np.float32))
    out, kb = sent(V, torch.int32), sent(1, torch.int8)
    calls = (lambda: rot.quantize_reduce([x] * 65, V, SEED, out=out, kblk_out=kb),
             lambda: rot.quantize_reduce_i16([x] * 65, V, SEED, out=sent(V, torch.int16), kblk_out=kb),
             lambda: rot.block_scales([x] * 65, V, SEED, out=kb),
             lambda: rot.ps_combine_ina(x, [x] * 65, V, 0.5, SEED, out=sent(V, torch.float32), kblk_out=kb),
             lambda: i8.block_scales([x] * 65, V, SEED, out=kb))
    for call in calls:
        with pytest.raises(ValueError, match=r"1\.\.64 worker buffers, got 65"):
            call()
    untouched(out, kb)


@pytest.mark.parametrize("V,e0", [(V, e0) for V in (32, 128, 256) for e0 in R.e0s(V)], ids=lambda v: f"{v:#x}")
def test_sign_keys_with_an_odd_counter_and_a_high_word(V, e0):
    """e0 >> 7 odd (the wave's second Philox call is at c + 1), c = 2^32 - 1 (the carry falls between the two
    calls) and e0 >> 7 past 32 bits: a fused reduce of each width, its decode, and the rotated byte quantiser."""
    check_fused(V, 4, "f32", e0, modes=("auto",))
    check_bytes(V, 4, "f32", e0, rots=(True,))


@pytest.mark.parametrize("V,src", [(16, "f32"), (32, "f16"), (128, "f32"), (256, "bf16")])
def test_a_slice_with_e0_at_its_start_is_that_slice_of_the_whole(V, src):
    """Calls on the views [lo, hi) with e0 = lo against [lo, hi) of the whole-bucket call with e0 = 0 (lo an
    odd multiple of 128, or of V at V = 256): device against device, and both against the replay."""
    from ina_amd import i8, rot
    W, n = 4, NBLK * V
    lo, hi = R.slice_lo(V)
    bufs = rows(V, W, src)
    part = [b[lo:hi] for b in bufs]
    b0, b1 = lo // V, hi // V
    for nbits in (32, 16):
        q, flags, kb, y = R.fused(V, W, src, 0, nbits, "given")
        given = torch.from_numpy(kb.copy()).to(bufs[0].device)
        whole = run_fused(bufs, V, nbits, given, 0, n)
        piece = run_fused(part, V, nbits, given[b0:b1], lo, hi - lo, b1 - b0)
        what = f"V={V} {src} int{nbits} slice [{lo}, {hi})"
        same_out(whole[0], q, what + " whole q")
        same_out(piece[0], q[lo:hi], what + " q")
        same_out(piece[3], y[lo:hi], what + " decode")
        assert torch.equal(piece[0][:hi - lo], whole[0][lo:hi]), what
        assert np.array_equal(R.canon(piece[3][:hi - lo].cpu().numpy()), R.canon(whole[3][lo:hi].cpu().numpy())), what
        if nbits == 16:
            same_out(piece[1], flags[b0:b1], what + " flags")
            assert torch.equal(piece[1][:b1 - b0], whole[1][b0:b1]), what
        # the decode of a slice of the whole call's sums, through scales that are a view at an odd offset
        yd = out16(hi - lo, torch.float32)
        rot.dequantize(whole[0][lo:hi], whole[2][b0:b1], V, SEED, out=yd, **key(lo))
        same_out(yd, y[lo:hi], what + " decode of the whole's slice")
    _, given, want = R.i8_case(V, W, src, 0, True)
    kb = scales_at(given)
    for w, (q, flags) in want.items():
        outs = []
        for buf, e0, m, k in ((bufs[w], 0, n, kb[:NBLK]), (part[w], lo, hi - lo, kb[b0:b1])):
            out, fl = out16(m, torch.int8), sent(m // V, torch.uint8, 3)
            i8.quantize(buf, k, V, SEED, out=out, overflow=fl, **key(e0))
            outs.append((out, fl))
        same_out(outs[1][0], q[lo:hi], f"i8.quantize slice V={V} worker {w}")
        same_out(outs[1][1], flags[b0:b1], f"i8.quantize slice flags V={V} worker {w}")
        assert torch.equal(outs[1][0][:hi - lo], outs[0][0][lo:hi]) and torch.equal(outs[1][1][:b1 - b0], outs[0][1][b0:b1])


def test_a_bucket_off_a_16_byte_boundary_is_refused_by_name():
    """Once per entry point: an input 4 bytes past a 16-byte boundary, and the outputs stay untouched."""
    from ina_amd import i8, rot
    from ina_amd._lib import InaError
    V, W = 32, 2
    n = NBLK * V
    bad = dev_rows(R.bucket(V, 4)[1][:W].copy(), 1)
    good = rows(V, 4)[:W]
    kb, fl = scales_at(None), sent(NBLK, torch.uint8, 3)
    o32, o16, o8, of = (out16(n, t) for t in (torch.int32, torch.int16, torch.int8, torch.float32))
    ints = dev(np.zeros(n + 1, np.int32))[1:]
    bytes_ = dev(np.zeros(n + 4, np.int8))[4:]
    given = scales_at(np.zeros(NBLK, np.int8))
    calls = (lambda: rot.block_scales(bad, V, SEED, out=kb),
             lambda: rot.quantize_reduce(bad, V, SEED, out=o32, kblk_out=kb),
             lambda: rot.quantize_reduce_i16(bad, V, SEED, out=o16, overflow=fl, kblk_out=kb),
             lambda: rot.dequantize(ints, given[:NBLK], V, SEED, out=of),
             lambda: rot.ps_combine_ina(good[0], bad, V, 0.5, SEED, out=of, kblk_out=kb),
             lambda: rot.ps_combine_ina(bad[0], good, V, 0.5, SEED, out=of, kblk_out=kb),
             lambda: i8.block_scales(bad, V, SEED, out=kb),
             lambda: i8.quantize(bad[0], given[:NBLK], V, SEED, out=o8, overflow=fl),
             lambda: i8.sum_slices([bytes_, bytes_], out=o16))
    for i, call in enumerate(calls):
        with pytest.raises(InaError, match="16-byte aligned"):
            call()
        untouched(kb, fl, o32, o16, o8, of)


@pytest.mark.parametrize("G", (3, 64))
def test_slice_sum_over_views_of_one_receive_buffer(G):
    """i8.sum_slices on G views of one buffer at 128-byte-multiple offsets, as dist.ByteWireAggregator passes
    them; a ragged tail, whole columns of -128 and of 127."""
    from ina_amd import i8
    shard = 128 * 3
    n = shard - 5
    recv = np.random.default_rng(G).integers(-128, 128, G * shard).astype(np.int8).reshape(G, shard)
    recv[:, 0], recv[:, 1], recv[:, n - 1] = -128, 127, -128
    d = dev(recv.reshape(-1), 16)
    out = out16(n, torch.int16)
    i8.sum_slices([d[g * shard:g * shard + n] for g in range(G)], out=out)
    same_out(out, iref.sum_slices(list(recv[:, :n])), f"sum_slices G={G}")
