"""tests/_rot_limits.py on the yardsticks alone (no GPU): the planted inputs reach what
tests/test_gpu_rot_limits.py means them to reach, so a later edit to the builders cannot quietly empty the
device tests."""
import numpy as np
import pytest
import torch

from tests import _rot_limits as R
from tests import _rot_ref as rref
from tests._limits import mixed

CASES = pytest.mark.parametrize("V,W,src", R.CASES, ids=lambda v: str(v))
OVERFLOWING = pytest.mark.parametrize("V,W,src", [c for c in R.CASES if c[2] != "f16"], ids=lambda v: str(v))


def scales(V, W, src):
    """Every AUTO scale array the device tests compare: both fused reduces' and the byte wire's two."""
    yield from (R.fused(V, W, src, 0, nbits, "auto")[2] for nbits in (16, 32))
    yield from (R.i8_case(V, W, src, 0, rot)[0] for rot in (False, True))


@OVERFLOWING
def test_big_block_is_finite_and_overflows_in_the_butterfly(V, W, src):
    x, r = R.bucket(V, W, src)[1][:, R.blk("big", V)], R.rotated(V, W, src)[0, R.blk("big", V)]
    assert np.isfinite(x).all() and np.isinf(r).any() and np.isnan(r).any()
    assert all(kb[R.PLANT["big"]] == -126 for kb in list(scales(V, W, src))[:2] + [R.i8_case(V, W, src, 0, True)[0]])
    q, flags, _, y = R.fused(V, W, src, 0, 16, "auto")
    assert flags[R.PLANT["big"]] == 1 and np.isnan(y[R.blk("big", V)]).any()


@OVERFLOWING
def test_tiny_block_rotates_into_the_subnormals(V, W, src):
    r = R.rotated(V, W, src)[W - 1, R.blk("tiny", V)]
    assert ((np.abs(r) < 2.0**-126) & (r != 0)).any()
    assert all(kb[R.PLANT["tiny"]] == 127 for kb in scales(V, W, src))


@pytest.mark.parametrize("V", R.V_NEW + R.V_OLD)
def test_fp16_tiny_and_big_are_the_type_s_own(V):
    h = R.bucket(V, 4, "f16")[0].view(torch.int16).numpy().view(np.uint16)
    tiny, big = h[3, R.blk("tiny", V)], h[0, R.blk("big", V)]
    assert ((tiny & 0x7C00 == 0) & (tiny & 0x03FF != 0)).any()              # fp16 subnormals
    assert (big & 0x7FFF == 0x7BFF).any() and (big & 0x7C00 != 0x7C00).all()  # +-65504, nothing rounded to inf


@CASES
def test_zero_nan_and_negative_zero_blocks_give_127(V, W, src):
    for kb in scales(V, W, src):
        assert [int(kb[R.PLANT[name]]) for name in ("zero", "nan", "negzero")] == [127, 127, 127]


@CASES
def test_inf_blocks_give_minus_126(V, W, src):
    for kb in scales(V, W, src):
        assert int(kb[R.PLANT["inf2"]]) == -126 and int(kb[R.PLANT["nan_inf"]]) == -126


@CASES
@pytest.mark.parametrize("mode", ("auto", "given"))
def test_int16_flags_are_mixed_and_as_listed(V, W, src, mode):
    flags = R.fused(V, W, src, 0, 16, mode)[1]
    mixed(flags)
    planted = sorted(R.PLANT.values())
    assert [s for s in planted if flags[s]] == R.flagged_plants(V, src, mode)
    if mode == "given":
        assert flags[3] == 1 and flags[1] == 0
    # the clamp rate: the case must not test the clamp and nothing else
    assert flags[list(R.ORDINARY)].sum() * 4 <= len(R.ORDINARY)


@CASES
def test_integer_plants_land_where_they_are_meant_to(V, W, src):
    r = R.rotated(V, W, src)
    m = V.bit_length() - 1
    for name, want in (("i_inside", [-32768.0] * W), ("i_sat", [32768.0] * W),
                       ("i_leave", [28672.0, 28672.0, -28672.0, -28672.0] + [0.0] * (W - 4)),
                       ("i_last2", [0.0] * (W - 2) + [20480.0] * 2), ("wrap", [1.0] * W)):
        b = r[:, R.blk(name, V)]
        assert np.array_equal(b[:, 0], np.array(want, np.float32)) and not b[:, 1:].any(), name
    q16, _, kb, _ = R.fused(V, W, src, 0, 16, "given")
    assert [int(q16[R.PLANT[name] * V]) for name in ("i_inside", "i_sat", "i_leave", "i_last2")] == [-32768, 32767, 0, 32767]
    assert abs(2 * 28672) > 32767 and m >= 3              # i_leave's running sum after two workers
    e = R.PLANT["wrap"] * V
    q32 = R.fused(V, W, src, 0, 32, "given")[0]
    assert int(q32[e]) != W * (2**31 - 1) and (int(q32[e]) - W * (2**31 - 1)) % 2**32 == 0


@CASES
@pytest.mark.parametrize("rot", (False, True), ids=("plain", "rot"))
def test_byte_wire_flags_are_mixed_and_mostly_clear(V, W, src, rot):
    _, given, out = R.i8_case(V, W, src, 0, rot)
    for w, (q, flags) in out.items():
        mixed(flags)
        assert flags[3] == 1 and flags[list(R.ORDINARY)].sum() * 4 <= len(R.ORDINARY), w
        assert q.min() >= -127


def test_keys_need_the_high_word_and_the_odd_counter():
    n = 1024
    sg = lambda e0, count=n: rref.signs(count, R.SEED, **R.key(e0))
    # a counter that wraps at 2^32 (stream indices taken mod 2^39) gives other signs past the carry
    for e0, first in ((R.E0_CARRY, 128), (R.E0_CARRY256, 256)):
        wrapped = np.concatenate([sg(e0, first), sg((e0 + first) % 2**39, n - first)])
        assert np.array_equal(sg(e0)[:first], wrapped[:first])
        assert (sg(e0)[first:] != wrapped[first:]).sum() > (n - first) // 4
    assert (sg(R.E0_HIGH) != sg(R.E0_HIGH % 2**39)).sum() > n // 4
    # an odd counter: its signs are neither neighbour's, and the second call is at c + 1, not c | 1
    assert (R.E0_ODD >> 7) % 2 == 1 and (R.E0_CARRY >> 7) % 2 == 1
    for other in (R.E0_ODD - 128, R.E0_ODD + 128):
        assert (sg(R.E0_ODD) != sg(other)).sum() > n // 4
    assert (sg(R.E0_ODD)[128:256] != sg(R.E0_ODD)[:128]).sum() > 32
    for V in R.V_NEW + R.V_OLD:
        assert all(e0 % 128 == 0 and e0 % V == 0 for e0 in R.e0s(V))


@pytest.mark.parametrize("V", R.V_NEW + R.V_OLD)
def test_slices_start_on_an_odd_multiple_of_128(V):
    lo, hi = R.slice_lo(V)
    assert lo % V == 0 and (lo // max(V, 128)) % 2 == 1 and hi == lo + 9 * V and hi <= R.NBLK * V
    inside = [s for s in R.PLANT.values() if lo <= s * V < hi]
    assert inside, "the slice holds at least one planted block"
