"""tests/_wire_limits.py on the yardsticks alone (no GPU): the builders reach what tests/test_gpu_wire_limits.py
means them to reach -- the ragged tails, the shifts per (V, G), the lanes that hold the maxima, the flags of the
plants -- so a later edit to them cannot quietly empty the device tests."""
import numpy as np
import pytest

from tests import _i4_ref as r4
from tests import _rot_limits as R
from tests import _wire_limits as L
from tests._limits import mixed

CASES = pytest.mark.parametrize("V,W,src", R.CASES, ids=lambda v: str(v))


def test_slice_counts_are_the_instances_and_the_loop_remainders():
    assert set(L.G_STATIC) == {4, 16} and [G % 16 for G in L.G_LOOP] == [5, 15, 15, 15]
    assert [G // 16 for G in L.G_LOOP] == [0, 0, 1, 3]                   # a last batch of 15 after 0, 1 and 3 whole ones
    assert L.G_N % L.G_V == 0 and L.rag_of(L.G_N) == 2 and L.G_N // 16 == 5
    for kind in L.SUMS:
        lo, hi = L.lim(kind)
        sums = (r4.unpack(L.g_case(kind, 63, "extreme")[0]) if L.nibble(kind) else L.g_case(kind, 63, "extreme")[0]).astype(int).sum(0)
        assert sums.min() == 63 * lo and sums.max() == 63 * hi, kind
    assert (63 * -8, 63 * 7) == (-504, 441)


def test_ragged_tails_cover_every_dword_count():
    assert [L.rag_of(n) for n in L.RAG_SUM_N] == [2, 2, 2] and [n // 32 for n in L.RAG_SUM_N] == [0, 1, 2]
    v8 = [(V * nblk // 32, L.rag_of(V * nblk)) for V, nblk in L.RAG_RQ if V == 8]
    assert v8 == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]           # no whole chunk, then one
    assert [(V * nblk // 32, L.rag_of(V * nblk)) for V, nblk in L.RAG_RQ if V == 16] == [(0, 2), (1, 0), (1, 2)]
    for G in L.RAG_G:
        for V, nblk in L.RAG_RQ:
            parts, (q, sh) = L.rag_rq_case(G, V, nblk)
            S = r4.sum_slices(list(parts)).reshape(nblk, V)
            assert np.abs(S).max() == np.abs(S[-1]).max() == 8 * G and sh[-1] == {3: 0, 16: 1, 33: 2}[G]
            assert not sh[:-2].any() and (nblk == 1 or sh[-2] == {3: 0, 16: 0, 33: 1}[G])
        for n in L.RAG_SUM_N:
            s = L.rag_sum_case(G, n)[1][0]
            assert s[n - 1] == -8 * G and s[n - 8] == 7 * G


@pytest.mark.parametrize("kind", L.REQUANT)
@pytest.mark.parametrize("V", L.ALL_V)
def test_block_maxima_sit_in_the_first_the_last_and_a_middle_lane(kind, V):
    per, want_top = L.lane_values(kind), 3 if L.nibble(kind) else 7
    for G in L.V_G:
        parts, (q, sh), planted = L.v_case(kind, V, G)
        S = (r4.sum_slices(list(parts)) if L.nibble(kind) else parts.astype(int).sum(0)).reshape(L.NBLK, V).astype(int)
        where = np.abs(S).argmax(1)
        assert (np.abs(S) == np.abs(S).max(1)[:, None]).sum(1).tolist() == [1] * L.NBLK          # one maximum a block
        assert where.tolist() == [L.max_pos(b, V) for b in range(L.NBLK)] and np.array_equal(S[np.arange(L.NBLK), where], planted)
        table = L.NIBBLE_TARGETS if L.nibble(kind) else L.BYTE_TARGETS
        assert sh.tolist() == [table[abs(int(t))] for t in planted]
        if G == 64:
            assert set(sh.tolist()) == set(range(want_top + 1)) and planted.min() == L.lim(kind)[0] * 64
        lanes = V // per                                                   # the group the maximum crosses
        if lanes > 1:
            in_lane = where // per
            assert {0, lanes - 1, lanes // 2} <= set(in_lane.tolist())
            for lane in (0, lanes - 1):                                    # each with a shift above 0 at G = 64
                assert G == 3 or sh[in_lane == lane].max() >= 1
    assert V < 32 or V // 16 > 1                                           # every V >= 32 crosses lanes for bytes


@CASES
@pytest.mark.parametrize("rot", (False, True), ids=("plain", "rot"))
def test_nibble_flags_are_mixed_and_minus_8_is_never_asked_for(V, W, src, rot):
    kb, given, out = L.q4_case(V, W, src, 0, rot)
    assert given[1] == -128 and given[3] == min(int(kb[3]) + 8, 127)
    for w, (q, flags) in out.items():
        mixed(flags)
        assert flags[3] == 1 and flags[list(R.ORDINARY)].sum() * 4 <= len(R.ORDINARY), w
        assert flags[[R.PLANT[p] for p in ("nan", "inf2", "nan_inf")]].tolist() == [1, w in (1, 2), w in (0, W - 1)], w
        assert not flags[[R.PLANT[p] for p in ("zero", "negzero")]].any()
        assert r4.unpack(q).min() >= -7 and r4.unpack(q).max() == 7
    assert [int(kb[R.PLANT[p]]) for p in ("zero", "nan", "negzero", "inf2")] == [127, 127, 127, -126]


@CASES
def test_byte_siblings_flag_and_the_residual_heals(V, W, src):
    for rot in (False, True):
        for case in (L.sr_case(V, W, src, rot), L.ef_case(V, W, src, rot)):
            for w, got in case[2].items():
                mixed(got[1])
                assert got[1][3] == 1 and got[0].min() >= -127, w
        for w, (q, flags, res) in L.ef_case(V, W, src, rot)[2].items():
            assert np.isfinite(res).all() and res.any() and not res[R.blk("nan", V)].any(), w
    assert np.isfinite(L.residuals(V, W)).all()


def test_keys_slices_and_views():
    for V in (32, 128, 256):
        for e0 in R.e0s(V):
            assert not np.array_equal(R.canon(L.gather_case(V, e0)[3]), R.canon(L.gather_case(V)[3]))
    q8, sh, kb, y = L.gather_case(32)
    assert sh[9] > 7 and set(np.minimum(sh, 7).tolist()) == set(range(8))
    assert L.SHARD // 2 == 3 * 64 and L.SHARD % L.VIEW_V == 0            # nibble views at odd multiples of 64 bytes
    for kind in L.SUMS:
        for G in L.V_G:
            recv, n, want = L.view_case(kind, G)
            assert recv.shape == (G, L.SHARD // (2 if L.nibble(kind) else 1)) and want[0].size == n
    assert L.rag_of(L.view_case("i4.sum", 3)[1]) == 3
    assert L.view_case("i4.rq", 64)[2][1].max() == 3 and L.view_case("i8.rq", 64)[2][1].max() >= 5
