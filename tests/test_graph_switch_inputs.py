"""The inputs of tests/test_gpu_graph_switch.py, checked without a GPU: the replay sequences hold every
ordered pair of kinds, every batch of a graph has the same number of rows, and the oracle accepts the
sequence (tests/_scratch_reuse.py builds them).  An edit then cannot drop a pair silently."""
import numpy as np
import pytest

from oracle import oracle as orc

from _scratch_reuse import DIGIT_KINDS, REPLAY_KINDS, expected_paths, replay_kinds, replay_reference


@pytest.mark.parametrize("kinds", [REPLAY_KINDS, DIGIT_KINDS])
@pytest.mark.parametrize("seed", [2000 + (1 << 17) % 991, 2000 + (1 << 20) % 991, 5])
def test_sequence_holds_every_ordered_pair(kinds, seed):
    seq = replay_kinds(seed + len(kinds), kinds)
    assert seq[0] == "in_order" and len(seq) == len(kinds) ** 2 + 1
    assert set(zip(seq, seq[1:])) == {(a, b) for a in kinds for b in kinds}


@pytest.mark.parametrize("kinds", [REPLAY_KINDS, DIGIT_KINDS])
def test_oracle_accepts_the_sequence(kinds):
    num_slots = 1 << 17
    steps, ref, hi = replay_reference(num_slots, 32, kinds)
    assert [k for k, *_ in steps] == replay_kinds(2000 + num_slots % 991 + len(kinds), kinds)
    assert {len(pk) for _, pk, *_ in steps} == {16000}
    paths = set()
    for kind, pk, want_pk, want_act, regs in steps:
        assert want_pk.shape == pk.shape and want_act.shape == (len(pk),)
        assert (want_act == orc.ACT_FWD_AGG).any() or (want_act == orc.ACT_DROP).any(), kind
        paths |= expected_paths(pk, num_slots, kind, 2000, 1)
    # the batches alone already promise the four bulk paths (the sort only where the graph sorts)
    assert paths >= ({"in_order", "runs", "local", "sorted"} if kinds is REPLAY_KINDS else {"in_order", "local"})
    assert sum(int((a == orc.ACT_FWD_AGG).sum()) for *_, a, _ in steps) > 0
    cnt, frag, regs = (np.asarray(x) for x in steps[-1][4])
    assert regs.any() or cnt.any() or frag.any()
