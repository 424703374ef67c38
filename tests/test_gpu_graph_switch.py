"""The switch under hipGraph replay (csrc/ina_switch.hip).  A captured call freezes what the host reads at
call time: the sort epoch the kernels tag their control words with, the tuning and the plan.  Every replay
of one graph then meets the tags the previous replay left under its own epoch; `unsorted[0]`, "the batch
is not in slot order", is only ever set.  One captured call is replayed over a seeded walk of 37 batches
of 16,000 rows (V = 32, 8 senders x 2,000 slots; an ack run takes one sender's place) that holds every
ordered pair of {in_order, runs, runs_acks, near40, near1500, shuffled} and starts in slot order; the
reference is the CPU oracle with state carried from replay to replay -- actions, rewritten rows, count /
frag / regs of the touched slots after every replay, every register after the last.

Every mode is captured twice: under the default sort chunks, where near1500 sorts at this size, and under
set_tuning(switch_sort_rounds=16) around the capture (the tuning is frozen there), where it reaches the
near-sorted lists as in _scratch_reuse.main.

Measured on an MI355X (the paths each mode prints): after the first out-of-order replay of a graph an
in-order batch is no longer "in_order" -- it equals the oracle and takes the near-sorted lists
("local") -- see INTEGRATION.md section 5.  Per kind, in all eight modes and both pools: in_order ->
in_order (first replay) then local; runs, runs_acks -> runs; near40 -> local; near1500 -> sorted (local
under switch_sort_rounds=16); shuffled -> sorted, or local where its slots fit the lists' scan budget.  The
digit-pass graph sorts every batch.  Two graphs alternating retake in_order whenever the other graph ran
last.  The tests assert these.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

from _scratch_reuse import (DEV, DIGIT_KINDS, REPLAY_KINDS, REPLAY_PER, REPLAY_SEQ0, check_regs, check_rows, host,
                            reg_views, replay_reference)

pytestmark = pytest.mark.gpu
V = 32
K, WS = 16, 1 / 9
N_LOCAL = REPLAY_PER * V - 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ina_amd import ops  # noqa: F401  (fails loudly if libina.so is missing)


def ops():
    from ina_amd import ops as o
    return o


class Captured:
    """One switch, the row buffers every replay is copied into, and the call of `mode` over them."""

    def __init__(self, o, mode, num_slots, npk, seed=0):
        self.o, self.mode = o, mode
        self.fused, self.split = mode.startswith("apply"), "split" in mode
        self.blk = mode.endswith("blk")
        stride = o.nga_stride(V)
        self.sw = o.Switch(V, num_slots=num_slots, switch_id=1, device=DEV)
        self.d = torch.zeros((npk, stride), dtype=torch.uint8, device=DEV)
        self.desc = torch.zeros(npk, dtype=torch.int64, device=DEV)
        self.act = torch.zeros(npk, dtype=torch.uint8, device=DEV)
        self.hdr = torch.zeros((npk, 16), dtype=torch.uint8, device=DEV)
        self.pay = torch.zeros((npk, 4 * V), dtype=torch.uint8, device=DEV)
        if self.fused:
            g = torch.Generator(device="cpu").manual_seed(77 + seed)
            self.local = torch.zeros(N_LOCAL, device=DEV)
            self.out = torch.zeros(N_LOCAL, device=DEV)
            self.acks = torch.zeros((REPLAY_PER, 16 if self.split else stride), dtype=torch.uint8, device=DEV)
            self.ad = torch.zeros(REPLAY_PER, dtype=torch.int64, device=DEV)
            self.k = (torch.randint(10, 21, (REPLAY_PER,), dtype=torch.int8, generator=g).to(DEV) if self.blk else K)
            # the unfused pair, run eagerly on a second switch
            self.two = o.Switch(V, num_slots=num_slots, switch_id=1, device=DEV)

    def fill(self, pk, rng=None):
        """The batch into the captured buffers (and the descriptors, split rows, PS inputs of the mode)."""
        o = self.o
        self.d.copy_(torch.from_numpy(pk))
        if self.mode != "process_nodesc":
            o.nga_descriptors(self.d, out=self.desc)
        if self.split:
            self.hdr[:, :15] = self.d[:, :15]
            self.pay.copy_(self.d[:, 15:15 + 4 * V])
        if self.fused:
            self.local.copy_(torch.from_numpy(rng.standard_normal(N_LOCAL).astype(np.float32)))
            self.out.fill_(float("nan"))
            self.acks.zero_()
            self.ad.zero_()

    def call(self):
        sw, m = self.sw, self.mode
        if m == "process":
            sw.process(self.d, actions=self.act, desc=self.desc)
        elif m == "process_nodesc":
            sw.process(self.d, actions=self.act)
        elif m == "process_split":
            sw.process_split(self.hdr, self.pay, actions=self.act, desc=self.desc)
        elif m == "sort_run":
            sw.sort(self.d, self.desc, actions=self.act)
            sw.run(self.d, self.act)
        elif self.split:
            sw.process_apply_split(self.hdr, self.pay, REPLAY_SEQ0, self.local, self.k, WS, out=self.out,
                                   ack_hdr=self.acks, ack_desc=self.ad, actions=self.act, desc=self.desc)
        else:
            sw.process_apply(self.d, REPLAY_SEQ0, self.local, self.k, WS, out=self.out, acks=self.acks,
                             ack_desc=self.ad, actions=self.act, desc=self.desc)

    def rows(self):
        d = host(self.d).copy()
        if self.split:
            d[:, :15] = host(self.hdr)[:, :15]
            d[:, 15:15 + 4 * V] = host(self.pay)
        return d

    def check_ps(self, pk, want_act, tag):
        """out, the ack rows and their descriptors against process + apply_completed[_blk] run eagerly, bit
        for bit, for every slot that completes at most once in the batch.  These batches mix degrees, so a
        few slots complete twice; what such a slot keeps is unspecified (include/ina.h, ina_switch_ps: two
        completions of one slot are written by different waves; measured, slot 1488 of a runs_acks batch
        kept the earlier, the later, or values that are neither's whole row from run to run, and the unfused
        apply is as unordered), so those slots are left out -- and counted: they stay under 5 %."""
        o, two = self.o, self.two
        d2 = torch.from_numpy(pk).to(DEV)
        act2 = two.process(d2, desc=o.nga_descriptors(d2))
        assert np.array_equal(host(act2), host(self.act)), tag
        out2 = torch.full_like(self.local, float("nan"))
        acks2 = torch.zeros((REPLAY_PER, d2.shape[1]), dtype=torch.uint8, device=DEV)
        if self.blk:
            o.apply_completed_blk(d2, act2, V, REPLAY_SEQ0, self.local, self.k, WS, out=out2, acks=acks2)
        else:
            o.apply_completed(d2, act2, V, REPLAY_SEQ0, self.local, K, WS, out=out2, acks=acks2)
        frag = host(d2)[:, 11:15].astype(np.int64) @ (1 << np.array([24, 16, 8, 0], np.int64))
        slots, times = np.unique(frag[want_act == orc.ACT_FWD_AGG] - REPLAY_SEQ0, return_counts=True)
        nslot = -(-N_LOCAL // V)
        once = np.ones(nslot, bool)
        multi = slots[(times > 1) & (slots >= 0) & (slots < nslot)]
        once[multi] = False
        assert len(slots) > 100 and len(multi) < 0.05 * len(slots), (tag, len(slots), len(multi))
        same = np.ones(nslot * V, bool)
        same[:N_LOCAL] = host(self.out).view(np.uint32) == host(out2).view(np.uint32)
        bad = np.flatnonzero(~same.reshape(-1, V).all(1) & once)
        assert bad.size == 0, (tag, "out differs at slots", bad[:8])
        assert np.array_equal(host(self.acks)[once, :15], host(acks2)[once, :15]), tag
        assert np.array_equal(host(self.ad)[once], host(o.nga_descriptors(acks2))[once]), tag


def capture(c, stream, pk, rng, n_graphs=1):
    """Warm-up on the capture stream (it sizes the scratch), registers back to zero, then the graph(s)."""
    c.fill(pk, rng)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        c.call()
    stream.synchronize()
    for sw in [c.sw] + ([c.two] if c.fused else []):
        sw.count.zero_()
        sw.frag.zero_()
        sw.regs.zero_()
    torch.cuda.synchronize()
    graphs = []
    for _ in range(n_graphs):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            c.call()
        graphs.append(g)
    return graphs


def replay_all(c, graphs, steps, ref, hi, num_slots):
    """Every step through graphs[i % len]: the oracle's results first, then the path it took."""
    rng = np.random.default_rng(5)
    ptr = c.sw._scratch.data_ptr()
    paths = []
    for i, (kind, pk, want_pk, want_act, regs) in enumerate(steps):
        tag = (c.mode, i, kind)
        c.fill(pk, rng)
        torch.cuda.synchronize()
        graphs[i % len(graphs)].replay()
        torch.cuda.synchronize()
        assert c.sw._scratch.data_ptr() == ptr, tag
        check_rows(host(c.act), c.rows(), want_act, want_pk, False, tag)
        check_regs(c.sw, regs, hi, tag)
        paths.append(c.sw.batch_path(len(pk)))
        if c.fused:
            c.check_ps(pk, want_act, tag)
    check_regs(c.sw, reg_views(ref), num_slots, (c.mode, "final"))
    kinds = [k for k, *_ in steps]
    print(f"{c.mode} pool {num_slots} graphs {len(graphs)}: " + " ".join(f"{k}:{p}" for k, p in zip(kinds, paths)))
    print(f"  {c.mode} pool {num_slots}: " + "".join(p[0].upper() for p in paths))
    return kinds, paths


def after_disorder(kinds, paths):
    """The paths of the in-order batches that follow the first replay that was not "in_order"."""
    first = next(i for i, p in enumerate(paths) if p != "in_order")
    return [p for k, p in list(zip(kinds, paths))[first + 1:] if k == "in_order"]


MODES = ["process", "process_nodesc", "process_split", "sort_run", "apply", "apply_split", "apply_blk",
         "apply_split_blk"]


@pytest.mark.parametrize("rounds", [0, 16])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("num_slots", [1 << 17, 1 << 20])
def test_one_graph_over_every_pair_of_kinds(num_slots, mode, rounds):
    """rounds = 0: the default sort chunks, under which near1500 sorts at this size, so the walk holds the
    four bulk paths and every change between runs, lists and sort.  rounds = 16: captured under
    set_tuning(switch_sort_rounds=16), the 4,096-packet chunks with which near1500 reaches the lists, as in
    _scratch_reuse.main -- the tuning is frozen at capture, so the default is back before the first replay.
    There the lists run over a large-jitter batch, whose detection waves store their keys, before and
    after every other kind."""
    o = ops()
    steps, ref, hi = replay_reference(num_slots, V)
    c = Captured(o, mode, num_slots, len(steps[0][1]))
    s = torch.cuda.Stream(DEV)
    o.set_tuning(switch_sort_rounds=rounds)
    try:
        graphs = capture(c, s, steps[0][1], np.random.default_rng(4))
    finally:
        o.set_tuning(switch_sort_rounds=0)
    kinds, paths = replay_all(c, graphs, steps, ref, hi, num_slots)
    assert paths[0] == "in_order"                       # seen before the sticky tag is set
    # the "descent found" tag stays: no later batch in slot order of this graph is "in_order" again
    after = after_disorder(kinds, paths)
    assert len(after) >= 5 and "in_order" not in after, paths
    by_kind = {k: {p for kk, p in zip(kinds, paths) if kk == k} for k in REPLAY_KINDS}
    assert by_kind["runs"] == by_kind["runs_acks"] == {"runs"} and by_kind["near40"] == {"local"}, by_kind
    if rounds == 16:
        assert by_kind["near1500"] == {"local"}, by_kind
        want = ("runs", "local")
    else:
        assert {"in_order", "runs", "local", "sorted"} <= set(paths), paths
        want = ("runs", "local", "sorted")
    follows = set(zip(paths, paths[1:]))
    for a in want:
        for b in want:
            assert a == b or (a, b) in follows, (a, b, paths)


@pytest.mark.parametrize("num_slots", [1 << 17, 1 << 20])
def test_digit_passes_graph(num_slots):
    """Captured under set_tuning(switch_sort=3): the tuning is read at capture time, so the replays run
    the LSD digit passes although the default is back before the first of them."""
    o = ops()
    steps, ref, hi = replay_reference(num_slots, V, DIGIT_KINDS)
    c = Captured(o, "process", num_slots, len(steps[0][1]))
    s = torch.cuda.Stream(DEV)
    o.set_tuning(switch_sort=3)
    try:
        graphs = capture(c, s, steps[0][1], None)
    finally:
        o.set_tuning(switch_sort=0)
    kinds, paths = replay_all(c, graphs, steps, ref, hi, num_slots)
    assert set(paths) == {"sorted"}, paths              # the digit passes sort every batch, in order or not


@pytest.mark.parametrize("mode", ["process", "apply_split"])
def test_two_graphs_over_one_scratch(mode):
    """The same call captured twice over one Switch and scratch, replayed alternately: two frozen epochs,
    each meeting the other's tags."""
    o = ops()
    num_slots = 1 << 17
    steps, ref, hi = replay_reference(num_slots, V)
    c = Captured(o, mode, num_slots, len(steps[0][1]))
    s = torch.cuda.Stream(DEV)
    graphs = capture(c, s, steps[0][1], np.random.default_rng(4), n_graphs=2)
    kinds, paths = replay_all(c, graphs, steps, ref, hi, num_slots)
    assert {"runs", "local", "sorted"} <= set(paths), paths
    # each graph clears the other's tag: a batch in slot order is "in_order" again after the other graph ran
    assert "in_order" in after_disorder(kinds, paths), paths
