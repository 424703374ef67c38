"""The bulk entry points on a side stream and under hipGraph replay (every
device ina_* call is asynchronous on the caller's stream and can be captured).  tests/_graph.py holds the
table -- one row per entry point -- and the yardsticks; nothing here is compared with an eager run of
the code under test.

1. stream order: on a non-default stream, behind a device-side delay, the copy of fresh inputs over
   stale ones, the call, the copy-out.  An event behind the delay is still pending when the call has
   returned (else the case is void and fails), so a launch or a clear issued on any other stream runs
   before the copy and the sentinel fill of the outputs: it reads the stale inputs, or is overwritten;
2. replay: captured once (one stream, torch's default global capture mode) with caller-supplied
   outputs, replayed on three fresh inputs: flags and a large maximum, then all-zero flags and a smaller
   maximum -- which a clear left out of the graph fails -- then mixed.  Error-feedback rows carry one
   residual through the three replays; stochastic-rounding and rotation rows repeat the captured
   (seed, step, sub, e0) on every replay, and a second capture at step + 1 differs.
"""
import time

import numpy as np
import pytest
import torch

from tests import _graph as G
from tests._graph import DEV, ROWS, STEP, Stage, capped, mods, pinned, warm, wide

gpu = pytest.mark.gpu
BY_NAME = {r.name: r for r in ROWS}


@pytest.fixture(scope="module")
def cycles_per_ms():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ina_amd import ops  # noqa: F401  (fails loudly if libina.so is missing)
    return G.sleep_cycles_per_ms()


def test_table_covers_the_entry_points():
    """The coverage rule, over the `_lib` prototype names: every entry point that clears in front of its
    kernel has a row whose output must go down in phase 2 (or, the checksum, must not accumulate); two
    single-launch rows per source, one over W buckets where the source has such an entry point; W = 3 and
    a run-time W of 17 both occur; one grid-cap-1 row per family; every device entry point of the four newer wire
    sources (G.WIRES) has a row.  Then, from the yardsticks alone, that the phases do what the GPU tests rely on:
    flags and shifts go down in phase 2 -- with the carried state too -- and a keyed row's first output differs
    between STEP and STEP + 1 on the very inputs test_replay_repeats_the_captured_key draws."""
    from ina_amd import _lib
    sigs = {}
    for name in dir(_lib):
        if name.startswith("SIGNATURES"):
            sigs.update(getattr(_lib, name))
    named = {p for r in ROWS for p in r.protos}
    assert named <= set(sigs), sorted(named - set(sigs))
    assert len(BY_NAME) == len(ROWS)
    for p in G.CLEARING:
        rs = [r for r in ROWS if p in r.protos]
        assert rs, p
        assert all(r.flags or r.peak or p == "ina_checksum_i32" for r in rs), p
    clearing_rows = {r.name for r in ROWS if set(r.protos) & G.CLEARING}
    for src, has_w in G.SINGLE.items():
        rs = [r for r in ROWS if r.src == src and r.name not in clearing_rows]
        assert len(rs) >= 2, (src, rs)
        if has_w:
            assert any("_w3" in r.name or "_w17" in r.name for r in rs), src
    assert any("_w3" in r.name for r in ROWS) and any("_w17" in r.name for r in ROWS)
    capped_srcs = {r.src for r in ROWS if r.cap}
    assert capped_srcs >= {"ina_kernels.hip", "ina_x16.hip", "ina_sr.hip", "ina_reduce_sr.hip", "ina_shard.hip",
                           "ina_blk.hip", "ina_ef.hip", "ina_rot.hip", "ina_i8.hip", "ina_i8_gather.hip",
                           "ina_i8_ef.hip", "ina_i8_sr.hip", "ina_i4.hip"}, capped_srcs
    assert G.WIRES <= named, sorted(G.WIRES - named)
    assert all(sigs[p][-1] is sigs["ina_sum_i8_slices"][-1] for p in G.WIRES)      # each ends in the stream argument
    for p in G.WIRES - {"ina_dequantize_i8_gather"} - {q for q in G.WIRES if "block_scales" in q}:
        rs = [r for r in ROWS if p in r.protos]                   # a quantiser clears flags, a requantiser writes shifts
        assert any(r.flags or r.shifts or p == "ina_sum_i4_slices" for r in rs), p
    rng = np.random.default_rng(1)
    for r in ROWS:                                    # the phases do what the replays rely on
        w = [r.want(wide(r.ins(rng, p)), STEP) for p in (1, 2, 3)]
        if r.flags:
            assert w[0][r.flags].any() and not w[1][r.flags].any() and w[2][r.flags].any(), r.name
            assert not np.array_equal(w[0][r.flags], w[2][r.flags]), r.name
        if r.peak:
            assert w[0][r.peak][0] > 100 * w[1][r.peak][0] > 0, r.name
        if r.shifts:                                  # a stale shift byte of phase 1 would show in phase 2
            assert r.shifts in r.odd and w[0][r.shifts].max() >= 1 and not w[1][r.shifts].any() and w[2][r.shifts].any(), r.name
            assert not np.array_equal(w[0][r.shifts], w[2][r.shifts]), r.name
        if r.name == "i4_sum_requant_w33":
            assert {1, 2} <= set(w[0][r.shifts].tolist()), w[0][r.shifts]
        if r.state and r.flags:                       # test_replay's chain: the state the yardstick leaves goes on
            g = np.random.default_rng(200 + len(r.name))
            h, seen = None, []
            for i, ph in enumerate([r.ins(g, p) for p in (1, 2, 3)]):
                h = {**wide(ph), **({n: want[n] for n in r.state} if i else {})}
                want = r.want(h, STEP)
                seen.append(want[r.flags].copy())
            assert seen[0].any() and not seen[1].any() and seen[2].any() and not np.array_equal(seen[0], seen[2]), r.name
            assert all(np.isfinite(want[n]).all() and want[n].any() for n in r.state), r.name
        if r.keyed:
            hosts = wide(r.ins(np.random.default_rng(300 + len(r.name)), r.key_phase))
            first = next(iter(r.outs))
            assert not np.array_equal(r.want(hosts, STEP)[first], r.want(hosts, STEP + 1)[first]), r.name


def _read(st):
    torch.cuda.synchronize()
    return {n: st.t[n].cpu() for n in st.names()}


@gpu
@pytest.mark.parametrize("name", list(BY_NAME))
def test_stream_order(name, cycles_per_ms):
    row = BY_NAME[name]
    rng = np.random.default_rng(100 + len(name))
    stale, fresh = row.ins(rng, 1), pinned(row.ins(rng, 3))
    st = Stage(row, stale)
    s = torch.cuda.Stream(DEV)
    behind = torch.cuda.Event()
    out_host = {n: torch.empty_like(st.t[n], device="cpu").pin_memory() for n in st.names()}
    with capped(row):
        warm(row, st, stale, s)                       # kernels loaded, symbols checked
        st.load(stale)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(G.DELAY_MS * cycles_per_ms))
            behind.record(s)
            st.sentinel_outputs()                     # behind the delay too: a clear that ran early is overwritten
            t0 = time.perf_counter()
            st.load(fresh, non_blocking=True)
            row.call(mods(), st.t, STEP)
            enqueue_ms = (time.perf_counter() - t0) * 1e3
            pending = not behind.query()
            for n, h in out_host.items():
                h.copy_(st.t[n], non_blocking=True)
    s.synchronize()
    print(f"{name}: host enqueue of the copies and the call {enqueue_ms:.3f} ms, delay {G.DELAY_MS} ms")
    assert pending, f"void: the {G.DELAY_MS} ms delay ended before the call returned ({enqueue_ms:.3f} ms)"
    st.check(out_host, row.want(wide(fresh), STEP), "stream order")


def _capture(row, st, s, step):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        row.call(mods(), st.t, step)
    return g


@gpu
@pytest.mark.parametrize("name", list(BY_NAME))
def test_replay(name, cycles_per_ms):
    row = BY_NAME[name]
    rng = np.random.default_rng(200 + len(name))
    phases = [row.ins(rng, p) for p in (1, 2, 3)]
    st = Stage(row, phases[0])
    s = torch.cuda.Stream(DEV)
    with capped(row):                                 # the grid cap is read at capture time
        warm(row, st, row.ins(rng, 3), s)
        g = _capture(row, st, s, STEP)
    st.load(phases[0])                                # the state the replays start from (the warm-up moved it)
    h = None
    for i, ph in enumerate(phases):
        st.load(ph, skip=row.state if i else ())
        st.sentinel_outputs()
        torch.cuda.synchronize()
        g.replay()
        h = {**wide(ph), **({n: want[n] for n in row.state} if i else {})}
        want = row.want(h, STEP)
        st.check(_read(st), want, f"replay {i + 1}")
        if row.flags:
            assert bool(want[row.flags].any()) == (i != 1), i


@gpu
@pytest.mark.parametrize("name", [r.name for r in ROWS if r.keyed])
def test_replay_repeats_the_captured_key(name, cycles_per_ms):
    """A replay draws what the captured (seed, step) draws, every time; the step advances only with a new
    capture, whose replays are the yardstick's at step + 1 and differ from the first graph's."""
    row = BY_NAME[name]
    rng = np.random.default_rng(300 + len(name))
    hosts = row.ins(rng, row.key_phase)
    st = Stage(row, hosts)
    s = torch.cuda.Stream(DEV)
    warm(row, st, hosts, s)
    got = []
    for step in (STEP, STEP + 1):
        g = _capture(row, st, s, step)
        for rep in range(2):
            st.load(hosts)                            # a state the call updates starts every replay from the same values
            st.sentinel_outputs()
            torch.cuda.synchronize()
            g.replay()
            out = _read(st)
            st.check(out, row.want(wide(hosts), step), f"step {step} replay {rep + 1}")
        got.append(out)
    first = next(iter(row.outs))
    assert not torch.equal(got[0][first], got[1][first])
