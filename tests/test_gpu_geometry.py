"""Launch geometry: every grid-stride loop of csrc/ past its first pass, at small sizes.

The grid caps are sized for the benchmark's buckets, so at the sizes of the other tests every
thread runs its loop body once.  Here the cap is lowered (tuning key 0 in the product library;
keys 4, 5, 6 and 14 in a lab build, run once in a child process) or n is taken past a fixed cap,
and n is derived from the cap (tests/_geometry_lab.py, n_for): at least four passes, the last
one ragged inside one workgroup.  Every comparison is bit for bit against the CPU oracle, into
sentinel-filled outputs a few elements longer than the result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _geometry_lab import (BLOCK, CAPS, DEV, KEY0_CASES, LAB_IDS, REPO, X16, combine_case, dev, judge, n_for, ops,
                           passes, run_case, sent, to16)
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

COMBINE_CAP, FANIN_CAP, MULTI_CAP = 256, 256, 512      # g_combine_blocks, kFaninBlocks, the absmax_multi grids
ABSMAX_U = 4                                           # kAbsmaxU


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def all_ok(results):
    bad = [f"{label}: first differing element {first}" for label, ok, first in results if not ok]
    assert not bad, bad
    assert results


# ---- a. tuning key 0 --------------------------------------------------------------------------
def key0(cap):
    ops().set_tuning(max_blocks=16384 if cap is None else cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", list(KEY0_CASES))
def test_default_cap_kernels_stride(name, cap):
    all_ok(run_case(ops(), KEY0_CASES[name], cap, key0))


def test_sizes_make_every_loop_run_more_than_twice():
    """The arithmetic of n_for, on the host: passes of the busiest thread and the ragged last pass."""
    for cap in CAPS:
        S = cap * BLOCK
        for per, U in ((1, 1), (4, 1), (8, 1), (4, 2), (4, 4)):
            n = n_for(cap, per, U)
            items = n // per
            assert passes(cap, items) >= 4 and 64 < items % S < 128
            assert per == 1 or n % per
            if U > 1:       # chunk_loop: two U-way passes, then a full and a ragged one-chunk pass
                assert items // (U * S) == 2 and 1 <= (items - 2 * U * S) // S < U


# ---- b. fixed caps, by size -------------------------------------------------------------------
@pytest.mark.parametrize("W", [3, 6])
def test_ps_combine_past_its_cap(W):
    """W = 3: one chunk in flight, W = 6: two (chunk_loop<2>), under g_combine_blocks = 256."""
    all_ok(run_case(ops(), combine_case("ps_combine", W, S=COMBINE_CAP), COMBINE_CAP))


def absmax_regions(cap, U):
    """(name, value index) per region of a chunk_loop<U> kernel under `cap` workgroups at
    n = n_for(cap, 4, U): 16-byte chunk c holds values 4c .. 4c + 3."""
    S, n = cap * BLOCK, n_for(cap, 4, U)
    if U == 1:
        chunks = [("first pass", 5), ("second pass", S + 7), ("third pass", 3 * S - 1), ("ragged last pass", 3 * S + 68)]
    else:
        chunks = [("first U-pass, chunk 0", S // 2), ("first U-pass, last chunk", (U - 1) * S + 9),
                  ("second U-pass", U * S + 2 * S + 77), ("remainder pass", 2 * U * S + 100),
                  ("ragged remainder pass", 2 * U * S + S + 68)]
    return n, [(name, 4 * c + i % 4) for i, (name, c) in enumerate(chunks)] + [("scalar tail", n - 1)]


def noise(n, W, dtype, seed):
    """Small-magnitude buckets: host arrays as the oracle sees them (fp32) and device tensors."""
    rng = np.random.default_rng(seed)
    x0 = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    host, devs = [], []
    for w in range(W):
        x = (x0 * np.float32(1 + w / 16)).astype(np.float32)
        if dtype is torch.float32:
            host.append(x)
            devs.append(dev(x))
        else:
            t, wide = to16(x, dtype)
            host.append(wide)
            devs.append(t.to(DEV))
    return host, devs


def check_planted(call, host, devs, base, regions, workers):
    """One planted maximum per region (and worker): the kernel must return it, not the noise's."""
    o, results = ops(), []
    b = base if base is not None else np.float32(0)
    quiet = np.float32(max(np.abs(h - b).max() for h in host))
    assert quiet < 0.1
    out = sent(1, torch.float32)
    call(o, out)
    results.append(judge("noise alone", out, np.array([quiet], np.float32)))
    for w in workers:
        for name, idx in regions:
            keep = devs[w][idx].clone()
            devs[w][idx] = 3.0
            want = np.abs(np.float32(3.0) - (base[idx] if base is not None else np.float32(0))).astype(np.float32)
            out = sent(1, torch.float32)
            call(o, out)
            results.append(judge(f"maximum in the {name} of worker {w} (value {idx})", out, np.array([want], np.float32)))
            devs[w][idx] = keep
    all_ok(results)


@pytest.mark.parametrize("with_base", [False, True])
def test_absmax_finds_a_maximum_in_every_region(with_base):
    """k_absmax_f32: chunk_loop<4> under kFaninBlocks = 256 -- two 4-way passes, the one-chunk
    remainder loop twice, the scalar tail."""
    n, regions = absmax_regions(FANIN_CAP, ABSMAX_U)
    assert n % 4 and passes(FANIN_CAP, n // 4) == 2 * ABSMAX_U + 2
    host, devs = noise(n, 1, torch.float32, 40)
    base = (np.random.default_rng(41).standard_normal(n) * 1e-3).astype(np.float32) if with_base else None
    db = dev(base) if with_base else None
    check_planted(lambda o, out: o.absmax(devs[0], base=db, out=out), host, devs, base, regions, [0])


@pytest.mark.parametrize("W", [3, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_absmax_multi_finds_a_maximum_in_every_region(dtype, W):
    """k_absmax_multi_f32 / _x16: one chunk per pass under 512 workgroups, with a base; the
    maximum in every pass of worker W - 1 and of worker 0."""
    n, regions = absmax_regions(MULTI_CAP, 1)
    assert n % 4 and passes(MULTI_CAP, n // 4) == 4
    host, devs = noise(n, W, dtype, 42 + W)
    base = (np.random.default_rng(43).standard_normal(n) * 1e-3).astype(np.float32)
    db = dev(base)
    check_planted(lambda o, out: o.absmax_multi(devs, base=db, out=out), host, devs, base, regions, [W - 1, 0])
    check_planted(lambda o, out: o.absmax_multi(devs, out=out), host, devs, None, regions[-2:], [W - 1])


def test_absmax_16bit_single_bucket_past_its_cap():
    """absmax of a bf16 / fp16 bucket is the multi-bucket pass with W = 1."""
    n, regions = absmax_regions(MULTI_CAP, 1)
    for dtype in X16.values():
        host, devs = noise(n, 1, dtype, 44)
        check_planted(lambda o, out: o.absmax(devs[0], out=out), host, devs, None, regions, [0])


CHECKSUM_OVER = n_for(FANIN_CAP, 4) + 2                 # 4 passes of 16-byte chunks, n % 4 == 3


@pytest.mark.parametrize("n", [1, 3, 4, 1023, CHECKSUM_OVER])
def test_checksum_sizes(n):
    o = ops()
    from ina_amd import _lib
    assert n < 2000 or (n % 4 and passes(FANIN_CAP, n // 4) == 4)
    x = np.random.default_rng(n).integers(-2**31, 2**31, n + 1, dtype=np.int64).astype(np.int32)
    d = dev(x)
    results = []
    for tag, view, host in (("aligned", d[:n], x[:n]), ("4 bytes off", d[1:], x[1:])):
        assert view.data_ptr() % 16 == (0 if tag == "aligned" else 4)
        out = sent(1, torch.int32)
        _lib.check(o.load().ina_checksum_i32(view.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "checksum")
        results.append(judge(f"checksum n={n} {tag}", out, np.array([orc.checksum_i32(host)], np.uint32)))
    all_ok(results)


# ---- 2. the same under the lab build's caps ---------------------------------------------------
LAB_TIMEOUT = 900        # seconds for the whole child (one process, every case)


@pytest.fixture(scope="module")
def lab_records(tmp_path_factory):
    """tests/_geometry_lab.py once, in a fresh process on libina_lab.so: its records by name."""
    from ina_amd import _lib
    lab = os.path.join(os.path.dirname(_lib.LIB_PATH), "libina_lab.so")
    assert os.path.exists(lab), f"{lab} is not built (make -C csrc lab; __graft_entry__.build() makes it)"
    out = str(tmp_path_factory.mktemp("geometry") / "lab.jsonl")
    env = dict(os.environ, INA_LIBRARY="libina_lab.so")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_geometry_lab.py"), out], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=LAB_TIMEOUT)
    recs = {}
    if os.path.exists(out):
        with open(out) as fh:
            recs = {rec["name"]: rec for rec in map(json.loads, fh)}
    return r, recs


def test_lab_child_ran_every_case(lab_records):
    r, recs = lab_records
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert f"geometry lab child ok: {len(LAB_IDS)} records" in r.stdout
    assert sorted(recs) == sorted(LAB_IDS)


@pytest.mark.parametrize("name", LAB_IDS)
def test_lab_caps_change_only_speed(lab_records, name):
    r, recs = lab_records
    assert name in recs, f"the child stopped before {name}: {r.stderr[-1500:]}"
    rec = recs[name]
    assert rec["ok"], f"{rec['what']}: first differing element {rec['first']}"
    assert rec["checks"] > 0
