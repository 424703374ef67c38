"""Yardstick and shared cases of the block-scaled int16 wire tests (include/ina_shard_blk.h): the
oracle's own quantize_i16_wire / i16_wire_finish with each block's k, beside tests/_blk_ref.py.

The oracle treats every element (and every slot of V values for the flags) on its own, so its result
on block s alone at k = kblk[s] is the slice of its whole-bucket result at that k: it is called once
per DISTINCT scale over the whole bucket and block s takes its rows from the call at its own scale
(at most 254 calls where V = 1 would otherwise need one per element).  Nothing here calls a
block-scaled entry point except check_case, which compares the library with these references.

Run as a script (tests/test_gpu_shard_blk.py does, in a child process under the lab build of the
library, the one build that accepts the elementwise grid cap, tuning key 14): the grid-stride case
with a grid of two workgroups."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "distributed-training-ina_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import oracle as orc          # noqa: E402
from tests import _blk_ref as ref         # noqa: E402

DEV = "cuda:0"


def _by_scale(n, V, kb, fn):
    """fn(k) -> (arrays of n values, arrays of one entry per block) over the whole bucket at the
    global k; block s takes its part of fn(keff(kb[s]))."""
    nblk = (n + V - 1) // V
    ke = np.maximum(np.asarray(kb[:nblk], np.int64), -126)         # a given -127 / -128 is read as -126
    of_value = np.repeat(ke, V)[:n]
    vals = flags = None
    for k in np.unique(ke):
        v, f = fn(int(k))
        if vals is None:
            vals, flags = [np.empty_like(a) for a in v], [np.empty_like(a) for a in f]
        for o, a in zip(vals, v):
            o[of_value == k] = a[of_value == k]
        for o, a in zip(flags, f):
            o[ke == k] = a[ke == k]
    return vals, flags


def wire_ref(x, kb, V):
    x = np.ascontiguousarray(x, np.float32)
    return _by_scale(x.size, V, kb, lambda k: ([orc.quantize_i16_wire(x, k)], []))[0][0]


def finish_ref(wsum, kb, V):
    """(int16 sums, fp32 y, one flag per block)"""
    wsum = np.ascontiguousarray(wsum, np.int32)

    def at(k):
        o16, y, f = orc.i16_wire_finish(wsum, k, V)
        return [o16, y], [f]
    (o16, y), (f,) = _by_scale(wsum.size, V, kb, at)
    return o16, y, f


def same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(got.view(f"u{got.itemsize}") != want.view(f"u{want.itemsize}"))      # bit for bit
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def ranks_bucket(n, V, seed, special=True):
    """[3, n] fp32 from _blk_ref.bucket (neighbouring blocks carry different k), with one NaN and one
    +inf planted where the bucket has room for them."""
    x = ref.bucket(np.random.default_rng(seed), 3, n, V)
    if special and n >= 8:
        x[1, 1] = np.nan
        x[2, n - 2] = np.inf
    return x


def given_scales(x, V):
    """The agreed scales with 3 added to every third block: there single ranks and the sum saturate."""
    kb = ref.kblk_ref(x, V, degree=3, bits=16).astype(np.int64)
    kb[::3] += 3
    return np.minimum(kb, 127).astype(np.int8)


class Expected:
    """References of one (bucket, scales): computed once, shared by the aligned and the offset run."""

    def __init__(self, x, kb, V):
        self.x, self.kb, self.V = x, kb, V
        self.wires = [wire_ref(r, kb, V) for r in x]
        self.wsum = np.sum([w.astype(np.int64) for w in self.wires], axis=0).astype(np.int32)
        self.o16, self.y, self.flags = finish_ref(self.wsum, kb, V)


def run_case(exp, off, tag):
    """Both kernels on exp's bucket with every buffer `off` elements into its allocation."""
    import torch
    from ina_amd import ops
    x, kb, V = exp.x, exp.kb, exp.V
    n = x.shape[1]
    nblk = (n + V - 1) // V
    kbd = torch.from_numpy(kb).to(DEV)

    def at(a, dtype):
        buf = torch.zeros(n + off, dtype=dtype, device=DEV)
        if a is not None:
            buf[off:] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return buf[off:]

    for r in range(x.shape[0]):
        same(ops.quantize_i16_wire_blk(at(x[r], torch.float32), kbd, V, out=at(None, torch.int32)), exp.wires[r],
             f"wire rank {r} {tag}")
    src = at(exp.wsum, torch.int32)
    g16, gy, gf = ops.i16_wire_finish_blk(src, kbd, V, out16=at(None, torch.int16), y=at(None, torch.float32),
                                          overflow=torch.full((nblk,), 7, dtype=torch.uint8, device=DEV))
    same(g16, exp.o16, f"finish int16 {tag}")
    same(gy, exp.y, f"finish y {tag}")
    same(gf, exp.flags, f"finish flags {tag}")
    only = torch.full((nblk,), 7, dtype=torch.uint8, device=DEV)          # flags alone: every flag written
    r16, ry, rf = ops.i16_wire_finish_blk(src, kbd, V, overflow=only, want_out16=False, want_y=False)
    assert r16 is None and ry is None and rf is only
    same(only, exp.flags, f"flags-only call {tag}")


def main():
    """Child of test_grid_stride_under_the_lab_build: a grid of two workgroups over n = 65,536 + 5."""
    import torch
    from ina_amd import ops
    assert os.environ.get("INA_LIBRARY") == "libina_lab.so"
    ops.set_tuning(max_blocks=2, ew_blocks=2)
    n = 65_536 + 5
    for V in (32, 100):
        x = ranks_bucket(n, V, 900 + V)
        for kb in (given_scales(x, V), ref.kblk_ref(x, V, degree=3, bits=16)):
            exp = Expected(x, kb, V)
            for off in (0, 1):
                run_case(exp, off, f"lab grid of 2, V={V} off={off}")
    torch.cuda.synchronize()
    print("shard blk lab child ok")


if __name__ == "__main__":
    main()
