"""The child process of tests/test_gpu_blk_x16.py's lab cases: the block-scaled 16-bit kernels whose grid
caps only a lab build of the library lets a caller set (csrc/Makefile `lab`: tuning keys 4 and 14) -- the
scales, the int32 reduce and the decode -- at a grid of two workgroups, so that with n = 5123 every
grid-stride loop runs three times and ends on a ragged chunk.  Expectations are the per-block CPU oracle
(tests/_blk_ref.py) on the widened buckets.  Usage:
    INA_LIBRARY=libina_lab.so python tests/_blk_x16_lab.py OUT.jsonl
writes one JSON record per case: {"name", "ok", "checks", "first"}; it stops at the first error the
library or the HIP runtime reports instead of going on using the device."""
import json
import os
import sys

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
for _p in (REPO, os.path.join(REPO, "distributed-training-ina_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DTYPES = ("bf16", "f16")
CASES = ("scales", "reduce_i32", "decode")
IDS = [f"{c}-{d}" for c in CASES for d in DTYPES]
N, V, GRID = 5123, 32, 2


def run(case, dtype):
    """[(label, device tensor or ndarray, expected ndarray)]"""
    import numpy as np
    import torch
    from ina_amd import blk
    from tests import _blk_ref as ref

    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    rng = np.random.default_rng(len(case) + len(dtype))
    t = torch.from_numpy(ref.bucket(rng, 17, N, V, lo=-7.0, hi=3.0)).to(dt)
    xs, w = [r.to("cuda:0") for r in t], t.float().numpy()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")          # noqa: E731
    out = []
    if case == "scales":
        base = (rng.standard_normal(N) * 1e-3).astype(np.float32)
        for W in (1, 4, 5):
            out.append((f"W={W}", blk.block_scales(xs[:W], V, bits=16), ref.kblk_ref(w[:W], V, W, 16)))
            out.append((f"W={W} base", blk.block_scales(xs[:W], V, base=dev(base)),
                        ref.kblk_ref(w[:W], V, W, 32, base=base)))
    elif case == "reduce_i32":
        for W in (1, 3, 8, 16, 17):             # ew cap up to 8 workers, the streaming cap beyond
            kb = ref.kblk_ref(w[:W], V, W, 32)
            want = ref.quantize_reduce_i32(w[:W], kb, V)
            got, gk = blk.quantize_reduce(xs[:W], V)
            out += [(f"AUTO W={W}", got, want), (f"AUTO scales W={W}", gk, kb)]
            out.append((f"GIVEN W={W}", blk.quantize_reduce(xs[:W], V, kblk=dev(kb))[0], want))
    else:
        kb = rng.integers(-126, 128, (N + V - 1) // V).astype(np.int8)
        s32 = (rng.integers(-2**31, 2**31, N, dtype=np.int64) >> rng.integers(0, 31, N)).astype(np.int32)
        s16 = rng.integers(-2**15, 2**15, N, dtype=np.int64).astype(np.int16)
        for s in (s32, s16):
            want = torch.from_numpy(ref.dequantize(s, kb, V)).to(dt).view(torch.int16).numpy()
            out.append((str(s.dtype), blk.dequantize(dev(s), dev(kb), V, dtype=dt).view(torch.int16), want))
    return out


def main(path):
    import numpy as np
    import torch
    from ina_amd import ops

    ops.set_tuning(stream_blocks=GRID, ew_blocks=GRID)          # a product build refuses these: RuntimeError
    with open(path, "w") as fh:
        for name in IDS:
            case, dtype = name.split("-")
            first, checks = None, 0
            for label, got, want in run(case, dtype):
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                checks += 1
                if first is None and not (got.shape == want.shape and got.dtype == want.dtype and
                                          np.array_equal(got.view(f"u{got.itemsize}"), want.view(f"u{want.itemsize}"))):
                    first = label
            fh.write(json.dumps({"name": name, "ok": first is None, "checks": checks, "first": first}) + "\n")
            fh.flush()
    print(f"blk x16 lab child ok: {len(IDS)} records")


if __name__ == "__main__":
    main(sys.argv[1])
