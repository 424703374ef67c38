"""Shared pieces of tests/test_gpu_geometry.py, and -- run as a program -- its child process:
the same checks against a lab build of the library (csrc/Makefile `lab`, -DINA_LAB_KEYS=1) under
the grid caps that only a lab build lets a caller set (tuning keys 4, 5, 6 and 14).

Almost every kernel in csrc/ is a grid-stride loop under a grid cap sized for the benchmark's
buckets.  A case here is made for a cap c: with c workgroups of 256 threads one pass covers
c * 256 work items, and n is taken from that (n_for) so that the loop body runs at least four
times and the last pass ends inside workgroup 0: wave 0 has whole work, wave 1 a ragged tail,
waves 2 and 3 none.  Every output is a caller's buffer filled with 0x5A bytes (flags 0xFF) and
PAD elements longer than the result: what a skipped region leaves behind cannot equal the
oracle's bytes by luck of the allocator, and a store past the end shows.

A case is a function make(cap) -> run; make builds the inputs and the CPU oracle's results once,
run(o) launches and returns [(label, device tensor, expected ndarray, fill byte)].  Usage:
    INA_LIBRARY=libina_lab.so python tests/_geometry_lab.py OUT.jsonl
writes one JSON record per (case, key, cap): {"name", "ok", "first"}; it stops at the first
error the library or the HIP runtime reports instead of going on using the device.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
for _p in (REPO, os.path.join(REPO, "distributed-training-ina_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import oracle as orc                                    # noqa: E402
from tests import _blk_ref as ref                                   # noqa: E402

DEV = "cuda:0"
PAD = 5                      # elements (rows for 2-D outputs) past the result
FILL, FLAG_FILL = 0x5A, 0xFF
X16 = {"bf16": torch.bfloat16, "f16": torch.float16}
WSTEP = 0.125 * 0.3
BLOCK = 256                  # threads per workgroup in every kernel of csrc/


def ops():
    from ina_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent(shape, dtype, byte=FILL):
    """A device tensor of `shape` plus PAD (on the first axis), every byte `byte`."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    t = torch.empty((shape[0] + PAD,) + shape[1:], dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(byte)
    return t


def n_for(cap, per_item=1, U=1):
    """Values for a kernel whose work item covers `per_item` values under a grid cap of `cap`
    workgroups, U items in flight per thread.  U = 1: three full passes.  U > 1 (chunk_loop): two
    U-way passes and one full pass of the one-item remainder loop.  Then a last pass of 69 items
    (wave 0 whole, wave 1 five items and a ragged one, waves 2 and 3 none) and, for vector
    kernels, one value more, so that n % per_item != 0 and the scalar tail runs."""
    S = cap * BLOCK
    items = (3 * S if U == 1 else 2 * U * S + S) + 69
    return items * per_item + (1 if per_item > 1 else 0)


def passes(cap, items):
    """How often the busiest thread's loop body runs over `items` work items."""
    return -(-items // (cap * BLOCK))


def npk_for(cap, C=1):
    """Packets for the flat packet kernels (C 16-byte chunks per packet; C = 1: a thread per
    packet): the per-packet loop makes three full passes and a ragged one, and the chunk
    loop's last pass starts inside a packet and ends in wave 1 of workgroup 0."""
    S = cap * BLOCK
    npk = 3 * S + 69
    while C > 1 and not ((npk * C // S * S) % C and 64 < npk * C % S < 128):
        npk += 1
    assert 3 * S < npk < 4 * S
    return npk


def grads(rng, n, W=None):
    """N(0, 1e-2) with 1 % outliers x100, fp32: [n] or [W, n]."""
    shape = (n,) if W is None else (W, n)
    x = rng.standard_normal(shape) * 1e-2
    x[rng.random(shape) < 0.01] *= 100.0
    return x.astype(np.float32)


def plant_positions(rng, n, V, pass_vals):
    """The first and last value of the first and last slot of every pass, and one value in
    about 1 % of the slots."""
    pos = []
    for start in range(0, n, pass_vals):
        end = min(start + pass_vals, n)
        for slot in (start // V, (end - 1) // V):
            pos += [slot * V, min(slot * V + V, n) - 1]
    nslot = -(-n // V)
    for s in rng.choice(nslot, max(1, nslot // 100), replace=False):
        pos.append(int(s) * V + int(rng.integers(min(V, n - int(s) * V))))
    return np.unique(np.array(pos, np.int64))


def mixed(flags):
    """The oracle's flags are neither all set nor all clear."""
    assert 0 < int(flags.sum()) < flags.size, (int(flags.sum()), flags.size)


def to16(x, dtype):
    """fp32 array -> (16-bit host tensor, its exact fp32 widening)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return t, t.float().numpy()


def round16(f32, dtype):
    """What the dequantiser gives in a 16-bit type: the fp32 result rounded once, as bits."""
    return torch.from_numpy(f32).to(dtype).view(torch.int16).numpy()


def judge(label, got, want, byte=FILL):
    """Bit for bit over the result, `byte` in every byte past it: (label, ok, first bad element)."""
    torch.cuda.synchronize()
    g = got.detach().contiguous().view(torch.uint8).cpu().numpy().reshape(-1)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert g.size > w.size, label
    bad = np.flatnonzero(g[:w.size] != w)
    if bad.size == 0:
        bad = w.size + np.flatnonzero(g[w.size:] != byte)
    first = int(bad[0]) // max(1, np.ascontiguousarray(want).itemsize) if bad.size else None
    return label, bad.size == 0, first


def run_case(o, make, cap, setter=None):
    """make(cap) built, then run under setter(cap) (restored by setter(None)); the judgements."""
    run = make(cap)
    return judged(o, run, cap, setter)


def judged(o, run, cap, setter):
    if setter is not None:
        setter(cap)
    try:
        res = run(o)
        torch.cuda.synchronize()
    finally:
        if setter is not None:
            setter(None)
    return [judge(*r) for r in res]


# ---- raw calls for the entry points whose wrapper allocates the outputs itself --------------
FIELDS = (("bitmap", torch.int32), ("count", torch.uint8), ("flags", torch.uint8), ("index", torch.int32),
          ("switch_id", torch.uint8), ("frag_id", torch.int32))


def unpack_raw(o, pkts, npk, V, stride, with_values=True, pay=None):
    """ina_unpack_nga (ina_unpack_nga_split with `pay`) into sentinel-filled outputs."""
    from ina_amd import _lib
    f = {k: sent(npk, dt) for k, dt in FIELDS}
    fs = _lib.NgaFields(*[f[k].data_ptr() for k, _ in FIELDS])
    vals = sent(npk * V, torch.int32) if with_values else None
    vp = vals.data_ptr() if with_values else None
    st = torch.cuda.current_stream().cuda_stream
    if pay is None:
        _lib.check(o.load().ina_unpack_nga(pkts.data_ptr(), npk, V, stride, C.byref(fs), vp, st), "unpack_nga")
    else:
        _lib.check(o.load().ina_unpack_nga_split(pkts.data_ptr(), pay.data_ptr(), npk, V, C.byref(fs), vp, st),
                   "unpack_nga_split")
    return f, vals


def unpack_results(tag, f, vals, want_f, want_vals):
    res = [(f"{tag} {k}", f[k], want_f[k]) for k, _ in FIELDS]
    if vals is not None:
        res.append((f"{tag} values", vals, want_vals))
    return res


def to_split(packed, V):
    hdr = np.zeros((len(packed), 16), np.uint8)
    hdr[:, :15] = packed[:, :15]
    return hdr, np.ascontiguousarray(packed[:, 15:15 + 4 * V])


def desc_of(packed):
    """int64 descriptors = header bytes 4..11 of each packet."""
    return np.ascontiguousarray(packed[:, 4:12]).view(np.int64).reshape(-1)


HDR = dict(bitmap=5, count=8, switch_id=1, seq0=4_000_000_000, num_slots=1000)


def orc_pack(vals, V, stride, ovf=None, bitmap=HDR["bitmap"], flags=0):
    return orc.pack_nga(vals, V, bitmap, HDR["count"], HDR["switch_id"], HDR["seq0"], flags=flags,
                        num_slots=HDR["num_slots"], stride=stride, ovf=ovf)


# =============================================================================================
# cases under tuning key 0 (product library): make(cap) -> run
# =============================================================================================
def sum_reduce_case(kind):
    """unaligned: views 4 bytes off (k_sum_reduce_i32_scalar, an item a value); dyn: W = 5, not
    one of the specialised 1, 2, 3, 4, 8, 16 (k_sum_reduce_i32_vec_dyn, an item 4 values)."""
    def make(cap):
        rng = np.random.default_rng(11)
        W, n, off = (3, n_for(cap, 1), 1) if kind == "unaligned" else (5, n_for(cap, 4), 0)
        bufs = [rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32) for _ in range(W)]
        want = orc.sum_reduce_i32(bufs)
        d = [dev(np.concatenate([np.zeros(off, np.int32), b]))[off:] for b in bufs]
        assert all(t.data_ptr() % 16 == 4 * off for t in d)

        def run(o):
            out = sent(n, torch.int32)
            o.sum_reduce(d, out=out)
            return [(f"sum_reduce {kind} n={n}", out, want)]
        return run
    return make


I16_W = {8: 4, 256: 3, 512: 8, 100: 5}       # fused reduce: specialised and runtime worker counts


def i16_case(entry, V, src):
    """quantize_i16 / sum_reduce_i16 / quantize_reduce_i16 at slot size V; src: f32, bf16, f16.
    V % 8 == 0 up to 512 takes the ballot layout (an item 8 values), V = 100 the scalar kernel."""
    def make(cap):
        rng = np.random.default_rng(1000 + V)
        per = 8 if V != 100 else 1
        n, k = n_for(cap, per), 14
        pos = plant_positions(rng, n, V, cap * BLOCK * per)
        W = 1 if entry == "quantize_i16" else I16_W[V]
        if entry == "sum_reduce_i16":
            x = rng.integers(-3000, 3000, (W, n)).astype(np.int16)
            x[0, pos] = x[1, pos] = np.where(np.arange(pos.size) % 2, 30000, -30000)
            want, wf = orc.sum_reduce_i16_sat(list(x), V)
            d = [dev(r) for r in x]
        else:
            x = grads(rng, n, W)
            x[0, pos] = np.where(np.arange(pos.size) % 2, np.float32(1e3), np.float32(np.nan))
            if src == "f32":
                d, w32 = [dev(r) for r in x], list(x)
            else:
                pairs = [to16(r, X16[src]) for r in x]
                d, w32 = [p[0].to(DEV) for p in pairs], [p[1] for p in pairs]
            want, wf = (orc.quantize_i16_sat(w32[0], k, V) if W == 1 and entry == "quantize_i16"
                        else orc.quantize_reduce_i16_sat(w32, k, V))
        mixed(wf)

        def run(o):
            out, fl = sent(n, torch.int16), sent(wf.size, torch.uint8, FLAG_FILL)
            if entry == "quantize_i16":
                o.quantize_i16(d[0], k, V, out=out, overflow=fl)
            elif entry == "sum_reduce_i16":
                o.sum_reduce_i16(d, V, out=out, overflow=fl)
            else:
                o.quantize_reduce_i16(d, k, V, out=out, overflow=fl)
            tag = f"{entry} {src} V={V} W={W} n={n}"
            return [(tag, out, want), (tag + " flags", fl, wf, FLAG_FILL)]
        return run
    return make


def tight_packets_case():
    """The tight layout (stride 15 + 4V: k_pack_nga_bytes, an item a byte) with descriptors
    (k_nga_desc, an item a packet); nga_descriptors, make_descriptors (k_nga_make_desc), and
    unpack_nga's scalar path over the same rows (an item a value or a header)."""
    def make(cap):
        rng = np.random.default_rng(12)
        V = 8
        stride, npk = 15 + 4 * V, npk_for(cap)
        n = npk * V - 3
        vals = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
        ovf = (rng.random(npk) < 0.3).astype(np.uint8)
        want = orc_pack(vals, V, stride, ovf=ovf)
        want_plain = orc_pack(np.zeros(n, np.int32), V, stride)
        wf, wv = orc.unpack_nga(want, V, stride)
        dv, dovf, dpk = dev(vals), dev(ovf), dev(want)

        def run(o):
            out, desc = sent((npk, stride), torch.uint8), sent(npk, torch.int64)
            o.pack_nga(dv, V, HDR["bitmap"], HDR["count"], HDR["switch_id"], HDR["seq0"], num_slots=HDR["num_slots"],
                       stride=stride, overflow=dovf, out=out, desc=desc)
            d2 = sent(npk, torch.int64)
            o.nga_descriptors(dpk, out=d2)
            d3 = [sent(npk, torch.int64) for _ in range(2)]
            o.make_descriptors(npk, 2, HDR["count"], HDR["switch_id"], [HDR["seq0"], 7], num_slots=HDR["num_slots"],
                               outs=d3)
            want7 = desc_of(orc.pack_nga(np.zeros(n, np.int32), V, 0, HDR["count"], HDR["switch_id"], 7,
                                         num_slots=HDR["num_slots"], stride=stride))
            f, v = unpack_raw(o, dpk, npk, V, stride)
            return ([(f"pack_nga tight npk={npk}", out, want), ("pack_nga tight desc", desc, desc_of(want)),
                     ("nga_descriptors", d2, desc_of(want)), ("make_descriptors 0", d3[0], desc_of(want_plain)),
                     ("make_descriptors 1", d3[1], want7)] + unpack_results("unpack_nga scalar", f, v, wf, wv))
        return run
    return make


def unpack_hdr_case():
    """unpack_nga without values over 16-byte-multiple rows: k_unpack_nga_hdr, an item a packet."""
    def make(cap):
        rng = np.random.default_rng(13)
        V, npk = 32, npk_for(cap)
        stride = 144
        vals = rng.integers(-2**31, 2**31, npk * V - 5, dtype=np.int64).astype(np.int32)
        pk = np.zeros((npk, stride), np.uint8)
        pk[:, :15 + 4 * V] = orc_pack(vals, V, 15 + 4 * V, ovf=(rng.random(npk) < 0.3).astype(np.uint8))
        wf, _ = orc.unpack_nga(pk, V, stride)
        dpk = dev(pk)

        def run(o):
            f, _ = unpack_raw(o, dpk, npk, V, stride, with_values=False)
            return unpack_results(f"unpack_nga headers npk={npk}", f, None, wf, None)
        return run
    return make


def pack_c128_case():
    """pack_c128 into rows 4 bytes off 16-byte alignment: k_pack_c128, an item a 32-bit word."""
    def make(cap):
        rng = np.random.default_rng(14)
        S, pn = cap * BLOCK, 1
        while not (131 * pn > 3 * S and 64 < 131 * pn % S < 128):
            pn += 1
        g = rng.integers(-2**31, 2**31, pn * 128, dtype=np.int64).astype(np.int32)
        want = orc.pack_c128(g, pn, 3, 0x01020304, 9)
        dg = dev(g)

        def run(o):
            buf = sent(pn * 524 + 4, torch.uint8)
            out = buf[4:]
            assert out.data_ptr() % 16 == 4
            o.pack_c128(dg, pn, 3, 0x01020304, 9, out=out)
            return [(f"pack_c128 packets={pn} words={131 * pn}", out, want),
                    ("pack_c128 bytes before the rows", buf[:4], np.zeros(0, np.uint8))]
        return run
    return make


def blk_case(V, W, n_of, parts="all"):
    """The per-block-scale entry points (include/ina_blk.h) at block size V on W buckets, GIVEN
    and AUTO, against the per-block oracle (tests/_blk_ref.py).  parts: "all", or "reduce" for the
    two fused int32 reduces alone.  Every third block's given scale is 6 too large for int16 and
    NaNs are planted at the block edges of every pass, so the int16 flags are mixed."""
    def make(cap):
        rng = np.random.default_rng(2000 + 7 * V + W)
        n = n_of(cap)
        nblk = -(-n // V)
        x = ref.bucket(rng, W, n, V, lo=-6, hi=2)
        vec = V in (8, 256)
        pos = plant_positions(rng, n, V, (cap * BLOCK * 4) if vec else cap * 4 * V)
        x[0, pos[::2]] = np.nan
        kb = ref.kblk_ref(x, V, W, 16)
        hot = np.arange(nblk) % 3 == 1
        kb[hot] = np.minimum(kb[hot].astype(int) + 6, 127).astype(np.int8)
        kb32, kb16 = ref.kblk_ref(x, V, W, 32), ref.kblk_ref(x, V, W, 16)
        base = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        local = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        w = {"s32": ref.quantize_reduce_i32(x, kb, V), "a32": ref.quantize_reduce_i32(x, kb32, V)}
        if parts == "all":
            w["q"] = ref.quantize_i32(x[0], kb, V)
            w["q16"], w["qf"] = ref.quantize_i16(x[0], kb, V)
            w["s16"], w["sf"] = ref.quantize_reduce_i16(x, kb, V)
            w["a16"], w["af"] = ref.quantize_reduce_i16(x, kb16, V)
            mixed(w["qf"]), mixed(w["sf"]), mixed(w["af"])
            w["dq32"], w["dq16"] = ref.dequantize(w["s32"], kb, V), ref.dequantize(w["s16"], kb, V)
            w["apply"] = ref.ps_apply(local, w["s32"], kb, V, WSTEP)
            w["kbase"] = ref.kblk_ref(x, V, W, 32, base=base)
            w["kloc"] = ref.kblk_ref(x, V, W, 32, base=local)
            w["comb"] = ref.ps_combine_ina(local, x, w["kloc"], V, WSTEP)
        xs, kbd = [dev(r) for r in x], dev(kb)
        dbase, dlocal = dev(base), dev(local)
        ds32 = dev(w["s32"])
        ds16 = dev(w["s16"]) if parts == "all" else None

        def run(o):
            t = f"V={V} W={W} n={n}"
            r = []
            out = sent(n, torch.int32)
            o.quantize_reduce_blk(xs, V, kblk=kbd, out=out)
            r.append((f"quantize_reduce_blk GIVEN {t}", out, w["s32"]))
            out, ko = sent(n, torch.int32), sent(nblk, torch.int8)
            o.quantize_reduce_blk(xs, V, out=out, kblk_out=ko)
            r += [(f"quantize_reduce_blk AUTO {t}", out, w["a32"]), (f"quantize_reduce_blk AUTO scales {t}", ko, kb32)]
            if parts != "all":
                return r
            out = sent(n, torch.int32)
            o.quantize_blk(xs[0], kbd, V, out=out)
            r.append((f"quantize_blk {t}", out, w["q"]))
            out, fl = sent(n, torch.int16), sent(nblk, torch.uint8, FLAG_FILL)
            o.quantize_i16_blk(xs[0], kbd, V, out=out, overflow=fl)
            r += [(f"quantize_i16_blk {t}", out, w["q16"]), (f"quantize_i16_blk flags {t}", fl, w["qf"], FLAG_FILL)]
            out, fl = sent(n, torch.int16), sent(nblk, torch.uint8, FLAG_FILL)
            o.quantize_reduce_i16_blk(xs, V, kblk=kbd, out=out, overflow=fl)
            r += [(f"quantize_reduce_i16_blk GIVEN {t}", out, w["s16"]),
                  (f"quantize_reduce_i16_blk GIVEN flags {t}", fl, w["sf"], FLAG_FILL)]
            out, fl, ko = sent(n, torch.int16), sent(nblk, torch.uint8, FLAG_FILL), sent(nblk, torch.int8)
            o.quantize_reduce_i16_blk(xs, V, out=out, overflow=fl, kblk_out=ko)
            r += [(f"quantize_reduce_i16_blk AUTO {t}", out, w["a16"]),
                  (f"quantize_reduce_i16_blk AUTO flags {t}", fl, w["af"], FLAG_FILL),
                  (f"quantize_reduce_i16_blk AUTO scales {t}", ko, kb16)]
            for name, src, want in (("i32", ds32, w["dq32"]), ("i16", ds16, w["dq16"])):
                out = sent(n, torch.float32)
                o.dequantize_blk(src, kbd, V, out=out)
                r.append((f"dequantize_blk {name} {t}", out, want))
            out = sent(n, torch.float32)
            o.ps_apply_blk(dlocal, ds32, kbd, V, WSTEP, out=out)
            r.append((f"ps_apply_blk {t}", out, w["apply"]))
            for name, b, want in (("", None, kb32), (" base", dbase, w["kbase"])):
                ko = sent(nblk, torch.int8)
                o.block_scales(xs, V, bits=32, base=b, out=ko)
                r.append((f"block_scales{name} {t}", ko, want))
            out, ko = sent(n, torch.float32), sent(nblk, torch.int8)
            o.ps_combine_ina_blk(dlocal, xs, V, WSTEP, out=out, kblk_out=ko)
            r += [(f"ps_combine_ina_blk {t}", out, w["comb"]), (f"ps_combine_ina_blk scales {t}", ko, w["kloc"])]
            return r
        return run
    return make


def blk_scalar_n(V):
    """k_blk_scalar: a wave per block of V values, 4 blocks per workgroup.  Three full passes, then
    wave 0 a whole block, wave 1 the short last block, waves 2 and 3 none."""
    return lambda cap: (3 * cap * 4 + 2) * V - V // 3


def blk_i16_case(V):
    """quantize_reduce_i16_blk's vector kernel (k_qr_blk_i16: a wave per 512 values), GIVEN and AUTO."""
    def make(cap):
        rng = np.random.default_rng(3000 + V)
        n, W = n_for(cap, 8), 4 if V == 8 else 5
        nblk = -(-n // V)
        x = ref.bucket(rng, W, n, V, lo=-6, hi=2)
        pos = plant_positions(rng, n, V, cap * BLOCK * 8)
        x[0, pos[::2]] = np.nan
        kb = ref.kblk_ref(x, V, W, 16)
        hot = np.arange(nblk) % 3 == 1
        kb[hot] = np.minimum(kb[hot].astype(int) + 6, 127).astype(np.int8)
        kb16 = ref.kblk_ref(x, V, W, 16)
        s16, sf = ref.quantize_reduce_i16(x, kb, V)
        a16, af = ref.quantize_reduce_i16(x, kb16, V)
        mixed(sf), mixed(af)
        xs, kbd = [dev(r) for r in x], dev(kb)

        def run(o):
            t = f"V={V} W={W} n={n}"
            out, fl = sent(n, torch.int16), sent(nblk, torch.uint8, FLAG_FILL)
            o.quantize_reduce_i16_blk(xs, V, kblk=kbd, out=out, overflow=fl)
            r = [(f"quantize_reduce_i16_blk GIVEN {t}", out, s16), (f"GIVEN flags {t}", fl, sf, FLAG_FILL)]
            out, fl, ko = sent(n, torch.int16), sent(nblk, torch.uint8, FLAG_FILL), sent(nblk, torch.int8)
            o.quantize_reduce_i16_blk(xs, V, out=out, overflow=fl, kblk_out=ko)
            return r + [(f"quantize_reduce_i16_blk AUTO {t}", out, a16), (f"AUTO flags {t}", fl, af, FLAG_FILL),
                        (f"AUTO scales {t}", ko, kb16)]
        return run
    return make


KEY0_CASES = {
    "sum_reduce-unaligned": sum_reduce_case("unaligned"),
    "sum_reduce-vec_dyn": sum_reduce_case("dyn"),
    "packets-tight": tight_packets_case(),
    "unpack_nga-headers": unpack_hdr_case(),
    "pack_c128-scalar": pack_c128_case(),
    "blk-scalar-V12": blk_case(12, 3, blk_scalar_n(12)),
    "blk-scalar-V1000": blk_case(1000, 2, blk_scalar_n(1000)),
    "quantize_reduce_i16_blk-V8": blk_i16_case(8),
    "quantize_reduce_i16_blk-V256": blk_i16_case(256),
}
for _V in (8, 256, 512, 100):
    for _src in ("f32", "bf16", "f16"):
        KEY0_CASES[f"quantize_i16-{_src}-V{_V}"] = i16_case("quantize_i16", _V, _src)
        KEY0_CASES[f"quantize_reduce_i16-{_src}-V{_V}"] = i16_case("quantize_reduce_i16", _V, _src)
    KEY0_CASES[f"sum_reduce_i16-V{_V}"] = i16_case("sum_reduce_i16", _V, "i16")


# =============================================================================================
# cases under the lab keys 4 (stream), 5 (fp32 combine), 6 (INA combines), 14 (elementwise)
# =============================================================================================
def _src(x, src):
    """fp32 rows -> (device tensors in `src`, the fp32 arrays the oracle takes)."""
    if src == "f32":
        return [dev(r) for r in x], [np.ascontiguousarray(r) for r in x]
    pairs = [to16(r, X16[src]) for r in x]
    return [p[0].to(DEV) for p in pairs], [p[1] for p in pairs]


def quantize_case(src):
    def make(cap):
        n, k = n_for(cap, 4), 16
        d, w = _src(grads(np.random.default_rng(21), n, 1), src)
        want = orc.quantize_i32(w[0], k)

        def run(o):
            out = sent(n, torch.int32)
            o.quantize(d[0], k, out=out)
            return [(f"quantize {src} n={n}", out, want)]
        return run
    return make


def dequantize_case(sdt, ydt):
    """sdt: i32 / i16; ydt: f32 / bf16 / f16 (int16 to a 16-bit type: an item 8 values)."""
    def make(cap):
        rng = np.random.default_rng(22)
        n, k = n_for(cap, 8 if (sdt == "i16" and ydt != "f32") else 4), 12
        s = (rng.integers(-2**31, 2**31, n, dtype=np.int64) >> rng.integers(0, 31, n)).astype(np.int32)
        s = s.astype(np.int16) if sdt == "i16" else s
        f32 = orc.dequantize_i16(s, k) if sdt == "i16" else orc.dequantize_i32(s, k)
        want = f32 if ydt == "f32" else round16(f32, X16[ydt])
        ds = dev(s)

        def run(o):
            out = sent(n, torch.float32 if ydt == "f32" else X16[ydt])
            o.dequantize(ds, k, out=out)
            return [(f"dequantize {sdt}->{ydt} n={n}", out, want)]
        return run
    return make


def ps_apply_case():
    def make(cap):
        rng = np.random.default_rng(23)
        n, k = n_for(cap, 4), 16
        local = grads(rng, n)
        s = rng.integers(-2**20, 2**20, n).astype(np.int32)
        want = (local + orc.dequantize_i32(s, k) * np.float32(WSTEP)).astype(np.float32)
        dl, ds = dev(local), dev(s)

        def run(o):
            out = sent(n, torch.float32)
            o.ps_apply(dl, ds, k, WSTEP, out=out)
            return [(f"ps_apply n={n}", out, want)]
        return run
    return make


def quantize_reduce_case(W, src):
    """W <= 8: one chunk in flight under the elementwise cap; W > 8: two under the stream cap."""
    def make(cap):
        n, k = n_for(cap, 4, 1 if W <= 8 else 2), 16
        d, w = _src(grads(np.random.default_rng(24 + W), n, W), src)
        want = orc.quantize_reduce_i32(w, k)

        def run(o):
            out = sent(n, torch.int32)
            o.quantize_reduce(d, k, out=out)
            return [(f"quantize_reduce {src} W={W} n={n}", out, want)]
        return run
    return make


def combine_case(kind, W, S=None):
    """ps_combine (W <= 4: one chunk in flight, else two) and the INA combine.  S: a fixed cap
    (the product library's 256) instead of the case's."""
    def make(cap):
        rng = np.random.default_rng(25 + W)
        n = n_for(S or cap, 4, 1 if W <= 4 else 2)
        local, paras = grads(rng, n), grads(rng, n, W)
        want = (orc.ps_combine_f32(local, list(paras), WSTEP) if kind == "ps_combine"
                else orc.ps_combine_ina_f32(local, list(paras), 16, WSTEP))
        dl, dp = dev(local), [dev(p) for p in paras]

        def run(o):
            out = sent(n, torch.float32)
            if kind == "ps_combine":
                o.ps_combine(dl, dp, WSTEP, out=out)
            else:
                from ina_amd import ps
                ps.combine_ina(dl, dp, 16, WSTEP, out=out)
            return [(f"{kind} W={W} n={n}", out, want)]
        return run
    return make


def wire_case():
    def make(cap):
        rng = np.random.default_rng(26)
        n, k, V = n_for(cap, 4), 14, 32
        x = grads(rng, n)
        pos = plant_positions(rng, n, V, cap * BLOCK * 4)
        x[pos] = np.where(np.arange(pos.size) % 2, np.float32(1e3), np.float32(np.nan))
        wire = orc.quantize_i16_wire(x, k)
        wsum = (wire + orc.quantize_i16_wire(grads(rng, n), k)).astype(np.int32)
        w16, wy, wf = orc.i16_wire_finish(wsum, k, V)
        mixed(wf)
        dx, dsum = dev(x), dev(wsum)

        def run(o):
            out = sent(n, torch.int32)
            o.quantize_i16_wire(dx, k, out=out)
            o16, y, fl = sent(n, torch.int16), sent(n, torch.float32), sent(wf.size, torch.uint8, FLAG_FILL)
            o.i16_wire_finish(dsum, k, V, out16=o16, y=y, overflow=fl)
            return [(f"quantize_i16_wire n={n}", out, wire), ("i16_wire_finish int16", o16, w16),
                    ("i16_wire_finish fp32", y, wy), ("i16_wire_finish flags", fl, wf, FLAG_FILL)]
        return run
    return make


def _flat_want(vals, V, stride, **kw):
    """The oracle's wire bytes in rows of `stride`, the padding zero as the flat kernels write it."""
    tight = orc_pack(vals, V, 15 + 4 * V, **kw)
    out = np.zeros((len(tight), stride), np.uint8)
    out[:, :15 + 4 * V] = tight
    return out


def pack_flat_case(V):
    """pack_nga in padded rows (k_pack_nga_flat) with overflow flags and descriptors, and
    unpack_nga's flat kernel back over the same rows."""
    def make(cap):
        o = ops()
        rng = np.random.default_rng(27 + V)
        stride = o.nga_stride(V)
        npk = npk_for(cap, stride // 16)
        n = npk * V - V // 3
        vals = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
        ovf = (rng.random(npk) < 0.3).astype(np.uint8)
        want = _flat_want(vals, V, stride, ovf=ovf)
        wf, wv = orc.unpack_nga(want, V, stride)
        dv, dovf, dpk = dev(vals), dev(ovf), dev(want)

        def run(o):
            out, desc = sent((npk, stride), torch.uint8), sent(npk, torch.int64)
            o.pack_nga(dv, V, HDR["bitmap"], HDR["count"], HDR["switch_id"], HDR["seq0"], num_slots=HDR["num_slots"],
                       overflow=dovf, out=out, desc=desc)
            r = [(f"pack_nga V={V} npk={npk}", out, want), (f"pack_nga V={V} desc", desc, desc_of(want))]
            if V % 4 == 0:
                f, v = unpack_raw(o, dpk, npk, V, stride)
                r += unpack_results(f"unpack_nga V={V}", f, v, wf, wv)
            return r
        return run
    return make


def quantize_pack_case(V, src):
    """quantize_pack_nga with a base and descriptors (V = 256 takes a covering grid: not here)."""
    def make(cap):
        o = ops()
        rng = np.random.default_rng(28 + V)
        stride, k = o.nga_stride(V), 16
        npk = npk_for(cap, stride // 16)
        n = npk * V - V // 3
        d, w = _src(grads(rng, n, 1), src)
        base = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        want = _flat_want(orc.quantize_i32((w[0] - base).astype(np.float32), k), V, stride)
        db = dev(base)

        def run(o):
            out, desc = sent((npk, stride), torch.uint8), sent(npk, torch.int64)
            o.quantize_pack_nga(d[0], k, V, HDR["bitmap"], HDR["count"], HDR["switch_id"], HDR["seq0"], base=db,
                                num_slots=HDR["num_slots"], out=out, desc=desc)
            return [(f"quantize_pack_nga {src} V={V} npk={npk}", out, want),
                    (f"quantize_pack_nga {src} V={V} desc", desc, desc_of(want))]
        return run
    return make


def multi_case(W, split, src="f32"):
    """quantize_pack_nga_multi (packed rows) / _multi_split (split rows): W workers, a base and
    descriptors; the split form also packs int32 values and unpacks the rows again."""
    def make(cap):
        o = ops()
        rng = np.random.default_rng(29 + W)
        V, k = 32, 16
        stride = o.nga_stride(V)
        npk = npk_for(cap, 1 if split else stride // 16)
        n = npk * V - V // 3
        d, w = _src(grads(rng, n, W), src)
        base = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        q = [orc.quantize_i32((a - base).astype(np.float32), k) for a in w]
        want = [_flat_want(q[i], V, stride, bitmap=i + 1) for i in range(W)]
        db, bm = dev(base), list(range(1, W + 1))
        ovf = (rng.random(npk) < 0.3).astype(np.uint8)
        want0 = _flat_want(q[0], V, stride, ovf=ovf)
        wf, wv = orc.unpack_nga(want0, V, stride)
        dq0, dovf = dev(q[0]), dev(ovf)
        h0, p0 = (dev(a) for a in to_split(want0, V))

        def run(o):
            t = f"{src} W={W} npk={npk}"
            descs = [sent(npk, torch.int64) for _ in range(W)]
            r = []
            if not split:
                outs = [sent((npk, stride), torch.uint8) for _ in range(W)]
                o.quantize_pack_nga_multi(d, k, V, bm, HDR["count"], HDR["switch_id"], HDR["seq0"], base=db,
                                          num_slots=HDR["num_slots"], outs=outs, descs=descs)
                for i in range(W):
                    r += [(f"quantize_pack_nga_multi {t} worker {i}", outs[i], want[i]),
                          (f"quantize_pack_nga_multi {t} desc {i}", descs[i], desc_of(want[i]))]
                return r
            hdrs, pays = [sent((npk, 16), torch.uint8) for _ in range(W)], [sent((npk, 4 * V), torch.uint8) for _ in range(W)]
            o.quantize_pack_nga_multi_split(d, k, V, bm, HDR["count"], HDR["switch_id"], HDR["seq0"], base=db,
                                            num_slots=HDR["num_slots"], hdrs=hdrs, pays=pays, descs=descs)
            for i in range(W):
                wh, wp = to_split(want[i], V)
                r += [(f"multi_split {t} hdr {i}", hdrs[i], wh), (f"multi_split {t} pay {i}", pays[i], wp),
                      (f"multi_split {t} desc {i}", descs[i], desc_of(want[i]))]
            if src == "f32":
                hdr, pay, desc = sent((npk, 16), torch.uint8), sent((npk, 4 * V), torch.uint8), sent(npk, torch.int64)
                o.pack_nga_split(dq0, V, HDR["bitmap"], HDR["count"], HDR["switch_id"], HDR["seq0"],
                                 num_slots=HDR["num_slots"], overflow=dovf, hdr=hdr, pay=pay, desc=desc)
                wh, wp = to_split(want0, V)
                r += [(f"pack_nga_split hdr npk={npk}", hdr, wh), ("pack_nga_split pay", pay, wp),
                      ("pack_nga_split desc", desc, desc_of(want0))]
                f, v = unpack_raw(o, h0, npk, V, 16, pay=p0)
                r += unpack_results("unpack_nga_split", f, v, wf, wv)
            return r
        return run
    return make


LAB_CASES = {
    "ps_apply": ps_apply_case(),
    "ps_combine-W3": combine_case("ps_combine", 3),
    "ps_combine-W6": combine_case("ps_combine", 6),
    "combine_ina-W3": combine_case("combine_ina", 3),
    "combine_ina-W6": combine_case("combine_ina", 6),
    "i16_wire": wire_case(),
    "pack_nga-V32": pack_flat_case(32),
    "pack_nga-V256": pack_flat_case(256),
    "pack_nga-V100": pack_flat_case(100),
    "quantize_pack_nga_multi-W3": multi_case(3, False),
    "quantize_pack_nga_multi-W9": multi_case(9, False),
    "split_rows-f32": multi_case(3, True),
    "blk-vec-V8": blk_case(8, 4, lambda cap: n_for(cap, 4)),
    "blk-vec-V256": blk_case(256, 5, lambda cap: n_for(cap, 4)),
    "blk-reduce-V8-W9": blk_case(8, 9, lambda cap: n_for(cap, 4), "reduce"),
    "blk-reduce-V256-W4": blk_case(256, 4, lambda cap: n_for(cap, 4), "reduce"),
    "blk-reduce-V8-W5": blk_case(8, 5, lambda cap: n_for(cap, 4), "reduce"),
    "blk-reduce-V256-W9": blk_case(256, 9, lambda cap: n_for(cap, 4), "reduce"),
}
for _s in ("f32", "bf16", "f16"):
    LAB_CASES[f"quantize-{_s}"] = quantize_case(_s)
    LAB_CASES[f"dequantize-i32-{_s}"] = dequantize_case("i32", _s)
    LAB_CASES[f"dequantize-i16-{_s}"] = dequantize_case("i16", _s)
    for _W in (3, 8, 9, 17):
        LAB_CASES[f"quantize_reduce-{_s}-W{_W}"] = quantize_reduce_case(_W, _s)
    for _V in (32, 100):
        LAB_CASES[f"quantize_pack_nga-{_s}-V{_V}"] = quantize_pack_case(_V, _s)
for _s in ("bf16", "f16"):
    LAB_CASES[f"split_rows-{_s}"] = multi_case(3, True, _s)

LAB_KEYS = {4: ("stream_blocks", 16384), 5: ("combine_blocks", 256), 6: ("combine_ina_blocks", 8192),
            14: ("ew_blocks", 1 << 24)}
CAPS = (1, 3)
LAB_IDS = [f"{name}-key{key}-cap{cap}" for name in LAB_CASES for key in LAB_KEYS for cap in CAPS]


def lab_setter(o, key):
    kw, default = LAB_KEYS[key]
    return lambda cap: o.set_tuning(**{kw: default if cap is None else cap})


def main():
    out_path = sys.argv[1]
    assert "lab" in os.environ.get("INA_LIBRARY", ""), "the child runs the lab build (INA_LIBRARY=libina_lab.so)"
    o = ops()
    with open(out_path, "w") as fh:
        for name, make in LAB_CASES.items():
            for cap in CAPS:
                run = make(cap)             # inputs and the oracle's results: once for the four keys
                for key in LAB_KEYS:
                    # any error of the library or the runtime ends the child here: nothing more
                    # is started on the device after it
                    res = judged(o, run, cap, lab_setter(o, key))
                    bad = [r for r in res if not r[1]]
                    rec = {"name": f"{name}-key{key}-cap{cap}", "ok": not bad,
                           "first": bad[0][2] if bad else None, "what": bad[0][0] if bad else None,
                           "checks": len(res)}
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()
    print(f"geometry lab child ok: {len(LAB_IDS)} records")


if __name__ == "__main__":
    main()
