"""bench_extra.py -- secondary per-kernel timings for DESIGN.md (not the headline line).

Each row: median device time of one launch (HIP events on the launch stream,
20 launches after 3 warm-ups) and the algorithmic HBM bytes of that launch
(SURVEY.md 8d), so GB/s = bytes / time and frac = GB/s / 8000.  Cold caches: a
512 MiB buffer is READ before every timed launch (outside its events), so working
sets below the 256 MB Infinity Cache do not replay from it ("cache
flush between iterations").  The flush only reads: a written flush buffer would leave
up to 256 MB of dirty lines whose write-back lands inside the next timed launch.
"""
from __future__ import annotations

import statistics

import torch

HBM = 8000.0


_FLUSH = []


def _flush():
    from ina_amd import ops
    if not _FLUSH:
        _FLUSH.append(torch.ones(128 << 20, dtype=torch.int32, device="cuda"))   # 512 MiB
        torch.cuda.synchronize()
    ops.checksum(_FLUSH[0])          # streams 512 MiB in, writes 4 bytes


def _time(fn, reps=20, warm=3, cold=True):
    s = torch.cuda.current_stream()
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        if cold:
            _flush()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        ts.append((a, b))
    torch.cuda.synchronize()
    return statistics.median([a.elapsed_time(b) for a, b in ts]) / 1e3


def _row(name, secs, nbytes, **kw):
    gbs = nbytes / secs / 1e9
    r = {"kernel": name, "us": round(secs * 1e6, 2), "bytes": int(nbytes),
         "GB/s": round(gbs, 1), "frac": round(gbs / HBM, 4)}
    r.update(kw)
    return r


def run_x16(dev, dtype=torch.bfloat16):
    """bf16 gradient buckets (include/ina.h "bf16 / fp16 gradients") at the config-2 and config-4
    shapes.  Each 16-bit call is timed in the same run beside (a) its fp32 sibling on an fp32
    bucket of the same length, twice -- the two times' difference is the run-to-run spread --
    and (b) what a user without the 16-bit entry points does: widen (into a preallocated fp32
    buffer, no allocation in the timed region) then call the sibling.  bytes = algorithmic HBM
    bytes of the 16-bit call; the siblings' rows carry their own."""
    from ina_amd import ops
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    n, k = 25_557_032, 16
    name16 = {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]

    def trio(name, nb16, nb32, f16, f32, widen):
        """rows for one op: sibling, 16-bit, widen + sibling, sibling again"""
        t32a = _time(f32)
        t16 = _time(f16)
        tw = _time(lambda: (widen(), f32()))
        t32b = _time(f32)
        lo, hi = min(t32a, t32b), max(t32a, t32b)
        rows.append(_row(f"{name} [{name16}]", t16, nb16, sibling_us=[round(t32a * 1e6, 2), round(t32b * 1e6, 2)],
                         sibling_frac=round(nb32 / lo / 1e9 / HBM, 4),
                         sibling_spread_us=round((hi - lo) * 1e6, 2), widen_then_sibling_us=round(tw * 1e6, 2),
                         faster_than_widen_then_sibling=bool(t16 < tw),
                         no_slower_than_sibling=bool(t16 <= hi + (hi - lo))))

    # config 2: W = 4 to int32; config 4: W = 16 to int16 (V = 256)
    W2, W4, V = 4, 16, 256
    b32 = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(W4)]
    b16 = [b.to(dtype) for b in b32]
    wid = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(W4)]
    q = torch.empty(n, dtype=torch.int32, device=dev)
    trio("quantize_x16_i32", 6 * n, 8 * n, lambda: ops.quantize(b16[0], k, out=q),
         lambda: ops.quantize(b32[0], k, out=q), lambda: wid[0].copy_(b16[0]))
    trio(f"quantize_reduce_x16_i32 W={W2} (C2)", (2 * W2 + 4) * n, (4 * W2 + 4) * n,
         lambda: ops.quantize_reduce(b16[:W2], k, out=q), lambda: ops.quantize_reduce(b32[:W2], k, out=q),
         lambda: [w.copy_(x) for w, x in zip(wid[:W2], b16[:W2])])
    o16 = torch.empty(n, dtype=torch.int16, device=dev)
    f = torch.empty((n + V - 1) // V, dtype=torch.uint8, device=dev)
    trio(f"quantize_reduce_x16_i16_sat W={W4} V={V} (C4)", (2 * W4 + 2) * n + f.numel(), (4 * W4 + 2) * n + f.numel(),
         lambda: ops.quantize_reduce_i16(b16, 13, V, out=o16, overflow=f),
         lambda: ops.quantize_reduce_i16(b32, 13, V, out=o16, overflow=f),
         lambda: [w.copy_(x) for w, x in zip(wid, b16)])
    # dequantise: the 16-bit call against the fp32 call, and against the fp32 call + a narrowing copy
    ops.quantize_reduce(b32[:W2], k, out=q)
    y32 = torch.empty(n, dtype=torch.float32, device=dev)
    y16 = torch.empty(n, dtype=dtype, device=dev)
    trio("dequantize_i32_x16", 6 * n, 8 * n, lambda: ops.dequantize(q, k, out=y16),
         lambda: ops.dequantize(q, k, out=y32), lambda: y16.copy_(y32))
    # the 8 workers' split packs in one launch, against an fp32 base
    Wp = 8
    base = torch.randn(n, device=dev, generator=gen) * 1e-2
    npk = (n + V - 1) // V
    hdrs = [torch.zeros((npk, 16), dtype=torch.uint8, device=dev) for _ in range(Wp)]
    pays = [torch.empty((npk, 4 * V), dtype=torch.uint8, device=dev) for _ in range(Wp)]
    args = (k, V, list(range(1, Wp + 1)), Wp, 1, 1)
    out_b = Wp * (npk * 16 + npk * 4 * V)
    trio(f"quantize_pack_nga_multi_split_x16 W={Wp} V={V}", (2 * Wp + 4) * n + out_b, (4 * Wp + 4) * n + out_b,
         lambda: ops.quantize_pack_nga_multi_split(b16[:Wp], *args, base=base, hdrs=hdrs, pays=pays),
         lambda: ops.quantize_pack_nga_multi_split(b32[:Wp], *args, base=base, hdrs=hdrs, pays=pays),
         lambda: [w.copy_(x) for w, x in zip(wid[:Wp], b16[:Wp])])
    return rows


def _wall(fn, reps=20, warm=3):
    """Median wall time of fn() from an idle device to an idle device (for paths with a host read)."""
    import time
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        _flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def run_blk(dev):
    """Per-block scales (include/ina_blk.h) at the ResNet-50 size, cold caches, median of 20, the
    whole set twice in this process (run 1 / run 2).  GIVEN calls and ps_apply_blk beside their
    global-k sibling timed twice (the two times' difference is the spread); the bar is sibling time
    x bytes ratio + spread.  AUTO calls and the block-scaled PS combine beside the composition a
    caller would otherwise write (block_scales, then the GIVEN call) -- they must beat it -- and
    beside the global-k sibling (ratio reported).  The PS combine also against today's k="auto"
    path (absmax_multi, the host read, ina_ps_combine_ina_f32), both as wall time."""
    from ina_amd import ops, ps
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    n, k = 25_557_032, 16
    Wmax = 16
    b = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(Wmax)]
    local = torch.randn(n, device=dev, generator=gen) * 1e-2
    q = torch.empty(n, dtype=torch.int32, device=dev)
    o16 = torch.empty(n, dtype=torch.int16, device=dev)
    y = torch.empty(n, dtype=torch.float32, device=dev)

    def given(run, name, V, nb_sib, f_blk, f_sib):
        nblk = (n + V - 1) // V
        ta, tb, tc = _time(f_sib), _time(f_blk), _time(f_sib)
        lo, hi = min(ta, tc), max(ta, tc)
        bar = hi * (nb_sib + nblk) / nb_sib + (hi - lo)
        rows.append(_row(f"{name} V={V} [blk given, run {run}]", tb, nb_sib + nblk,
                         sibling_us=[round(ta * 1e6, 2), round(tc * 1e6, 2)], sibling_spread_us=round((hi - lo) * 1e6, 2),
                         bar_us=round(bar * 1e6, 2), bar_met=bool(tb <= bar)))

    def auto(run, name, V, nb_sib, f_auto, f_scales, f_given, f_sib):
        nblk = (n + V - 1) // V
        ts, ta, tc = _time(f_sib), _time(f_auto), _time(lambda: (f_scales(), f_given()))
        rows.append(_row(f"{name} V={V} [blk auto, run {run}]", ta, nb_sib + nblk,
                         scales_then_given_us=round(tc * 1e6, 2), beats_scales_then_given=bool(ta < tc),
                         sibling_us=round(ts * 1e6, 2), ratio_to_sibling=round(ta / ts, 3)))

    for run in (1, 2):
        for V in (256, 32):
            nblk = (n + V - 1) // V
            f = torch.empty(nblk, dtype=torch.uint8, device=dev)
            kb32 = ops.block_scales(b[:8], V, bits=32)
            kb16 = ops.block_scales(b, V, bits=16)
            kb = torch.empty(nblk, dtype=torch.int8, device=dev)
            given(run, "quantize", V, 8 * n, lambda: ops.quantize_blk(b[0], kb32, V, out=q),
                  lambda: ops.quantize(b[0], k, out=q))
            given(run, "quantize_i16", V, 6 * n + nblk, lambda: ops.quantize_i16_blk(b[0], kb16, V, out=o16, overflow=f),
                  lambda: ops.quantize_i16(b[0], 13, V, out=o16, overflow=f))
            given(run, "quantize_reduce W=8", V, 36 * n, lambda: ops.quantize_reduce_blk(b[:8], V, kblk=kb32, out=q),
                  lambda: ops.quantize_reduce(b[:8], k, out=q))
            for W in (4, 16):
                given(run, f"quantize_reduce_i16 W={W}", V, (4 * W + 2) * n + nblk,
                      lambda: ops.quantize_reduce_i16_blk(b[:W], V, kblk=kb16, out=o16, overflow=f),
                      lambda: ops.quantize_reduce_i16(b[:W], 13, V, out=o16, overflow=f))
            ops.quantize_reduce(b[:8], k, out=q)
            given(run, "dequantize_i32", V, 8 * n, lambda: ops.dequantize_blk(q, kb32, V, out=y),
                  lambda: ops.dequantize(q, k, out=y))
            given(run, "dequantize_i16", V, 6 * n, lambda: ops.dequantize_blk(o16, kb16, V, out=y),
                  lambda: ops.dequantize(o16, 13, out=y))
            given(run, "ps_apply", V, 12 * n, lambda: ops.ps_apply_blk(local, q, kb32, V, 0.1, out=y),
                  lambda: ops.ps_apply(local, q, k, 0.1, out=y))
            for W in (4, 16):
                auto(run, f"quantize_reduce_i16 W={W}", V, (4 * W + 2) * n + nblk,
                     lambda: ops.quantize_reduce_i16_blk(b[:W], V, out=o16, overflow=f, kblk_out=kb),
                     lambda: ops.block_scales(b[:W], V, bits=16, out=kb),
                     lambda: ops.quantize_reduce_i16_blk(b[:W], V, kblk=kb, out=o16, overflow=f),
                     lambda: ops.quantize_reduce_i16(b[:W], 13, V, out=o16, overflow=f))
            auto(run, "quantize_reduce W=8", V, 36 * n,
                 lambda: ops.quantize_reduce_blk(b[:8], V, out=q, kblk_out=kb),
                 lambda: ops.block_scales(b[:8], V, bits=32, out=kb),
                 lambda: ops.quantize_reduce_blk(b[:8], V, kblk=kb, out=q),
                 lambda: ops.quantize_reduce(b[:8], k, out=q))
            # the PS combine's composition: scales of the deltas, the fused reduce cannot take a base, so
            # the caller's second pass is the global-k combine's bytes again (timed as block_scales + sibling)
            auto(run, "ps_combine_ina W=8", V, 40 * n,
                 lambda: ops.ps_combine_ina_blk(local, b[:8], V, 0.1, out=y, kblk_out=kb),
                 lambda: ops.block_scales(b[:8], V, bits=32, base=local, out=kb),
                 lambda: ps.combine_ina(local, b[:8], k, 0.1, out=y),
                 lambda: ps.combine_ina(local, b[:8], k, 0.1, out=y))
            t_auto = _wall(lambda: ps.combine_ina(local, b[:8], "auto", 0.1, out=y))
            t_blk = _wall(lambda: ps.combine_ina(local, b[:8], "block", 0.1, out=y, block=V))
            rows.append(_row(f"ps.combine_ina k=block V={V} W=8 [wall, run {run}]", t_blk, 40 * n + nblk,
                             k_auto_wall_us=round(t_auto * 1e6, 2), ratio_to_k_auto=round(t_blk / t_auto, 3)))
    return rows


def run_ef(dev):
    """Error feedback (include/ina_ef.h) at the ResNet-50 size, cold caches, median of 20, the whole
    set twice in this process (run 1 / run 2).  Each EF call beside (a) the composition a caller
    writes today -- torch add, the sibling quantiser, the sibling dequantiser, torch sub, every buffer
    preallocated -- and (b) its non-EF sibling, timed twice (the two times' difference is the
    spread).  The bar, relative only: the EF call beats (a) by more than the spread.  Its ratio to
    sibling time x byte ratio is reported, not gated.  The packs against ef.quantize +
    pack_nga_split per worker."""
    from ina_amd import ef, ops
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(19)
    n, k, V, W = 25_557_032, 16, 256, 8
    nblk = (n + V - 1) // V
    xs = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(W)]
    rs = [torch.randn(n, device=dev, generator=gen) * 2.0 ** -(k + 2) for _ in range(W)]
    x, r, x16 = xs[0], rs[0], xs[0].bfloat16()
    v, d = torch.empty_like(x), torch.empty_like(x)
    q = torch.empty(n, dtype=torch.int32, device=dev)
    o16 = torch.empty(n, dtype=torch.int16, device=dev)
    f = torch.empty(nblk, dtype=torch.uint8, device=dev)
    kb32 = ops.block_scales([x], V, bits=32)
    kb16 = ops.block_scales([x], V, bits=16)
    kb = torch.empty(nblk, dtype=torch.int8, device=dev)
    hdrs = [torch.zeros((nblk, 16), dtype=torch.uint8, device=dev) for _ in range(W)]
    pays = [torch.empty((nblk, 4 * V), dtype=torch.uint8, device=dev) for _ in range(W)]
    key = (V, list(range(1, W + 1)), W, 1, 1)

    def row(run, name, nb_ef, nb_sib, f_ef, f_comp, f_sib):
        ta, te, tc, tb = _time(f_sib), _time(f_ef), _time(f_comp), _time(f_sib)
        lo, hi = min(ta, tb), max(ta, tb)
        rows.append(_row(f"{name} [ef, run {run}]", te, nb_ef, composition_us=round(tc * 1e6, 2),
                         sibling_us=[round(ta * 1e6, 2), round(tb * 1e6, 2)], sibling_spread_us=round((hi - lo) * 1e6, 2),
                         beats_composition_by_more_than_spread=bool(tc - te > hi - lo),
                         ratio_to_sibling_x_bytes=round(te / (lo * nb_ef / nb_sib), 3)))

    def comp(src, quant, deq):
        def run():
            torch.add(src, r, out=v)
            quant()
            deq()
            torch.sub(v, d, out=r)
        return run

    def per_worker(quant):
        def run():
            for w in range(W):
                ops.pack_nga_split(quant(w), V, w + 1, W, 1, 1, hdr=hdrs[w], pay=pays[w])
        return run

    for run in (1, 2):
        row(run, "quantize fp32 -> int32", 16 * n, 8 * n, lambda: ef.quantize(x, r, k, out=q),
            comp(x, lambda: ops.quantize(v, k, out=q), lambda: ops.dequantize(q, k, out=d)),
            lambda: ops.quantize(x, k, out=q))
        row(run, f"quantize_i16 fp32 -> int16 V={V}", 14 * n, 6 * n,
            lambda: ef.quantize_i16(x, r, 13, V, out=o16, overflow=f),
            comp(x, lambda: ops.quantize_i16(v, 13, V, out=o16, overflow=f), lambda: ops.dequantize(o16, 13, out=d)),
            lambda: ops.quantize_i16(x, 13, V, out=o16, overflow=f))
        row(run, "quantize bf16 -> int32", 14 * n, 6 * n, lambda: ef.quantize(x16, r, k, out=q),
            comp(x16, lambda: ops.quantize(v, k, out=q), lambda: ops.dequantize(q, k, out=d)),
            lambda: ops.quantize(x16, k, out=q))
        row(run, f"quantize_i16 bf16 -> int16 V={V} (12 B a value; the issue's byte ratio is 10/4)", 10 * n, 4 * n,
            lambda: ef.quantize_i16(x16, r, 13, V, out=o16, overflow=f),
            comp(x16, lambda: ops.quantize_i16(v, 13, V, out=o16, overflow=f), lambda: ops.dequantize(o16, 13, out=d)),
            lambda: ops.quantize_i16(x16, 13, V, out=o16, overflow=f))
        row(run, f"quantize_blk given V={V}", 16 * n, 8 * n, lambda: ef.quantize_blk(x, r, V, kblk=kb32, out=q),
            comp(x, lambda: ops.quantize_blk(v, kb32, V, out=q), lambda: ops.dequantize_blk(q, kb32, V, out=d)),
            lambda: ops.quantize_blk(x, kb32, V, out=q))
        row(run, f"quantize_blk auto V={V}", 16 * n, 12 * n, lambda: ef.quantize_blk(x, r, V, out=q, kblk_out=kb),
            comp(x, lambda: ops.quantize_blk(v, ops.block_scales([v], V, degree=1, out=kb), V, out=q),
                 lambda: ops.dequantize_blk(q, kb, V, out=d)),
            lambda: ops.quantize_blk(x, ops.block_scales([x], V, degree=1, out=kb), V, out=q))
        row(run, f"quantize_i16_blk given V={V}", 14 * n, 6 * n,
            lambda: ef.quantize_i16_blk(x, r, V, kblk=kb16, out=o16, overflow=f),
            comp(x, lambda: ops.quantize_i16_blk(v, kb16, V, out=o16, overflow=f),
                 lambda: ops.dequantize_blk(o16, kb16, V, out=d)),
            lambda: ops.quantize_i16_blk(x, kb16, V, out=o16, overflow=f))
        row(run, f"quantize_i16_blk auto V={V}", 14 * n, 10 * n,
            lambda: ef.quantize_i16_blk(x, r, V, out=o16, overflow=f, kblk_out=kb),
            comp(x, lambda: ops.quantize_i16_blk(v, ops.block_scales([v], V, bits=16, degree=1, out=kb), V, out=o16,
                                                 overflow=f), lambda: ops.dequantize_blk(o16, kb, V, out=d)),
            lambda: ops.quantize_i16_blk(x, ops.block_scales([x], V, bits=16, degree=1, out=kb), V, out=o16,
                                         overflow=f))
        row(run, f"block_scales W={W} V={V}", 8 * W * n, 4 * W * n, lambda: ef.block_scales(xs, rs, V, out=kb),
            lambda: ([torch.add(a, b, out=v) for a, b in zip(xs, rs)], ops.block_scales(xs, V, out=kb)),
            lambda: ops.block_scales(xs, V, out=kb))
        row(run, f"quantize_pack_nga_multi_split W={W} V={V}", 16 * W * n, 8 * W * n,
            lambda: ef.quantize_pack_nga_multi_split(xs, rs, k, *key, hdrs=hdrs, pays=pays),
            per_worker(lambda w: ef.quantize(xs[w], rs[w], k, out=q)),
            lambda: ops.quantize_pack_nga_multi_split(xs, k, *key, hdrs=hdrs, pays=pays))
        row(run, f"quantize_pack_nga_multi_split_blk given W={W} V={V}", 16 * W * n, 8 * W * n,
            lambda: ef.quantize_pack_nga_multi_split(xs, rs, kb32, *key, hdrs=hdrs, pays=pays),
            per_worker(lambda w: ef.quantize_blk(xs[w], rs[w], V, kblk=kb32, out=q)[0]),
            lambda: ops.quantize_pack_nga_multi_split_blk(xs, *key, kblk=kb32, hdrs=hdrs, pays=pays))
        row(run, f"quantize_pack_nga_multi_split_blk auto W={W} V={V}", 16 * W * n, 8 * W * n,
            lambda: ef.quantize_pack_nga_multi_split(xs, rs, None, *key, kblk_out=kb, hdrs=hdrs, pays=pays),
            lambda: (ef.block_scales(xs, rs, V, out=kb),
                     per_worker(lambda w: ef.quantize_blk(xs[w], rs[w], V, kblk=kb, out=q)[0])()),
            lambda: ops.quantize_pack_nga_multi_split_blk(xs, *key, kblk_out=kb, hdrs=hdrs, pays=pays))
    return rows


def run_ef_shard(dev):
    """Error feedback on the sharded int16 wire (include/ina_shard_ef.h) at the ResNet-50 size, cold
    caches, median of 20, the set twice in this process (run 1 / run 2), V = 256 and 32.  Each EF wire
    quantiser (16 B a value: x, r, word, r') beside (a) its non-EF wire sibling (8 B a value) timed
    twice -- the bar is sibling time x 16/8 plus the spread of the sibling's two timings -- and (b)
    the composition a caller would otherwise write, every buffer preallocated: torch add, the
    sibling, q16 out of the word and q16 * 2^-k in torch (two shifts and a multiply; the per-value
    2^-k of the block form is made once, outside the timing), torch sub.  Nothing is gated."""
    from ina_amd import ef, ops
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(23)
    n, k = 25_557_032, 9
    x = torch.randn(n, device=dev, generator=gen) * 1e-2
    r = torch.randn(n, device=dev, generator=gen) * 2.0 ** -(k + 2)
    v, d = torch.empty_like(x), torch.empty_like(x)
    w = torch.empty(n, dtype=torch.int32, device=dev)
    t = torch.empty(n, dtype=torch.int32, device=dev)

    def comp(quant, inv):
        def run():
            torch.add(x, r, out=v)
            quant()
            torch.bitwise_left_shift(w, 10, out=t)
            torch.bitwise_right_shift(t, 10, out=t)          # the word's low 22 bits, sign-extended
            torch.mul(t, inv, out=d)
            torch.sub(v, d, out=r)
        return run

    def row(run, name, f_ef, f_comp, f_sib):
        ta, te, tc, tb = _time(f_sib), _time(f_ef), _time(f_comp), _time(f_sib)
        lo, hi = min(ta, tb), max(ta, tb)
        rows.append(_row(f"{name} [ef wire, run {run}]", te, 16 * n, composition_us=round(tc * 1e6, 2),
                         composition_over_ef=round(tc / te, 2),
                         sibling_us=[round(ta * 1e6, 2), round(tb * 1e6, 2)], sibling_spread_us=round((hi - lo) * 1e6, 2),
                         bar_us=round((2 * lo + hi - lo) * 1e6, 2), within_bar=bool(te <= 2 * lo + hi - lo),
                         ratio_to_sibling_x_bytes=round(te / (2 * lo), 3)))

    for run in (1, 2):
        row(run, f"quantize_i16_wire k={k}", lambda: ef.quantize_i16_wire(x, r, k, out=w),
            comp(lambda: ops.quantize_i16_wire(v, k, out=w), 2.0 ** -k), lambda: ops.quantize_i16_wire(x, k, out=w))
        for V in (256, 32):
            kb = ops.block_scales([x], V, bits=16, degree=64)
            inv = torch.exp2(-kb.float()).repeat_interleave(V)[:n].contiguous()
            row(run, f"quantize_i16_wire_blk V={V}", lambda: ef.quantize_i16_wire_blk(x, r, kb, V, out=w),
                comp(lambda: ops.quantize_i16_wire_blk(v, kb, V, out=w), inv),
                lambda: ops.quantize_i16_wire_blk(x, kb, V, out=w))
            del inv
    return rows


def run_sr(dev):
    """Stochastic rounding (include/ina_sr.h) at the ResNet-50 size, cold caches, median of 20, the set
    twice in this process (run 1 / run 2): sr.quantize, sr.quantize_i16 (V = 256) and sr.quantize_i16_wire
    from fp32 and bf16 buckets, each beside its round-to-nearest sibling timed twice in the same run.  An
    SR call moves its sibling's bytes, so what is reported is SR time over sibling time (the faster of
    the sibling's two timings) next to the sibling's own spread.  Nothing is gated: no bar was known for
    ten Philox rounds under these streams."""
    from ina_amd import ops, sr, wire
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(29)
    n, k, V, seed = 25_557_032, 9, 256, 0x1234
    x32 = torch.randn(n, device=dev, generator=gen) * 1e-2
    q32 = torch.empty(n, dtype=torch.int32, device=dev)
    q16 = torch.empty(n, dtype=torch.int16, device=dev)
    ovf = torch.empty((n + V - 1) // V, dtype=torch.uint8, device=dev)

    def row(run, name, nbytes, f_sr, f_sib):
        ta, ts, tb = _time(f_sib), _time(f_sr), _time(f_sib)
        lo, hi = min(ta, tb), max(ta, tb)
        rows.append(_row(f"{name} [sr, run {run}]", ts, nbytes, sibling_us=[round(ta * 1e6, 2), round(tb * 1e6, 2)],
                         sibling_spread_us=round((hi - lo) * 1e6, 2), sr_over_sibling=round(ts / lo, 3),
                         sr_over_slower_sibling=round(ts / hi, 3)))

    for run in (1, 2):
        for x, tag in ((x32, "f32"), (x32.to(torch.bfloat16), "bf16")):
            b = x.element_size()
            row(run, f"quantize {tag}->i32", (b + 4) * n, lambda: sr.quantize(x, k, seed, step=run, out=q32),
                lambda: ops.quantize(x, k, out=q32))
            row(run, f"quantize_i16 {tag}->i16 V={V}", (b + 2) * n + ovf.numel(),
                lambda: sr.quantize_i16(x, k, V, seed, step=run, out=q16, overflow=ovf),
                lambda: ops.quantize_i16(x, k, V, out=q16, overflow=ovf))
            row(run, f"quantize_i16_wire {tag}->wire", (b + 4) * n,
                lambda: sr.quantize_i16_wire(x, k, seed, step=run, out=q32), lambda: wire.quantize(x, k, out=q32))
    return rows


def run_sr_packets(dev):
    """Stochastic rounding on the packet path (include/ina_pkt_sr.h) at the ResNet-50 size, cold caches,
    median of 20, the set twice in this process (run 1 / run 2): the 8-worker split pack at V = 256 and
    32 from fp32 and bf16 buckets, its block-scaled calls (scales given, and AUTO) from fp32, and the
    single-worker packed call.  Each SR call is timed beside its round-to-nearest sibling, timed twice in
    the same run (their difference is the spread), and beside the composition it replaces: per worker,
    sr.quantize into a preallocated int32 buffer, then the plain pack of it.  Nothing is gated."""
    from ina_amd import ops, sr
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    n, k, W, seed = 25_557_032, 9, 8, 0x1234
    xs32 = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(W)]
    xs16 = [x.to(torch.bfloat16) for x in xs32]
    base = torch.randn(n, device=dev, generator=gen) * 1e-3
    q32 = torch.empty(n, dtype=torch.int32, device=dev)
    bm = [1 << w for w in range(W)]

    def row(run, name, nbytes, f_sr, f_sib, f_comp):
        ta, ts, tc, tb = _time(f_sib), _time(f_sr), _time(f_comp), _time(f_sib)
        lo, hi = min(ta, tb), max(ta, tb)
        rows.append(_row(f"{name} [sr, run {run}]", ts, nbytes, sibling_us=[round(ta * 1e6, 2), round(tb * 1e6, 2)],
                         sibling_spread_us=round((hi - lo) * 1e6, 2), composition_us=round(tc * 1e6, 2),
                         sr_over_sibling=round(ts / lo, 3), sr_over_composition=round(ts / tc, 3),
                         beats_composition_by_more_than_spread=bool(tc - ts > hi - lo)))

    for run in (1, 2):
        for V in (256, 32):
            npk = (n + V - 1) // V
            hs = [torch.zeros((npk, 16), dtype=torch.uint8, device=dev) for _ in range(W)]
            ps = [torch.empty((npk, 4 * V), dtype=torch.uint8, device=dev) for _ in range(W)]
            rows_b = W * npk * (16 + 4 * V)
            kw = dict(base=base, hdrs=hs, pays=ps)

            def comp(xs):
                # (no SR quantiser takes block scales: for the block calls the global-k one stands in,
                # the same bytes and the same Philox work)
                for w in range(W):
                    sr.quantize(xs[w], k, seed, step=run, sub=w, base=base, out=q32)
                    ops.pack_nga_split(q32, V, bm[w], W, 1, 1, hdr=hs[w], pay=ps[w])

            for xs, tag in ((xs32, "f32"), (xs16, "bf16")):
                nb = W * n * xs[0].element_size() + 4 * n + rows_b
                row(run, f"multi_split W=8 {tag} V={V}", nb,
                    lambda: sr.quantize_pack_nga_multi_split(xs, k, V, bm, W, 1, 1, seed, step=run, **kw),
                    lambda: ops.quantize_pack_nga_multi_split(xs, k, V, bm, W, 1, 1, **kw), lambda: comp(xs))
            kblk = sr.block_scales(xs32, V, base=base)
            kout = torch.empty_like(kblk)
            nb = W * n * 4 + 4 * n + rows_b + npk
            row(run, f"multi_split_blk GIVEN W=8 f32 V={V}", nb,
                lambda: sr.quantize_pack_nga_multi_split(xs32, kblk, V, bm, W, 1, 1, seed, step=run, **kw),
                lambda: ops.quantize_pack_nga_multi_split_blk(xs32, V, bm, W, 1, 1, kblk=kblk, **kw),
                lambda: comp(xs32))
            row(run, f"multi_split_blk AUTO W=8 f32 V={V}", nb,
                lambda: sr.quantize_pack_nga_multi_split(xs32, None, V, bm, W, 1, 1, seed, step=run, kblk_out=kout, **kw),
                lambda: ops.quantize_pack_nga_multi_split_blk(xs32, V, bm, W, 1, 1, kblk_out=kout, **kw),
                lambda: comp(xs32))
            stride = ops.nga_stride(V)
            out = torch.empty((npk, stride), dtype=torch.uint8, device=dev)

            def comp1():
                sr.quantize(xs32[0], k, seed, step=run, base=base, out=q32)
                ops.pack_nga(q32, V, 1, W, 1, 1, out=out)
            row(run, f"packed one worker f32 V={V}", 8 * n + npk * stride,
                lambda: sr.quantize_pack_nga(xs32[0], k, V, 1, W, 1, 1, seed, step=run, base=base, out=out),
                lambda: ops.quantize_pack_nga(xs32[0], k, V, 1, W, 1, 1, base=base, out=out), comp1)
            del hs, ps, out
    return rows


def run_sr_reduce(dev):
    """Stochastic rounding in the fused quantise + reduce calls (include/ina_reduce_sr.h) at the ResNet-50
    size with W = 8 workers, cold caches, median of 20, the set twice in this process (run 1 / run 2):
    sr.quantize_reduce at config 2's k and sr.quantize_reduce_i16 at config 4's k and V, from fp32 and
    bf16 buckets.  Each SR call is timed beside its round-to-nearest sibling, timed twice in the same run
    (their difference is the spread), and beside the composition it replaces: W x sr.quantize /
    sr.quantize_i16 into W preallocated temporaries, then ops.sum_reduce / ops.sum_reduce_i16 (the flags
    of the composition are not OR-ed: that would only add to it).  Nothing is gated here; DESIGN 4.1m
    reads the rows."""
    from ina_amd import ops, sr
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(37)
    n, W, V, seed = 25_557_032, 8, 256, 0x1234
    xs32 = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(W)]
    xs16 = [x.to(torch.bfloat16) for x in xs32]
    o32 = torch.empty(n, dtype=torch.int32, device=dev)
    o16 = torch.empty(n, dtype=torch.int16, device=dev)
    ovf = torch.empty((n + V - 1) // V, dtype=torch.uint8, device=dev)
    t32 = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(W)]    # the composition's scratch
    t16 = [torch.empty(n, dtype=torch.int16, device=dev) for _ in range(W)]
    tov = torch.empty_like(ovf)

    def row(run, name, nbytes, f_sr, f_sib, f_comp):
        ta, ts, tc, tb = _time(f_sib), _time(f_sr), _time(f_comp), _time(f_sib)
        lo, hi = min(ta, tb), max(ta, tb)
        rows.append(_row(f"{name} [sr, run {run}]", ts, nbytes, sibling_us=[round(ta * 1e6, 2), round(tb * 1e6, 2)],
                         sibling_spread_us=round((hi - lo) * 1e6, 2), composition_us=round(tc * 1e6, 2),
                         sr_over_sibling=round(ts / lo, 3), sr_over_composition=round(ts / tc, 3),
                         beats_composition_by_more_than_spread=bool(tc - ts > hi - lo)))

    for run in (1, 2):
        for xs, tag in ((xs32, "f32"), (xs16, "bf16")):
            b = xs[0].element_size()

            def comp32(k=16):
                for w in range(W):
                    sr.quantize(xs[w], k, seed, step=run, sub=w, out=t32[w])
                ops.sum_reduce(t32, out=o32)

            def comp16(k=13):
                for w in range(W):
                    sr.quantize_i16(xs[w], k, V, seed, step=run, sub=w, out=t16[w], overflow=tov)
                ops.sum_reduce_i16(t16, V, out=o16, overflow=ovf)

            row(run, f"quantize_reduce W={W} {tag}->i32 (C2 size, k=16)", (W * b + 4) * n,
                lambda: sr.quantize_reduce(xs, 16, seed, step=run, out=o32),
                lambda: ops.quantize_reduce(xs, 16, out=o32), comp32)
            row(run, f"quantize_reduce_i16 W={W} {tag}->i16 V={V} (C4 size, k=13)", (W * b + 2) * n + ovf.numel(),
                lambda: sr.quantize_reduce_i16(xs, 13, V, seed, step=run, out=o16, overflow=ovf),
                lambda: ops.quantize_reduce_i16(xs, 13, V, out=o16, overflow=ovf), comp16)
    return rows


def run_blk_sr(dev):
    """Stochastic rounding with per-block scales (include/ina_blk_sr.h) at the ResNet-50 size, cold caches,
    median of 20, the set twice in this process (run 1 / run 2): blk_sr.quantize_reduce at W = 8 and
    blk_sr.quantize_reduce_i16 at W = 4 and W = 16, V = 256 and 32, from fp32 and bf16 buckets, scales given
    and computed (AUTO).  Each call is timed beside its round-to-nearest block sibling, timed twice in the
    same run (their difference is the spread), its global-k stochastic sibling, and the composition it
    replaces: blk_sr.block_scales where AUTO, then W x blk_sr.quantize into W preallocated int32
    temporaries, then ops.sum_reduce.  Nothing is gated here; DESIGN 4.1n reads the rows."""
    from ina_amd import blk, blk_sr, ops, sr
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(41)
    n, seed = 25_557_032, 0x1234
    xs32 = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(16)]
    xs16 = [x.to(torch.bfloat16) for x in xs32]
    o32 = torch.empty(n, dtype=torch.int32, device=dev)
    o16 = torch.empty(n, dtype=torch.int16, device=dev)
    t32 = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(16)]   # the composition's scratch

    def row(run, name, nbytes, f_sr, f_sib, f_glob, f_comp):
        ta, ts, tg, tc, tb = _time(f_sib), _time(f_sr), _time(f_glob), _time(f_comp), _time(f_sib)
        lo, hi = min(ta, tb), max(ta, tb)
        rows.append(_row(f"{name} [blk sr, run {run}]", ts, nbytes,
                         sibling_us=[round(ta * 1e6, 2), round(tb * 1e6, 2)], sibling_spread_us=round((hi - lo) * 1e6, 2),
                         global_k_sr_us=round(tg * 1e6, 2), composition_us=round(tc * 1e6, 2),
                         sr_over_sibling=round(ts / lo, 3), sr_over_global_k_sr=round(ts / tg, 3),
                         sr_over_composition=round(ts / tc, 3),
                         beats_composition_by_more_than_spread=bool(tc - ts > hi - lo)))

    for run in (1, 2):
        for V in (256, 32):
            nblk = (n + V - 1) // V
            ovf = torch.empty(nblk, dtype=torch.uint8, device=dev)
            kout = torch.empty(nblk, dtype=torch.int8, device=dev)
            for bits, W in ((32, 8), (16, 4), (16, 16)):
                k = sr.scale_for(0.06, W, bits)                     # the buckets' range: 6 sigma
                for src, tag in ((xs32, "f32"), (xs16, "bf16")):
                    xs, b = src[:W], src[0].element_size()
                    kb = blk_sr.block_scales(xs, V, bits=bits, degree=W)
                    for auto in (False, True):
                        kw = dict(kblk=None if auto else kb, kblk_out=kout)

                        def comp():
                            kk = blk_sr.block_scales(xs, V, bits=bits, degree=W, out=kout) if auto else kb
                            for w in range(W):
                                blk_sr.quantize(xs[w], kk, V, seed, step=run, sub=w, out=t32[w])
                            ops.sum_reduce(t32[:W], out=o32)

                        mode = "AUTO" if auto else "GIVEN"
                        if bits == 32:
                            row(run, f"quantize_reduce_blk W={W} {tag}->i32 V={V} {mode}", (W * b + 4) * n + nblk,
                                lambda: blk_sr.quantize_reduce(xs, V, seed, step=run, out=o32, **kw),
                                lambda: blk.quantize_reduce(xs, V, out=o32, **kw),
                                lambda: sr.quantize_reduce(xs, k, seed, step=run, out=o32), comp)
                        else:
                            row(run, f"quantize_reduce_i16_blk W={W} {tag}->i16 V={V} {mode}", (W * b + 2) * n + 2 * nblk,
                                lambda: blk_sr.quantize_reduce_i16(xs, V, seed, step=run, out=o16, overflow=ovf, **kw),
                                lambda: blk.quantize_reduce_i16(xs, V, out=o16, overflow=ovf, **kw),
                                lambda: sr.quantize_reduce_i16(xs, k, V, seed, step=run, out=o16, overflow=ovf), comp)
    return rows


def run_blk_x16(dev, dtype=torch.bfloat16):
    """Per-block scales for bf16 buckets (include/ina_x16_blk.h) at the ResNet-50 size, V = 256 and 32, cold
    caches, median of 20, the whole set twice in this process (run 1 / run 2).  Each 16-bit call beside (a) the
    fp32 block-scaled sibling on the widened bucket, timed twice -- the two times' difference is the spread --
    and (b) widen into a preallocated fp32 buffer, then the sibling.  The bar (run_x16's, relative only): the
    16-bit call beats (b) and is no slower than (a) plus (a)'s spread."""
    from ina_amd import blk, ops
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(18)
    n, Wmax, Wp = 25_557_032, 16, 8
    name16 = {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]
    b32 = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(Wmax)]
    b16 = [b.to(dtype) for b in b32]
    b32 = [b.float() for b in b16]                       # the widened buckets: the same values
    wid = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(Wmax)]
    base = torch.randn(n, device=dev, generator=gen) * 1e-2
    q = torch.empty(n, dtype=torch.int32, device=dev)
    o16 = torch.empty(n, dtype=torch.int16, device=dev)
    y32 = torch.empty(n, dtype=torch.float32, device=dev)
    y16 = torch.empty(n, dtype=dtype, device=dev)

    def widen(W):
        return lambda: [w.copy_(x) for w, x in zip(wid[:W], b16[:W])]

    def trio(run, name, V, nb16, f16, f32, pre):
        t32a = _time(f32)
        t16 = _time(f16)
        tw = _time(lambda: (pre(), f32()))
        t32b = _time(f32)
        lo, hi = min(t32a, t32b), max(t32a, t32b)
        rows.append(_row(f"{name} V={V} [{name16} blk, run {run}]", t16, nb16,
                         sibling_us=[round(t32a * 1e6, 2), round(t32b * 1e6, 2)],
                         sibling_spread_us=round((hi - lo) * 1e6, 2), widen_then_sibling_us=round(tw * 1e6, 2),
                         faster_than_widen_then_sibling=bool(t16 < tw),
                         no_slower_than_sibling=bool(t16 <= hi + (hi - lo))))

    for run in (1, 2):
        for V in (256, 32):
            nblk = (n + V - 1) // V
            f = torch.empty(nblk, dtype=torch.uint8, device=dev)
            kb = torch.empty(nblk, dtype=torch.int8, device=dev)
            kb32 = ops.block_scales(b32[:8], V, bits=32)
            kb16 = ops.block_scales(b32, V, bits=16)
            trio(run, "block_scales W=8", V, 16 * n + nblk, lambda: blk.block_scales(b16[:8], V, out=kb),
                 lambda: ops.block_scales(b32[:8], V, out=kb), widen(8))
            trio(run, "quantize", V, 6 * n + nblk, lambda: blk.quantize(b16[0], kb32, V, out=q),
                 lambda: ops.quantize_blk(b32[0], kb32, V, out=q), widen(1))
            trio(run, "quantize_i16", V, 4 * n + 2 * nblk, lambda: blk.quantize_i16(b16[0], kb16, V, out=o16, overflow=f),
                 lambda: ops.quantize_i16_blk(b32[0], kb16, V, out=o16, overflow=f), widen(1))
            trio(run, "quantize_reduce W=8 auto", V, 20 * n + nblk,
                 lambda: blk.quantize_reduce(b16[:8], V, out=q, kblk_out=kb),
                 lambda: ops.quantize_reduce_blk(b32[:8], V, out=q, kblk_out=kb), widen(8))
            for W in (4, 16):
                trio(run, f"quantize_reduce_i16 W={W} auto", V, (2 * W + 2) * n + 2 * nblk,
                     lambda: blk.quantize_reduce_i16(b16[:W], V, out=o16, overflow=f, kblk_out=kb),
                     lambda: ops.quantize_reduce_i16_blk(b32[:W], V, out=o16, overflow=f, kblk_out=kb), widen(W))
            # decode: the 16-bit call against the fp32 decode, and against the fp32 decode + a narrowing copy
            ops.quantize_reduce_blk(b32[:8], V, kblk=kb32, out=q)
            ops.quantize_reduce_i16_blk(b32, V, kblk=kb16, out=o16, overflow=f)
            trio(run, "dequantize_i32", V, 6 * n + nblk, lambda: blk.dequantize(q, kb32, V, out=y16),
                 lambda: ops.dequantize_blk(q, kb32, V, out=y32), lambda: y16.copy_(y32))
            trio(run, "dequantize_i16", V, 4 * n + nblk, lambda: blk.dequantize(o16, kb16, V, out=y16),
                 lambda: ops.dequantize_blk(o16, kb16, V, out=y32), lambda: y16.copy_(y32))
            # the 8 workers' split packs in one launch, against an fp32 base
            npk = nblk
            hdrs = [torch.zeros((npk, 16), dtype=torch.uint8, device=dev) for _ in range(Wp)]
            pays = [torch.empty((npk, 4 * V), dtype=torch.uint8, device=dev) for _ in range(Wp)]
            args = (V, list(range(1, Wp + 1)), Wp, 1, 1)
            out_b = Wp * (npk * 16 + npk * 4 * V)
            kbp = ops.block_scales(b32[:Wp], V, bits=32, base=base)
            for mode, kw in (("auto", dict(kblk_out=kb)), ("given", dict(kblk=kbp))):
                trio(run, f"quantize_pack_nga_multi_split W={Wp} {mode}", V, (2 * Wp + 4) * n + out_b + nblk,
                     lambda: blk.quantize_pack_nga_multi_split(b16[:Wp], *args, base=base, hdrs=hdrs, pays=pays, **kw),
                     lambda: ops.quantize_pack_nga_multi_split_blk(b32[:Wp], *args, base=base, hdrs=hdrs, pays=pays, **kw),
                     widen(Wp))
            del hdrs, pays
    return rows


def run_blk_packets(dev):
    """Per-block scales on the packet path (include/ina_pkt_blk.h) at the ResNet-50 size, W = 8, V = 256
    and 32, cold caches, median of 20, the whole set twice in this process (run 1 / run 2), as run_blk.
    The GIVEN multi split pack beside ina_quantize_pack_nga_multi_split, and apply_completed_blk on
    split rows beside the packed apply_completed on the same batch (the switch's output for 8 worker
    streams, 1 packet in 8 completed): sibling timed twice, bar = sibling time x bytes ratio + spread.
    The AUTO pack beside what a caller writes today: block_scales with base, then the GIVEN pack."""
    from ina_amd import ops
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(18)
    n, k, W = 25_557_032, 16, 8
    xs = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(W)]
    base = torch.randn(n, device=dev, generator=gen) * 1e-2
    y = torch.empty(n, dtype=torch.float32, device=dev)
    bitmaps = [1 << w for w in range(W)]

    def given(run, name, nb_sib, nblk, f_blk, f_sib):
        ta, tb, tc = _time(f_sib), _time(f_blk), _time(f_sib)
        lo, hi = min(ta, tc), max(ta, tc)
        bar = hi * (nb_sib + nblk) / nb_sib + (hi - lo)
        rows.append(_row(f"{name} [blk given, run {run}]", tb, nb_sib + nblk,
                         sibling_us=[round(ta * 1e6, 2), round(tc * 1e6, 2)], sibling_spread_us=round((hi - lo) * 1e6, 2),
                         bar_us=round(bar * 1e6, 2), bar_met=bool(tb <= bar)))
        return hi - lo

    for run in (1, 2):
        for V in (256, 32):
            npk = (n + V - 1) // V
            hdrs = [torch.zeros((npk, 16), dtype=torch.uint8, device=dev) for _ in range(W)]
            pays = [torch.empty((npk, 4 * V), dtype=torch.uint8, device=dev) for _ in range(W)]
            kb = ops.block_scales(xs, V, bits=32, base=base)
            kout = torch.empty(npk, dtype=torch.int8, device=dev)
            nb_pack = (4 * W + 4) * n + W * npk * (16 + 4 * V)
            spread = given(run, f"quantize_pack_nga_multi_split W={W} V={V}", nb_pack, npk,
                           lambda: ops.quantize_pack_nga_multi_split_blk(xs, V, bitmaps, W, 1, 1, base=base, kblk=kb,
                                                                         hdrs=hdrs, pays=pays),
                           lambda: ops.quantize_pack_nga_multi_split(xs, k, V, bitmaps, W, 1, 1, base=base, hdrs=hdrs,
                                                                     pays=pays))
            ta = _time(lambda: ops.quantize_pack_nga_multi_split_blk(xs, V, bitmaps, W, 1, 1, base=base, kblk_out=kout,
                                                                     hdrs=hdrs, pays=pays))
            tc = _time(lambda: (ops.block_scales(xs, V, bits=32, base=base, out=kout),
                                ops.quantize_pack_nga_multi_split_blk(xs, V, bitmaps, W, 1, 1, base=base, kblk=kout,
                                                                      hdrs=hdrs, pays=pays)))
            rows.append(_row(f"quantize_pack_nga_multi_split W={W} V={V} [blk auto, run {run}]", ta, nb_pack + npk,
                             scales_then_given_us=round(tc * 1e6, 2), sibling_spread_us=round(spread * 1e6, 2),
                             beats_scales_then_given_by_more_than_spread=bool(tc - ta > spread)))
            # the PS apply on the switch's output: split rows against the packed rows of the same batch
            slots = max(16384, npk)                      # a pool for the whole bucket: no slot is shared
            ops.quantize_pack_nga_multi_split_blk(xs, V, bitmaps, W, 1, 1, base=base, kblk=kb, hdrs=hdrs, pays=pays,
                                                  num_slots=slots)
            hd = torch.stack(hdrs, 1).reshape(W * npk, 16).contiguous()
            pa = torch.stack(pays, 1).reshape(W * npk, 4 * V).contiguous()
            del hdrs, pays
            act_s = ops.Switch(V, slots, 1, dev).process_split(hd, pa)
            rows_p = ops.quantize_pack_nga_multi(xs, k, V, bitmaps, W, 1, 1, base=base, num_slots=slots)
            pk = torch.stack(rows_p, 1).reshape(W * npk, -1).contiguous()
            del rows_p
            act_p = ops.Switch(V, slots, 1, dev).process(pk)
            done = int((act_s == 1).sum()), int((act_p == 1).sum())          # ACT_FWD_AGG
            assert done == (npk, npk), done
            nb_apply = npk * (16 + 4 * V) + W * npk + 8 * n
            given(run, f"apply_completed (split rows vs packed) W={W} V={V}", nb_apply, npk,
                  lambda: ops.apply_completed_blk(hd, act_s, V, 1, base, kb, 0.1, out=y, pay=pa),
                  lambda: ops.apply_completed(pk, act_p, V, 1, base, k, 0.1, out=y))
            del hd, pa, pk
    return rows


def run_blk_switch(dev):
    """Per-block scales in the fused switch + PS step (include/ina_switch_blk.h) at the ResNet-50 size,
    W = 8, V = 256 and 32, split rows, cold caches, median of 20, the whole set twice (run 1 / run 2), as
    run_blk_packets.  The batch is the steady-state one -- last step's acks in front of the 8 workers'
    packets, with descriptors, as bench.py's measure_packet_path builds it -- packed by the AUTO multi
    split pack.  Row 1: the fused block-scaled step beside the global-k fused step on the same batch
    (sibling timed before and after; bar = sibling time x bytes ratio + the sibling's spread; reported,
    not gated).  Row 2: beside what a caller wrote before, process_split then apply_completed_blk."""
    from ina_amd import ops
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(19)
    n, k, W = 25_557_032, 16, 8
    xs = [torch.randn(n, device=dev, generator=gen) * 1e-2 for _ in range(W)]
    glob = torch.randn(n, device=dev, generator=gen) * 1e-2
    upd = torch.empty_like(glob)
    bms = [w + 1 for w in range(W)]
    ws = 1.0 / (W + 1)
    for run in (1, 2):
        for V in (256, 32):
            npk = (n + V - 1) // V
            slots = 1 << 17 if V == 256 else 1 << 20
            hdr = torch.zeros(((W + 1) * npk, 16), dtype=torch.uint8, device=dev)      # [acks | workers]
            pay = torch.zeros(((W + 1) * npk, 4 * V), dtype=torch.uint8, device=dev)
            desc = torch.empty((W + 1) * npk, dtype=torch.int64, device=dev)
            acts = torch.empty((W + 1) * npk, dtype=torch.uint8, device=dev)
            kb = torch.empty(npk, dtype=torch.int8, device=dev)
            sw = ops.Switch(V, num_slots=slots, switch_id=1, device=dev)
            ops.quantize_pack_nga_multi_split_blk(xs, V, bms, W, 1, 1, base=glob, num_slots=slots, kblk_out=kb,
                                                  hdrs=list(hdr[npk:].view(W, npk, 16).unbind(0)),
                                                  pays=list(pay[npk:].view(W, npk, 4 * V).unbind(0)),
                                                  descs=list(desc[npk:].view(W, npk).unbind(0)))
            ops.nga_descriptors(hdr[:npk], out=desc[:npk])

            def fused(kk):
                sw.process_apply_split(hdr, pay, 1, glob, kk, ws, out=upd, ack_hdr=hdr[:npk], ack_desc=desc[:npk],
                                       keep_forwarded=False, actions=acts, desc=desc)

            def two_calls():
                sw.process_split(hdr, pay, actions=acts, desc=desc)
                ops.apply_completed_blk(hdr, acts, V, 1, glob, kb, ws, out=upd, acks=hdr[:npk], pay=pay)

            fused(kb)                                       # the first step's ack rows are another switch's;
            fused(kb)                                       # from the second on they are this one's
            done = int((acts[npk:] == 1).sum()), int((acts[:npk] == 3).sum())        # ACT_FWD_AGG, ACT_FWD_ACK
            assert done == (npk, npk), done
            npk_all = W * npk
            nb = (npk * 8 + (npk_all + npk) * (16 + 4 * V) + npk * (4 * V + 5) + npk_all + npk + 8 * n + 16 * npk)
            ta, tb, tc = _time(lambda: fused(k)), _time(lambda: fused(kb)), _time(lambda: fused(k))
            lo, hi = min(ta, tc), max(ta, tc)
            bar = hi * (nb + npk) / nb + (hi - lo)
            rows.append(_row(f"switch + PS fused, split rows W={W} V={V} [blk, run {run}]", tb, nb + npk,
                             sibling_us=[round(ta * 1e6, 2), round(tc * 1e6, 2)],
                             sibling_spread_us=round((hi - lo) * 1e6, 2), bar_us=round(bar * 1e6, 2),
                             bar_met=bool(tb <= bar)))
            t2 = _time(two_calls)
            rows.append(_row(f"process_split + apply_completed_blk, split rows W={W} V={V} [run {run}]", t2, nb + npk,
                             fused_blk_us=round(tb * 1e6, 2), sibling_spread_us=round((hi - lo) * 1e6, 2),
                             fused_beats_two_calls_by_more_than_spread=bool(t2 - tb > hi - lo)))
            del hdr, pay, desc, acts, sw
    return rows


DEFAULTS = {"max_blocks": 16384, "reduce_blocks": 0, "stream_blocks": 16384, "combine_blocks": 256,
            "combine_ina_blocks": 8192, "ew_blocks": 1 << 24}


def run_blk_shard(dev):
    """The block-scaled int16 wire (include/ina_shard_blk.h) at the ResNet-50 size, V = 256 and 32, cold
    caches, median of 20, the whole set twice in this process (run 1 / run 2), as run_blk:
    quantize_i16_wire_blk and i16_wire_finish_blk (y + out16 + flags), each beside its global-k sibling
    timed twice.  Bar: sibling time x (bytes + n/V) / bytes + the spread of the sibling's two timings;
    reported, not gated."""
    from ina_amd import ops
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(18)
    n, k = 25_557_032, 9
    x = torch.randn(n, device=dev, generator=gen) * 1e-2
    wire = torch.empty(n, dtype=torch.int32, device=dev)
    o16 = torch.empty(n, dtype=torch.int16, device=dev)
    y = torch.empty(n, dtype=torch.float32, device=dev)

    def given(run, name, V, nb_sib, f_blk, f_sib):
        nblk = (n + V - 1) // V
        ta, tb, tc = _time(f_sib), _time(f_blk), _time(f_sib)
        lo, hi = min(ta, tc), max(ta, tc)
        bar = hi * (nb_sib + nblk) / nb_sib + (hi - lo)
        rows.append(_row(f"{name} V={V} [blk given, run {run}]", tb, nb_sib + nblk,
                         sibling_us=[round(ta * 1e6, 2), round(tc * 1e6, 2)], sibling_spread_us=round((hi - lo) * 1e6, 2),
                         bar_us=round(bar * 1e6, 2), bar_met=bool(tb <= bar)))

    for run in (1, 2):
        for V in (256, 32):
            nblk = (n + V - 1) // V
            f = torch.empty(nblk, dtype=torch.uint8, device=dev)
            kb = ops.block_scales([x], V, bits=16, degree=64)          # the 64-rank wire's scales
            given(run, "quantize_i16_wire", V, 8 * n, lambda: ops.quantize_i16_wire_blk(x, kb, V, out=wire),
                  lambda: ops.quantize_i16_wire(x, k, out=wire))
            ops.quantize_i16_wire(x, k, out=wire)                      # the same summed wire for both decodes
            given(run, "i16_wire_finish (y + out16 + flags)", V, 10 * n + nblk,
                  lambda: ops.i16_wire_finish_blk(wire, kb, V, out16=o16, y=y, overflow=f),
                  lambda: ops.i16_wire_finish(wire, k, V, out16=o16, y=y, overflow=f))
    return rows


def run_x16_shard(dev):
    """bf16 / fp16 buckets on the sharded int16 wire (include/ina_shard_x16.h) at the ResNet-50 size, cold
    caches, median of 20, the whole set twice in this process (run 1 / run 2), as run_blk_shard.  Each of
    the four calls -- wire.quantize, wire.quantize_blk from a 16-bit bucket, wire.finish, wire.finish_blk
    into a 16-bit y (y + out16 + flags) -- beside (a) its fp32 sibling timed twice, the two times'
    difference being the spread, and (b) what a caller without the 16-bit entry points does around the
    sibling with a preallocated fp32 buffer: widen first (quantisers), or narrow afterwards (finishes).
    Bar: no slower than the sibling's slower timing plus the spread (the 16-bit call moves 6 bytes a
    value against 8, 8 + flags against 10 + flags), and faster than (b); reported, not gated."""
    from ina_amd import ops, wire
    rows = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(19)
    n, k, V = 25_557_032, 9, 256
    nblk = (n + V - 1) // V
    x = torch.randn(n, device=dev, generator=gen) * 1e-2
    wide = torch.empty(n, dtype=torch.float32, device=dev)
    w = torch.empty(n, dtype=torch.int32, device=dev)
    o16 = torch.empty(n, dtype=torch.int16, device=dev)
    y = torch.empty(n, dtype=torch.float32, device=dev)
    f = torch.empty(nblk, dtype=torch.uint8, device=dev)
    kb = ops.block_scales([x], V, bits=16, degree=64)              # the 64-rank wire's scales

    def one(run, name, dt, nb16, nbsib, f16, fsib, fround):
        ta, tb, tr, tc = _time(fsib), _time(f16), _time(fround), _time(fsib)
        lo, hi = min(ta, tc), max(ta, tc)
        bar = hi + (hi - lo)
        rows.append(_row(f"{name} {dt} [x16 shard, run {run}]", tb, nb16,
                         sibling_us=[round(ta * 1e6, 2), round(tc * 1e6, 2)], sibling_bytes=int(nbsib),
                         sibling_spread_us=round((hi - lo) * 1e6, 2), bar_us=round(bar * 1e6, 2),
                         bar_met=bool(tb <= bar), roundabout_us=round(tr * 1e6, 2), beats_roundabout=bool(tb < tr)))

    for run in (1, 2):
        for dt in (torch.bfloat16, torch.float16):
            name = "bf16" if dt == torch.bfloat16 else "fp16"
            x16 = x.to(dt)
            y16 = torch.empty(n, dtype=dt, device=dev)

            def widen_then(q):
                wide.copy_(x16)
                q(wide)

            one(run, "quantize_i16_wire", name, 6 * n, 8 * n, lambda: wire.quantize(x16, k, out=w),
                lambda: ops.quantize_i16_wire(x, k, out=w),
                lambda: widen_then(lambda t: ops.quantize_i16_wire(t, k, out=w)))
            one(run, f"quantize_i16_wire_blk V={V}", name, 6 * n + nblk, 8 * n + nblk,
                lambda: wire.quantize_blk(x16, kb, V, out=w), lambda: ops.quantize_i16_wire_blk(x, kb, V, out=w),
                lambda: widen_then(lambda t: ops.quantize_i16_wire_blk(t, kb, V, out=w)))
            ops.quantize_i16_wire(x, k, out=w)                     # the same summed wire for every decode

            def then_narrow(fin):
                fin()
                y16.copy_(y)

            one(run, "i16_wire_finish (y + out16 + flags)", name, 8 * n + nblk, 10 * n + nblk,
                lambda: wire.finish(w, k, V, out16=o16, y=y16, overflow=f),
                lambda: ops.i16_wire_finish(w, k, V, out16=o16, y=y, overflow=f),
                lambda: then_narrow(lambda: ops.i16_wire_finish(w, k, V, out16=o16, y=y, overflow=f)))
            one(run, f"i16_wire_finish_blk V={V} (y + out16 + flags)", name, 8 * n + 2 * nblk, 10 * n + 2 * nblk,
                lambda: wire.finish_blk(w, kb, V, out16=o16, y=y16, overflow=f),
                lambda: ops.i16_wire_finish_blk(w, kb, V, out16=o16, y=y, overflow=f),
                lambda: then_narrow(lambda: ops.i16_wire_finish_blk(w, kb, V, out16=o16, y=y, overflow=f)))
            del x16, y16
    return rows


def _sweep(ops, rows, sweeps, name, knob, values, fn, nbytes):
    """Time fn at each grid cap of one knob; keep all points, restore the default.  The grid-cap
    knobs exist in lab builds only (make EXTRA=-DINA_LAB_KEYS=1): the product library refuses
    them, and then only the default geometry is timed."""
    try:
        ops.set_tuning(**{knob: DEFAULTS[knob]})
    except RuntimeError:
        rows.append(_row(name, _time(fn), nbytes, note=f"default geometry ({knob}: lab builds only)"))
        return
    best = None
    for v in values:
        ops.set_tuning(**{knob: v})
        r = _row(name, _time(fn), nbytes, **{knob: v})
        sweeps.append(r)
        best = r if best is None or r["GB/s"] > best["GB/s"] else best
    ops.set_tuning(**{knob: DEFAULTS[knob]})
    r = _row(name, _time(fn), nbytes, note=f"default {knob}={DEFAULTS[knob]}")
    r["best_of_sweep"] = {knob: best[knob], "GB/s": best["GB/s"]}
    rows.append(r)


def run_extra(dev):
    from ina_amd import ops
    rows = []
    gsweep = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def rnd_i32(n):
        return torch.randint(-(1 << 20), 1 << 20, (n,), dtype=torch.int32, device=dev, generator=gen)

    def rnd_f32(n, scale=1e-2):
        return torch.randn(n, device=dev, generator=gen) * scale

    # --- sum-reduce tuning sweep, config 3 ---------------------------------------------
    n3, W3 = 26_214_400, 8
    b3 = [rnd_i32(n3) for _ in range(W3)]
    o3 = torch.empty(n3, dtype=torch.int32, device=dev)
    sweep = []
    for nt in (True, False):
        for unroll in (1, 2, 4):
            for blocks in (256, 512, 1024, 2048):
                ops.set_tuning(reduce_blocks=blocks, unroll=unroll, nontemporal=nt)
                t = _time(lambda: ops.sum_reduce(b3, out=o3))
                sweep.append(_row("sum_reduce_i32 W=8", t, (W3 + 1) * n3 * 4, nt=nt, unroll=unroll,
                                  max_blocks=blocks))
    ops.set_tuning(reduce_blocks=0, unroll=0, nontemporal=True)   # back to the automatic geometry
    rows.append(max(sweep, key=lambda r: r["GB/s"]) | {"note": "best of sweep"})
    for W in (2, 4, 16):
        bw = [rnd_i32(n3) for _ in range(W)] if W != 16 else b3 + [rnd_i32(n3) for _ in range(8)]
        t = _time(lambda: ops.sum_reduce(bw, out=o3))
        rows.append(_row(f"sum_reduce_i32 W={W}", t, (W + 1) * n3 * 4))
        del bw

    # --- quantise / dequantise ------------------------------------------------------------
    x = rnd_f32(n3)
    q = torch.empty(n3, dtype=torch.int32, device=dev)
    _sweep(ops, rows, gsweep, "quantize_f32_i32", "ew_blocks", (2048, 8192, 65536),
           lambda: ops.quantize(x, 16, out=q), 8 * n3)
    y = torch.empty(n3, dtype=torch.float32, device=dev)
    _sweep(ops, rows, gsweep, "dequantize_i32_f32", "ew_blocks", (2048, 8192, 65536),
           lambda: ops.dequantize(q, 16, out=y), 8 * n3)
    del x, q, y

    # --- config 5, one rank: a 1 GiB fp32 bucket through both wires' device steps ----------
    n5 = 268_435_456
    x5 = rnd_f32(n5)
    w5 = torch.empty(n5, dtype=torch.int32, device=dev)
    y5 = torch.empty(n5, dtype=torch.float32, device=dev)
    f5 = torch.empty(n5 // 256, dtype=torch.uint8, device=dev)
    rows.append(_row("quantize_f32_i32 (C5 rank, 1 GiB)", _time(lambda: ops.quantize(x5, 16, out=w5)), 8 * n5))
    rows.append(_row("dequantize_i32_f32 (C5 rank, 1 GiB)", _time(lambda: ops.dequantize(w5, 16, out=y5)),
                     8 * n5))
    rows.append(_row("quantize_i16_wire (C5 rank, 1 GiB, int16 wire)",
                     _time(lambda: ops.quantize_i16_wire(x5, 20, out=w5)), 8 * n5))
    rows.append(_row("i16_wire_finish (C5 rank, 1 GiB: saturate once, dequantise, slot flags)",
                     _time(lambda: ops.i16_wire_finish(w5, 20, 256, y=y5, overflow=f5, want_out16=False)),
                     8 * n5 + f5.numel()))
    del x5, w5, y5, f5

    # --- config 2: fused quantise + reduce, 4 x ResNet-50 fp32 -----------------------------
    n2 = 25_557_032
    b2 = [rnd_f32(n2) for _ in range(4)]
    o2 = torch.empty(n2, dtype=torch.int32, device=dev)
    _sweep(ops, rows, gsweep, "quantize_reduce_f32_i32 W=4 (C2)", "stream_blocks",
           (512, 2048, 8192), lambda: ops.quantize_reduce(b2, 16, out=o2), (4 * 4 + 4) * n2)
    # --- config 4: int16 saturating, 16 workers --------------------------------------------
    b4 = b2 + [rnd_f32(n2) for _ in range(12)]
    o4 = torch.empty(n2, dtype=torch.int16, device=dev)
    f4 = torch.empty((n2 + 255) // 256, dtype=torch.uint8, device=dev)
    _sweep(ops, rows, gsweep, "quantize_reduce_f32_i16 W=16 V=256 (C4)", "max_blocks",
           (2048, 8192, 16384, 32768),
           lambda: ops.quantize_reduce_i16(b4, 13, 256, out=o4, overflow=f4),
           (16 * 4 + 2) * n2 + f4.numel())
    # the C4 worker's own quantiser and the PS's dequantise of the int16 aggregate
    q4 = torch.empty(n2, dtype=torch.int16, device=dev)
    rows.append(_row("quantize_f32_i16_sat V=256 (C4 worker)",
                     _time(lambda: ops.quantize_i16(b4[0], 13, 256, out=q4, overflow=f4)),
                     6 * n2 + f4.numel()))
    y4 = torch.empty(n2, dtype=torch.float32, device=dev)
    rows.append(_row("dequantize_i16_f32 (C4 aggregate)", _time(lambda: ops.dequantize(o4, 13, out=y4)),
                     6 * n2))
    del q4, y4
    # --- PS combine (launch.py:42-52), W=4 ---------------------------------------------------
    local = rnd_f32(n2, 1.0)
    oc = torch.empty_like(local)
    _sweep(ops, rows, gsweep, "ps_combine_f32 W=4", "combine_blocks", (256, 512, 1024, 2048),
           lambda: ops.ps_combine(local, b2[:4], 0.2, out=oc), (4 + 2) * 4 * n2)
    from ina_amd import ps as ps_mod
    _sweep(ops, rows, gsweep, "ps_combine_ina_f32 W=4", "combine_ina_blocks", (256, 512, 2048, 8192),
           lambda: ps_mod.combine_ina(local, b2[:4], 16, 0.2, out=oc), (4 + 2) * 4 * n2)
    del b4, b2, local, oc, o4

    # --- packets, V = 256 over the C3 aggregate ------------------------------------------------
    V = 256
    stride = ops.nga_stride(V)
    npk = (n3 + V - 1) // V
    pk = torch.empty((npk, stride), dtype=torch.uint8, device=dev)
    grids = (1024, 2048, 8192, 16384, 32768)
    _sweep(ops, rows, gsweep, "pack_nga V=256", "stream_blocks", grids,
           lambda: ops.pack_nga(o3, V, 1, 8, 1, 1, out=pk), 4 * n3 + npk * stride)
    _sweep(ops, rows, gsweep, "unpack_nga V=256", "stream_blocks", grids,
           lambda: ops.unpack_nga(pk, V), npk * stride + 4 * n3 + npk * 15)
    # worker side, fused: NGA-256 packets of quantise(p_w - p_global) for a ResNet-50 bucket
    nr = 25_557_032
    xr, br = rnd_f32(nr), rnd_f32(nr)
    npr = (nr + V - 1) // V
    pr = torch.empty((npr, stride), dtype=torch.uint8, device=dev)
    _sweep(ops, rows, gsweep, "quantize_pack_nga V=256 ResNet-50 delta (worker side, fused)",
           "stream_blocks", grids, lambda: ops.quantize_pack_nga(xr, 16, V, 1, 8, 1, 1, base=br, out=pr),
           8 * nr + npr * stride)
    rows.append(_row("absmax_f32 ResNet-50 delta (dynamic scale)", _time(lambda: ops.absmax(xr, br)), 8 * nr))
    del xr, br, pr
    npc = 199_665   # ResNet-50 in C-128 packets (communicator.py:10)
    g = rnd_i32(npc * 128)
    pc = torch.empty((npc, 524), dtype=torch.uint8, device=dev)
    rows.append(_row("pack_c128 ResNet-50", _time(lambda: ops.pack_c128(g, npc, 1, 0, 0, out=pc)),
                     npc * (512 + 524)))

    # --- packet-stream switch: 8 workers x 100 MiB as NGA-256 packets ------------------------
    Ws = 8
    packed = [ops.pack_nga(b3[w], V, w + 1, Ws, 1, 1, num_slots=1 << 17, desc=True) for w in range(Ws)]
    stream = torch.cat([p for p, _ in packed])
    desc_all = torch.cat([d for _, d in packed])      # the pack kernels' packet descriptors
    del packed
    sw = ops.Switch(V, num_slots=1 << 17, switch_id=1, device=dev)
    acts = torch.empty(stream.shape[0], dtype=torch.uint8, device=dev)

    # replaying the same stream repeats the same work: every slot completes (count back to
    # 0) and keeps its frag id, so no state reset sits inside the timed region
    # algorithmic bytes: every packet read once, the forwarded (completing) 1/Ws of them
    # written back, each touched slot's V registers, count and frag written once (a slot's
    # registers are read only when a packet adds to a stored value -- never here, every
    # slot starts with count_reg == 1), one action byte per packet
    npk_all = stream.shape[0]
    sw_bytes = stream.numel() + stream.numel() // Ws + npk * (V * 4 + 5) + npk_all
    rows.append(_row("switch_process 8x NGA-256 (819,200 pkts, incl. slot sort; keys from descriptors)",
                     _time(lambda: sw.process(stream, acts, desc=desc_all), reps=5, warm=1), sw_bytes,
                     note="the pack kernels' 8-byte packet descriptors feed the slot sort "
                          "(ina_switch (descriptors))"))
    rows.append(_row("switch_process 8x NGA-256 (819,200 pkts, incl. slot sort; keys from headers)",
                     _time(lambda: sw.process(stream, acts), reps=5, warm=1), sw_bytes,
                     note="ina_switch_process: the key pass reads each packet's header line"))
    # the same packets in other arrival orders (the sort is order-independent; the run
    # kernel's gather follows the packets' places in the batch): round-robin over the
    # workers as a NIC interleaves them (a slot's W packets adjacent), and a random order
    for name, perm in (("round-robin over workers",
                        torch.arange(npk_all, device=dev).view(Ws, npk).t().reshape(-1)),
                       ("random", torch.randperm(npk_all, device=dev,
                                                 generator=torch.Generator(device=dev).manual_seed(9)))):
        st_p, ds_p = stream[perm], desc_all[perm]
        rows.append(_row(f"switch_process 8x NGA-256 (819,200 pkts, incl. slot sort; {name} arrival)",
                         _time(lambda: sw.process(st_p, acts, desc=ds_p), reps=5, warm=1), sw_bytes,
                         note="keys from descriptors; same packets, arrival order permuted"))
        del st_p, ds_p
    # PS side, fused, on the switch's output: completed slots -> dequantise -> update + acks
    sw.process(stream, acts)
    local3 = rnd_f32(n3)
    out3 = torch.empty_like(local3)
    acks = torch.empty((npk, stream.shape[1]), dtype=torch.uint8, device=dev)
    rows.append(_row("apply_completed_nga V=256 (PS side, fused; 102,400 completed of 819,200)",
                     _time(lambda: ops.apply_completed(stream, acts, V, 1, local3, 16, 0.1, out=out3,
                                                       acks=acks)),
                     npk_all + npk * stream.shape[1] + 8 * n3 + 16 * npk))   # ack rows: 16-B headers
    del local3, out3, acks

    # the whole INA packet path on one GPU, one step: 8 workers quantise+packetise their
    # deltas (p_w - p_global) into one arrival stream, the switch aggregates it, the PS
    # applies the completed slots and its acks go back through the switch to free them
    xs = [rnd_f32(n3) for _ in range(Ws)]
    glob_p = rnd_f32(n3)
    upd = torch.empty_like(glob_p)
    acks = torch.empty((npk, stream.shape[1]), dtype=torch.uint8, device=dev)
    ack_acts = torch.empty(npk, dtype=torch.uint8, device=dev)
    rows_w = stream.view(Ws, npk, stream.shape[1])

    desc_w = desc_all.view(Ws, npk)

    def ina_step():
        for w in range(Ws):
            ops.quantize_pack_nga(xs[w], 16, V, w + 1, Ws, 1, 1, base=glob_p, num_slots=1 << 17,
                                  out=rows_w[w], desc=desc_w[w])
        sw.process(stream, acts, desc=desc_all)
        ops.apply_completed(stream, acts, V, 1, glob_p, 16, 1.0 / (Ws + 1), out=upd, acks=acks)
        sw.process(acks, ack_acts)
    t = _time(ina_step, reps=5, warm=1)
    ina_step()
    torch.cuda.synchronize()
    ok = bool((acts == 1).sum() == npk) and bool((ack_acts == 3).all()) and not bool(sw.frag.any())
    row_b = stream.shape[1]
    path_bytes = (Ws * (8 * n3 + npk * row_b)                                   # fused worker packs
                  + stream.numel() + npk * row_b + npk * (V * 4 + 5) + npk_all  # switch
                  + npk_all + npk * row_b + 8 * n3 + 16 * npk                   # PS apply + acks
                  + npk * row_b + npk * 6)                                       # acks through the switch
    rows.append(_row("INA packet path step: 8 x quantise+pack -> switch -> apply -> acks (8 x 100 MiB fp32)",
                     t, path_bytes, aggregated_GBps=round(Ws * n3 * 4 / t / 1e9, 2), slots_freed=ok,
                     note="bytes = the sum of the four stages' algorithmic HBM bytes (so frac is the "
                          "path's roofline fraction); aggregated_GBps = worker fp32 bytes aggregated "
                          "per second through the packet path"))
    del acks, ack_acts, rows_w, stream, desc_w, desc_all

    # steady state: the PS's acks for step t reach the switch in the same batch as the
    # workers' packets for step t+1, in front of them (the ack frees the slot before the
    # slot's next packets claim it -- arrival order is what the slot sort keeps)
    big = torch.zeros(((Ws + 1) * npk, row_b), dtype=torch.uint8, device=dev)   # [acks | 8 workers]
    ack_rows, rows_w2 = big[:npk], big[npk:].view(Ws, npk, row_b)
    acts2 = torch.empty((Ws + 1) * npk, dtype=torch.uint8, device=dev)
    sw2 = ops.Switch(V, num_slots=1 << 17, switch_id=1, device=dev)
    desc_big = torch.empty((Ws + 1) * npk, dtype=torch.int64, device=dev)   # [acks | 8 workers]
    desc_ack, desc_w2 = desc_big[:npk], desc_big[npk:].view(Ws, npk)

    def ina_step_steady():
        for w in range(Ws):
            ops.quantize_pack_nga(xs[w], 16, V, w + 1, Ws, 1, 1, base=glob_p, num_slots=1 << 17,
                                  out=rows_w2[w], desc=desc_w2[w])
        ops.nga_descriptors(ack_rows, out=desc_ack)          # the PS's ack rows
        sw2.process(big, acts2, desc=desc_big)
        ops.apply_completed(big, acts2, V, 1, glob_p, 16, 1.0 / (Ws + 1), out=upd, acks=ack_rows)
    ina_step_steady()                      # first step: the ack rows are zero (another switch's)
    t = _time(ina_step_steady, reps=5, warm=1)
    ina_step_steady()
    torch.cuda.synchronize()
    ok = bool((acts2[npk:] == 1).sum() == npk) and bool((acts2[:npk] == 3).all())
    rows.append(_row("INA packet path step, steady state: step t's acks ride in front of step t+1's packets",
                     t, path_bytes - npk * 6, aggregated_GBps=round(Ws * n3 * 4 / t / 1e9, 2),
                     acks_and_slots_ok=ok,
                     note="one switch batch per step: (W+1) x 102,400 packets; bytes as the row above"))
    # the same with the PS on the switch's GPU: ina_switch with a PS step takes each completed
    # slot's sum from the switch's registers straight into the update and the ack row (the
    # completed packets are consumed, not written back)
    big.zero_()
    sw3 = ops.Switch(V, num_slots=1 << 17, switch_id=1, device=dev)

    def ina_step_fused():
        for w in range(Ws):
            ops.quantize_pack_nga(xs[w], 16, V, w + 1, Ws, 1, 1, base=glob_p, num_slots=1 << 17,
                                  out=rows_w2[w], desc=desc_w2[w])
        ops.nga_descriptors(ack_rows, out=desc_ack)
        sw3.process_apply(big, 1, glob_p, 16, 1.0 / (Ws + 1), out=upd, acks=ack_rows,
                          keep_forwarded=False, actions=acts2, desc=desc_big)
    ina_step_fused()
    t = _time(ina_step_fused, reps=5, warm=1)
    ina_step_fused()
    torch.cuda.synchronize()
    ok = bool((acts2[npk:] == 1).sum() == npk) and bool((acts2[:npk] == 3).all())
    fused_bytes = path_bytes - npk * 6 - (npk_all + npk * row_b) - npk * row_b  # no apply re-read, no fwd write
    rows.append(_row("INA packet path step, steady state, PS fused into the switch pass",
                     t, fused_bytes, aggregated_GBps=round(Ws * n3 * 4 / t / 1e9, 2),
                     acks_and_slots_ok=ok,
                     note="ina_switch with a PS step(keep_forwarded=0): bytes = the steady-state row's "
                          "minus the PS's re-read of completed packets and their write-back"))
    # the same with the 8 worker packs as ONE launch (ina_quantize_pack_nga_multi: the
    # shared base is read once for the 8 workers) -- bench.py's packet_path leg
    outs_w2, descs_w2 = list(rows_w2.unbind(0)), list(desc_w2.unbind(0))

    def ina_step_fused_multi():
        ops.quantize_pack_nga_multi(xs, 16, V, [w + 1 for w in range(Ws)], Ws, 1, 1, base=glob_p,
                                    num_slots=1 << 17, outs=outs_w2, descs=descs_w2)
        ops.nga_descriptors(ack_rows, out=desc_ack)
        sw3.process_apply(big, 1, glob_p, 16, 1.0 / (Ws + 1), out=upd, acks=ack_rows,
                          keep_forwarded=False, actions=acts2, desc=desc_big)
    ina_step_fused_multi()
    t = _time(ina_step_fused_multi, reps=5, warm=1)
    ina_step_fused_multi()
    torch.cuda.synchronize()
    ok = bool((acts2[npk:] == 1).sum() == npk) and bool((acts2[:npk] == 3).all())
    rows.append(_row("INA packet path step, steady state, PS fused, the 8 worker packs in one launch",
                     t, fused_bytes - (Ws - 1) * n3 * 4, aggregated_GBps=round(Ws * n3 * 4 / t / 1e9, 2),
                     acks_and_slots_ok=ok,
                     note="ina_quantize_pack_nga_multi + ina_switch with a PS step; bytes = the row above "
                          "with the shared base read once"))
    # the same step recorded once as a hipGraph and replayed: the step's 15 launches (8
    # worker packs, the descriptor pass, the switch's 5 sort/run launches, ...) leave the
    # CPU and the launch queue
    try:
        cap = torch.cuda.Stream(dev)
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            ina_step_fused()
        torch.cuda.current_stream().wait_stream(cap)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ina_step_fused()
        t = _time(graph.replay, reps=5, warm=1)
        graph.replay()
        torch.cuda.synchronize()
        ok = bool((acts2[npk:] == 1).sum() == npk) and bool((acts2[:npk] == 3).all())
        rows.append(_row("INA packet path step, steady state, PS fused, replayed as a hipGraph",
                         t, fused_bytes, aggregated_GBps=round(Ws * n3 * 4 / t / 1e9, 2),
                         acks_and_slots_ok=ok, note="torch.cuda.CUDAGraph capture of the row above"))
        del graph
    except Exception as e:                       # reported, not fatal: the eager row stands
        rows.append({"kernel": "INA packet path step, steady state, PS fused, replayed as a hipGraph",
                     "error": repr(e)[:300]})
    del xs, glob_p, upd, big, ack_rows, rows_w2, acts2, sw2, sw3, desc_big, desc_ack, desc_w2

    # small batches through the switch (P4 format: NGA-32, 16,384-slot pool): latency of
    # one ina_switch_process call, the stand-in's per-batch cost when packets arrive in
    # recvmmsg-sized batches
    for nb in (64, 1024, 16384):
        sw32 = ops.Switch(32, num_slots=16384, switch_id=1, device=dev)
        small = torch.cat([ops.pack_nga(rnd_i32(32 * nb // 8), 32, w + 1, 8, 1, 1) for w in range(8)])
        a32 = torch.empty(small.shape[0], dtype=torch.uint8, device=dev)
        rows.append(_row(f"switch_process small batch: {small.shape[0]} NGA-32 packets",
                         _time(lambda: sw32.process(small, a32), reps=20, warm=3),
                         small.numel(), note="latency row; bytes = packet bytes read"))
        del sw32, small, a32

    # --- end to end: pinned host -> HBM -> reduce -> pinned host -------------------------------
    hosts = [b.cpu().pin_memory() for b in b3]
    hout = torch.empty(n3, dtype=torch.int32).pin_memory()
    dbuf = [torch.empty(n3, dtype=torch.int32, device=dev) for _ in range(W3)]

    def e2e():
        for h, d in zip(hosts, dbuf):
            d.copy_(h, non_blocking=True)
        ops.sum_reduce(dbuf, out=o3)
        hout.copy_(o3, non_blocking=True)
    t = _time(e2e, reps=5, warm=1)
    rows.append(_row("end-to-end pinned H2D(8x100MiB)+reduce+D2H", t, (W3 + 1) * n3 * 4,
                     aggregated_GBps=round(W3 * n3 * 4 / t / 1e9, 2), note="one stream, phases in sequence"))
    # the product path (ina_sum_reduce_host_i32): zero copy for pinned buffers (the default),
    # then the chunked H2D / reduce / D2H copy pipeline (zero copy off) over its knobs
    want = hout.clone()
    hz = torch.empty(n3, dtype=torch.int32).pin_memory()
    zscratch = torch.empty(ops.load().ina_host_reduce_scratch_bytes(W3, 0), dtype=torch.uint8, device=dev)
    t = _time(lambda: ops.sum_reduce_host(hosts, out=hz, scratch=zscratch), reps=5, warm=1)
    rows.append(_row("end-to-end host reduce, zero copy (pinned buckets read over PCIe in place)", t,
                     (W3 + 1) * n3 * 4, aggregated_GBps=round(W3 * n3 * 4 / t / 1e9, 2),
                     matches=bool(torch.equal(hz, want))))
    del hz, zscratch
    ops.set_tuning(host_zero_copy=False)
    for h2d in (1, 2):
        for chunk in (1 << 18, 1 << 20, 1 << 22):
            ops.set_tuning(h2d_streams=h2d)
            scratch = torch.empty(ops.load().ina_host_reduce_scratch_bytes(W3, chunk),
                                  dtype=torch.uint8, device=dev)
            hp = torch.empty(n3, dtype=torch.int32).pin_memory()

            def piped():
                ops.sum_reduce_host(hosts, out=hp, chunk=chunk, scratch=scratch)
            t = _time(piped, reps=5, warm=1)
            rows.append(_row(f"end-to-end host reduce, copy pipeline (h2d streams {h2d}, chunk {chunk})", t,
                             (W3 + 1) * n3 * 4, aggregated_GBps=round(W3 * n3 * 4 / t / 1e9, 2),
                             matches=bool(torch.equal(hp, want))))
            del scratch
    ops.set_tuning(host_zero_copy=True)
    ops.set_tuning(h2d_streams=2)
    del hosts, hout, dbuf, b3, o3
    rows += run_x16(dev)
    rows += run_blk(dev)
    rows += run_ef(dev)
    rows += run_ef_shard(dev)
    rows += run_sr(dev)
    rows += run_sr_packets(dev)
    rows += run_sr_reduce(dev)
    rows += run_blk_sr(dev)
    rows += run_blk_x16(dev)
    rows += run_blk_packets(dev)
    rows += run_blk_switch(dev)
    rows += run_blk_shard(dev)
    rows += run_x16_shard(dev)
    return {"rows": rows, "sweep": sweep, "grid_sweeps": gsweep}
