"""Shared pieces of tests/test_gpu_graph_bulk.py: the table of bulk entry points and the two ways each
row is run -- behind a device-side delay on a side stream, and as a hipGraph replayed on fresh inputs.

A row names the `_lib` prototypes its call reaches (checked against what the call really looks up in the
library), makes its inputs for a phase, calls the wrapper with caller-supplied outputs, and gives the
expected outputs from the numpy / oracle yardsticks of the suite -- never from a run of the code under
test.  Phases: 1 raises flags and a large maximum (a saturating block, a NaN), 2 is calm (all-zero flags,
a smaller maximum), 3 is mixed.  Every device buffer is a view into a larger allocation filled with a
sentinel byte; the bytes around the view must survive, and a view that starts 2 or 4 bytes past a
16-byte boundary sends the call down its value-by-value path, the one that clears its flags with a
launch of its own in front of the kernel.

The stream-order window.  The side stream first runs torch.cuda._sleep for DELAY_MS, then the copy of
the fresh inputs, the call, the copy-out; an event recorded after the sleep must still be pending when
the call has returned, or the case is void and fails.  Measured on an MI355X (the figure every case
prints: the host clock around the copies and the call of a warmed row): 0.022-0.066 ms for the rows of one
to three buffers, up to 0.145 ms for the rows of 17 buckets or slices (18 copies; 0.086-0.106 ms in the run
that first held the rows of the newer wires), and the slowest i4_sum_requant_w33 (34 copies) at 0.149 ms =
HOST_ENQUEUE_MS_MEASURED.  Ten times that is 1.49 ms; DELAY_MS = 5 ms is that rounded up past one 4 ms
scheduler tick of the host, so that a thread put off once between two enqueues does not void the case.
"""
import contextlib

import numpy as np
import torch

from oracle import oracle as orc
from tests import _blk_ref as bref
from tests import _blk_sr_ref as bsref
from tests import _ef_ref as eref
from tests import _i4_ref as i4ref
from tests import _i8_ef_ref as i8eref
from tests import _i8_ref as i8ref
from tests import _i8_sr_ref as i8sref
from tests import _rot_ref as rref
from tests import _shard_blk_ref as shref
from tests import _sr_ref as sref
from tests import _sr_reduce_ref as srref

DEV = "cuda:0"
F32 = np.float32
V, NBLK = 32, 37
N_BLK, N_RAG = NBLK * V, NBLK * V + 5          # whole blocks; ragged where the entry point allows it
K = 8                                           # the global scale: int16 saturates from |x| = 128
SEED, STEP = 0x5EED1234ABCD, 9
SENTINEL = 0xA5
GUARD = 64                                      # bytes in front of and behind every view
HOST_ENQUEUE_MS_MEASURED = 0.149                # slowest row (33 nibble slices: 34 copies + the call)
DELAY_MS = 5.0


def mods():
    from ina_amd import blk_sr, ef, i4, i8, ops, rot, sr
    return {"o": ops, "ef": ef, "i4": i4, "i8": i8, "rot": rot, "sr": sr, "bsr": blk_sr}


# ---- inputs --------------------------------------------------------------------------------------
def grads(rng, phase, W, n, dtype=torch.float32):
    """W buckets of n values, |x| about 1/4: phase 1 with a block of thousands (saturates at 2^K) and a
    NaN, phase 3 with another block and another NaN, phase 2 neither."""
    x = (rng.standard_normal((W, n)) * 0.25).astype(F32)
    if phase in (1, 3):
        sat, nan, f = (3, 5, 4000.0) if phase == 1 else (7, 11, 1000.0)
        x[:, sat * V:(sat + 1) * V] *= F32(f)
        x[W // 2, nan * V + 2] = np.nan
    return [torch.from_numpy(x[w]).to(dtype) for w in range(W)]


def scales(n, lo=7):
    return torch.from_numpy((lo + np.arange(-(-n // V)) % 3).astype(np.int8))


def wide(t):
    """A host tensor (or a list or dict of them) as numpy; 16-bit floats widened exactly to float32."""
    if isinstance(t, dict):
        return {k: wide(x) for k, x in t.items()}
    if isinstance(t, (list, tuple)):
        return [wide(x) for x in t]
    return (t.float() if t.dtype in (torch.bfloat16, torch.float16) else t).numpy()


def absmax_ref(xs, base=None):
    with np.errstate(all="ignore"):
        d = [np.abs(x if base is None else (x - base).astype(F32)) for x in xs]
    return np.array([np.fmax.reduce(np.concatenate(d), initial=F32(0))], F32)         # NaN ignored


class Row:
    """One entry point.  ins(rng, phase) -> {name: host tensor or list}; outs: {name: (torch dtype, numel)};
    call(m, t, step) with t the device tensors by name; want(h, step) -> {name: numpy} from the widened
    host inputs h.  mis: names whose view starts off a 16-byte boundary; state: inputs the call updates
    in place (they carry over from replay to replay and are compared); flags / peak: the output that
    must go down in phase 2; keyed: the call draws random numbers under (SEED, step).  odd: names whose view
    starts one byte past a 16-byte boundary (the shift bytes of a requantiser); shifts: the output of block shifts
    that must hold a non-zero in phase 1 and none in phase 2, as flags must; key_phase: the phase whose inputs the
    key test replays (a stochastic requantiser draws nothing where every shift is 0, so it takes phase 1)."""

    def __init__(self, name, protos, ins, outs, call, want, mis=(), state=(), flags=None, peak=None, cap=False,
                 keyed=False, src=None, odd=(), shifts=None, key_phase=2):
        self.name, self.protos, self.ins, self.outs, self.call, self.want = name, tuple(protos), ins, outs, call, want
        self.mis, self.state, self.flags, self.peak, self.cap, self.keyed = set(mis), tuple(state), flags, peak, cap, keyed
        self.src, self.odd, self.shifts, self.key_phase = src, set(odd), shifts, key_phase

    def __repr__(self):
        return self.name


I16, I32, I8, U8, FP = torch.int16, torch.int32, torch.int8, torch.uint8, torch.float32
NB = NBLK + 1                                   # blocks of a ragged bucket


def _wire_sum(rng, phase, kb=None):
    """The int32 sum of three ranks' wire words (the oracle's quantiser), as the collective delivers it."""
    xs = wide(grads(rng, phase, 3, N_RAG))
    ws = [orc.quantize_i16_wire(x, K) if kb is None else shref.wire_ref(x, kb, V) for x in xs]
    return torch.from_numpy(np.sum(np.stack(ws).astype(np.int64), axis=0).astype(np.int32))


def _ints16(rng, phase, W, n):
    amp = 20000 if phase == 1 else 5000
    a = rng.integers(-amp, amp, (W, n)).astype(np.int16)
    if phase == 3:
        a[:, 7 * V:8 * V] = 30000
    return [torch.from_numpy(a[w]) for w in range(W)]


SAT = {1: 3, 3: 7}                              # the block grads() saturates in phases 1 and 3
N_I4 = N_BLK + 24                               # the exact nibble sum: whole chunks of 32 and a ragged lane of 3 dwords
RND = dict(sub=65, e0=16 * 1_000_003)           # the rounding stream of the stochastic requantiser


def _ef_scales(phase):
    """Given scales of the byte wire's error-feedback row.  A block that clamps leaves the clipped part in the
    residual, thousands here, and the next replay adds it in front of the rotation: so SAT's blocks sit at k = -8
    (a quantum of 256, nothing of theirs clamps: |r| <= 32 * 5000 / 8 < 127 * 256) except in the phase that is to
    clamp them, k = 4.  Phase 2 then carries phase 1's residual without a flag."""
    kb = scales(N_BLK, 4).numpy().copy()
    kb[list(SAT.values())] = -8
    if phase in SAT:
        kb[SAT[phase]] = 4
    return torch.from_numpy(kb)


def _spread(xs):
    """Block b of every bucket times 2^(b / NBLK): the blocks' maxima cover an octave, so some sit at a scale's
    threshold and cross it with the rotation's signs -- the scales of STEP and STEP + 1 differ."""
    f = torch.from_numpy(np.repeat(np.exp2(np.arange(NBLK) / NBLK), V).astype(F32))
    return [(x.float() * f).to(x.dtype) for x in xs]


def _bytes(rng, phase, W, n):
    """W byte slices.  Phase 1: the full range (17 slices: shifts up to 5); phase 2: within +-7, every |sum| at
    most 7 W <= 127 up to W = 18, so every shift is 0; phase 3: the full range in every other block."""
    big = {1: np.ones(n // V, bool), 2: np.zeros(n // V, bool), 3: np.arange(n // V) % 2 == 1}[phase]
    amp = np.repeat(np.where(big, 127, 7), V)
    return [torch.from_numpy(a) for a in rng.integers(-amp, amp + 1, (W, n)).astype(np.int8)]


def _nibbles(rng, phase, W, n, amp, plants):
    """W slices of packed nibbles within +-amp; plants: {phase: {block: nibble}}, the block's value 5 is that nibble
    in every slice (|sum| = W * |nibble|) ."""
    q = rng.integers(-amp, amp + 1, (W, n))
    for b, v in plants.get(phase, {}).items():
        q[:, b * V + 5] = v
    return [torch.from_numpy(i4ref.pack(r)) for r in q]


# 17 slices: |S| <= 7 * 17 = 119, every shift is 0 whatever is planted.  33 slices within +-3 stay within 99; a
# column of 7 is 231 (shift 1), of -8 is -264 (rne(264 / 2) = 132: shift 2)
PLANTS17 = {1: {3: 7, 4: -7}, 3: {7: -7}}
PLANTS33 = {1: {3: 7, 4: -8, 36: -8}, 3: {0: -8, 7: 7}}


def _shifted(q8, sh):
    """The int16 values the requantised gather decodes: q8 << min(shift, 7)."""
    return q8.astype(np.int16) << np.repeat(np.minimum(sh, 7), V).astype(np.int16)


def rows():
    R = []
    add = lambda *a, **k: R.append(Row(*a, **k))                                    # noqa: E731
    kb_rag, kb_blk = scales(N_RAG), scales(N_BLK)

    # -- entry points that clear flags or an atomic word in front of their kernel ----------------
    add("quantize_i16", ["ina_quantize_f32_i16_sat"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0]}, {"q": (I16, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["o"].quantize_i16(t["x"], K, V, out=t["q"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("q", "ovf"), orc.quantize_i16_sat(h["x"], K, V))),
        mis=["q"], flags="ovf", cap=True, src="ina_kernels.hip")
    add("sum_reduce_i16_w3", ["ina_sum_reduce_i16_sat"],
        lambda g, p: {"b": _ints16(g, p, 3, N_RAG)}, {"out": (I16, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["o"].sum_reduce_i16(t["b"], V, out=t["out"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("out", "ovf"), orc.sum_reduce_i16_sat(h["b"], V))),
        mis=["out"], flags="ovf", src="ina_kernels.hip")
    add("quantize_reduce_i16_w3", ["ina_quantize_reduce_f32_i16_sat"],
        lambda g, p: {"b": grads(g, p, 3, N_RAG)}, {"out": (I16, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["o"].quantize_reduce_i16(t["b"], K, V, out=t["out"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("out", "ovf"), orc.quantize_reduce_i16_sat(h["b"], K, V))),
        mis=["out"], flags="ovf", src="ina_kernels.hip")
    add("absmax", ["ina_absmax_f32"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0], "base": grads(g, 2, 1, N_RAG)[0]}, {"m": (FP, 1)},
        lambda m, t, s: m["o"].absmax(t["x"], t["base"], out=t["m"]),
        lambda h, s: {"m": absmax_ref([h["x"]], h["base"])}, peak="m", src="ina_kernels.hip")
    add("absmax_multi_w3", ["ina_absmax_multi_f32"],
        lambda g, p: {"x": grads(g, p, 3, N_RAG)}, {"m": (FP, 1)},
        lambda m, t, s: m["o"].absmax_multi(t["x"], out=t["m"]),
        lambda h, s: {"m": absmax_ref(h["x"])}, peak="m", src="ina_kernels.hip")
    add("checksum", ["ina_checksum_i32"],
        lambda g, p: {"x": torch.from_numpy(g.integers(-2 ** 31, 2 ** 31, N_RAG).astype(np.int32))}, {"c": (I32, 1)},
        lambda m, t, s: m["o"].check(m["o"].load().ina_checksum_i32(
            t["x"].data_ptr(), N_RAG, t["c"].data_ptr(), torch.cuda.current_stream().cuda_stream), "checksum"),
        lambda h, s: {"c": np.array([orc.checksum_i32(h["x"])], np.uint32).view(np.int32)}, src="ina_kernels.hip")
    add("quantize_i16_f16", ["ina_quantize_x16_i16_sat"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG, torch.float16)[0]}, {"q": (I16, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["o"].quantize_i16(t["x"], K, V, out=t["q"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("q", "ovf"), orc.quantize_i16_sat(h["x"], K, V))),
        mis=["q"], flags="ovf", src="ina_x16.hip")
    add("quantize_reduce_i16_bf16_w3", ["ina_quantize_reduce_x16_i16_sat"],
        lambda g, p: {"b": grads(g, p, 3, N_RAG, torch.bfloat16)}, {"out": (I16, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["o"].quantize_reduce_i16(t["b"], K, V, out=t["out"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("out", "ovf"), orc.quantize_reduce_i16_sat(h["b"], K, V))),
        mis=["out"], flags="ovf", cap=True, src="ina_x16.hip")
    add("absmax_multi_bf16_w17", ["ina_absmax_multi_x16"],
        lambda g, p: {"x": grads(g, p, 17, N_RAG, torch.bfloat16)}, {"m": (FP, 1)},
        lambda m, t, s: m["o"].absmax_multi(t["x"], out=t["m"]),
        lambda h, s: {"m": absmax_ref(h["x"])}, peak="m", src="ina_x16.hip")
    add("absmax_f16", ["ina_absmax_multi_x16"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG, torch.float16)[0]}, {"m": (FP, 1)},
        lambda m, t, s: m["o"].absmax(t["x"], out=t["m"]),
        lambda h, s: {"m": absmax_ref([h["x"]])}, peak="m", src="ina_x16.hip")
    add("sr_quantize_i16", ["ina_quantize_sr_f32_i16_sat"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0]}, {"q": (I16, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["sr"].quantize_i16(t["x"], K, V, SEED, step=s, out=t["q"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("q", "ovf"), sref.quantize_i16(h["x"], K, V, SEED, s))),
        mis=["q"], flags="ovf", cap=True, keyed=True, src="ina_sr.hip")
    add("sr_quantize_reduce_i16_w3", ["ina_quantize_reduce_sr_f32_i16_sat"],
        lambda g, p: {"b": grads(g, p, 3, N_RAG)}, {"out": (I16, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["sr"].quantize_reduce_i16(t["b"], K, V, SEED, step=s, out=t["out"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("out", "ovf"), srref.quantize_reduce_i16(h["b"], K, V, SEED, s))),
        mis=["out"], flags="ovf", cap=True, keyed=True, src="ina_reduce_sr.hip")
    add("i16_wire_finish", ["ina_i16_wire_finish"],
        lambda g, p: {"w": _wire_sum(g, p)}, {"o16": (I16, N_RAG), "y": (FP, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["o"].i16_wire_finish(t["w"], K, V, out16=t["o16"], y=t["y"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("o16", "y", "ovf"), orc.i16_wire_finish(h["w"], K, V))),
        mis=["o16"], flags="ovf", cap=True, src="ina_shard.hip")
    add("i16_wire_finish_blk", ["ina_i16_wire_finish_blk"],
        lambda g, p: {"w": _wire_sum(g, p, kb_rag.numpy()), "kb": kb_rag},
        {"o16": (I16, N_RAG), "y": (FP, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["o"].i16_wire_finish_blk(t["w"], t["kb"], V, out16=t["o16"], y=t["y"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("o16", "y", "ovf"), shref.finish_ref(h["w"], h["kb"], V))),
        mis=["o16"], flags="ovf", src="ina_shard.hip")

    # -- single-launch entry points, two per source, one of them over W buckets (3, or 17 at run time) --
    add("quantize_i16_blk", ["ina_quantize_blk_f32_i16_sat"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0], "kb": kb_rag}, {"q": (I16, N_RAG), "ovf": (U8, NB)},
        lambda m, t, s: m["o"].quantize_i16_blk(t["x"], t["kb"], V, out=t["q"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("q", "ovf"), bref.quantize_i16(h["x"], h["kb"], V))), flags="ovf", src="ina_blk.hip")
    add("quantize_reduce_blk_w17", ["ina_quantize_reduce_blk_f32_i32"],
        lambda g, p: {"b": grads(g, p, 17, N_RAG), "kb": kb_rag}, {"out": (I32, N_RAG)},
        lambda m, t, s: m["o"].quantize_reduce_blk(t["b"], V, kblk=t["kb"], out=t["out"]),
        lambda h, s: {"out": bref.quantize_reduce_i32(h["b"], h["kb"], V)}, cap=True, src="ina_blk.hip")
    add("ef_quantize", ["ina_quantize_ef_f32_i32"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0], "r": torch.zeros(N_RAG)}, {"q": (I32, N_RAG)},
        lambda m, t, s: m["ef"].quantize(t["x"], t["r"], K, out=t["q"]),
        lambda h, s: dict(zip(("q", "r"), eref.quantize(h["x"], h["r"], K))), state=["r"], cap=True, src="ina_ef.hip")
    add("ef_block_scales_w3", ["ina_block_scales_ef_f32"],
        lambda g, p: {"x": grads(g, p, 3, N_RAG), "r": grads(g, 2, 3, N_RAG)}, {"kb": (I8, NB)},
        lambda m, t, s: m["ef"].block_scales(t["x"], t["r"], V, bits=16, degree=3, out=t["kb"]),
        lambda h, s: {"kb": eref.block_scales(h["x"], h["r"], V, 3, 16)}, src="ina_ef.hip")
    add("rot_quantize_reduce_i16_w3", ["ina_quantize_reduce_rot_i16_sat"],
        lambda g, p: {"b": grads(g, p, 3, N_BLK)}, {"out": (I16, N_BLK), "ovf": (U8, NBLK), "kb": (I8, NBLK)},
        lambda m, t, s: m["rot"].quantize_reduce_i16(t["b"], V, SEED, step=s, out=t["out"], overflow=t["ovf"],
                                                     kblk_out=t["kb"]),
        lambda h, s: dict(zip(("out", "ovf", "kb"), rref.quantize_reduce(h["b"], V, SEED, bits=16, step=s))),
        flags="ovf", cap=True, keyed=True, src="ina_rot.hip")
    add("rot_dequantize", ["ina_dequantize_rot_i32"],
        lambda g, p: {"s": torch.from_numpy(g.integers(-2 ** 20, 2 ** 20, N_BLK).astype(np.int32)), "kb": kb_blk},
        {"y": (FP, N_BLK)},
        lambda m, t, s: m["rot"].dequantize(t["s"], t["kb"], V, SEED, step=s, out=t["y"]),
        lambda h, s: {"y": rref.dequantize(h["s"], h["kb"], V, SEED, step=s)}, keyed=True, src="ina_rot.hip")
    add("i8_quantize", ["ina_quantize_i8_wire"],
        lambda g, p: {"x": grads(g, p, 1, N_BLK)[0], "kb": scales(N_BLK, 4)}, {"q": (I8, N_BLK), "ovf": (U8, NBLK)},
        lambda m, t, s: m["i8"].quantize(t["x"], t["kb"], V, rotate=SEED, step=s, out=t["q"], overflow=t["ovf"]),
        lambda h, s: dict(zip(("q", "ovf"), i8ref.quantize(h["x"], h["kb"], V, rotate=SEED, step=s))),
        flags="ovf", cap=True, keyed=True, src="ina_i8.hip")
    add("i8_sum_slices_w17", ["ina_sum_i8_slices"],
        lambda g, p: {"p": [torch.from_numpy(a) for a in g.integers(-127, 128, (17, N_RAG)).astype(np.int8)]},
        {"out": (I16, N_RAG)},
        lambda m, t, s: m["i8"].sum_slices(t["p"], out=t["out"]),
        lambda h, s: {"out": i8ref.sum_slices(h["p"])}, src="ina_i8.hip")
    add("quantize_i16_wire", ["ina_quantize_f32_i16_wire"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0]}, {"w": (I32, N_RAG)},
        lambda m, t, s: m["o"].quantize_i16_wire(t["x"], K, out=t["w"]),
        lambda h, s: {"w": orc.quantize_i16_wire(h["x"], K)}, src="ina_shard.hip")
    add("quantize_i16_wire_blk", ["ina_quantize_blk_f32_i16_wire"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0], "kb": kb_rag}, {"w": (I32, N_RAG)},
        lambda m, t, s: m["o"].quantize_i16_wire_blk(t["x"], t["kb"], V, out=t["w"]),
        lambda h, s: {"w": shref.wire_ref(h["x"], h["kb"], V)}, src="ina_shard.hip")
    add("quantize_bf16", ["ina_quantize_x16_i32"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG, torch.bfloat16)[0]}, {"q": (I32, N_RAG)},
        lambda m, t, s: m["o"].quantize(t["x"], K, out=t["q"]),
        lambda h, s: {"q": orc.quantize_i32(h["x"], K)}, src="ina_x16.hip")
    add("quantize_reduce_f16_w17", ["ina_quantize_reduce_x16_i32"],
        lambda g, p: {"b": grads(g, p, 17, N_RAG, torch.float16)}, {"out": (I32, N_RAG)},
        lambda m, t, s: m["o"].quantize_reduce(t["b"], K, out=t["out"]),
        lambda h, s: {"out": orc.quantize_reduce_i32(h["b"], K)}, src="ina_x16.hip")
    add("sr_quantize", ["ina_quantize_sr_f32_i32"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0]}, {"q": (I32, N_RAG)},
        lambda m, t, s: m["sr"].quantize(t["x"], K, SEED, step=s, out=t["q"]),
        lambda h, s: {"q": sref.quantize(h["x"], K, SEED, s)}, keyed=True, src="ina_sr.hip")
    add("blk_sr_quantize", ["ina_quantize_blk_sr_f32_i32"],
        lambda g, p: {"x": grads(g, p, 1, N_RAG)[0], "kb": kb_rag}, {"q": (I32, N_RAG)},
        lambda m, t, s: m["bsr"].quantize(t["x"], t["kb"], V, SEED, step=s, out=t["q"]),
        lambda h, s: {"q": bsref.quantize(h["x"], h["kb"], V, SEED, s)}, keyed=True, src="ina_blk.hip")

    # -- the byte wire's requantised gather, error feedback and stochastic rounding; the nibble wire --------------
    ROT = dict(rotate=SEED)
    add("i8_sum_requant_w17", ["ina_sum_i8_slices_requant"],
        lambda g, p: {"p": _bytes(g, p, 17, N_BLK)}, {"q": (I8, N_BLK), "shift": (U8, NBLK)},
        lambda m, t, s: m["i8"].sum_slices_requant(t["p"], V, out=t["q"], shift=t["shift"]),
        lambda h, s: dict(zip(("q", "shift"), i8ref.requant(h["p"], V))),
        odd=["shift"], shifts="shift", cap=True, src="ina_i8_gather.hip")
    add("i8_dequantize_gather", ["ina_dequantize_i8_gather"],
        lambda g, p: {"q8": torch.from_numpy(g.integers(-127, 128, N_BLK).astype(np.int8)),
                      "sh": torch.from_numpy(((np.arange(NBLK) + p) % 8).astype(np.uint8)), "kb": kb_blk},
        {"y": (FP, N_BLK)},
        lambda m, t, s: m["i8"].dequantize_gather(t["q8"], t["sh"], t["kb"], V, step=s, out=t["y"], **ROT),
        lambda h, s: {"y": i8ref.dequantize(_shifted(h["q8"], h["sh"]), h["kb"], V, step=s, **ROT)},
        odd=["sh"], keyed=True, src="ina_i8_gather.hip")
    add("i8_ef_block_scales_w3", ["ina_block_scales_i8_ef"],
        lambda g, p: {"x": _spread(grads(g, p, 3, N_BLK)), "r": grads(g, 2, 3, N_BLK)}, {"kb": (I8, NBLK)},
        lambda m, t, s: m["i8"].block_scales_ef(t["x"], t["r"], V, step=s, out=t["kb"], **ROT),
        lambda h, s: {"kb": i8eref.block_scales(h["x"], h["r"], V, step=s, **ROT)},
        odd=["kb"], keyed=True, src="ina_i8_ef.hip")
    add("i8_ef_quantize", ["ina_quantize_ef_i8_wire"],
        lambda g, p: {"x": grads(g, p, 1, N_BLK)[0], "r": torch.zeros(N_BLK), "kb": _ef_scales(p)},
        {"q": (I8, N_BLK), "ovf": (U8, NBLK)},
        lambda m, t, s: m["i8"].quantize_ef(t["x"], t["r"], t["kb"], V, step=s, out=t["q"], overflow=t["ovf"], **ROT),
        lambda h, s: dict(zip(("q", "ovf", "r"), i8eref.quantize(h["x"], h["r"], h["kb"], V, step=s, **ROT))),
        odd=["ovf"], state=["r"], flags="ovf", cap=True, keyed=True, src="ina_i8_ef.hip")
    add("i8_sr_block_scales_w3", ["ina_block_scales_i8_sr"],
        lambda g, p: {"x": _spread(grads(g, p, 3, N_BLK))}, {"kb": (I8, NBLK)},
        lambda m, t, s: m["i8"].block_scales_sr(t["x"], V, step=s, sub=1, out=t["kb"], **ROT),
        lambda h, s: {"kb": i8sref.block_scales(h["x"], V, step=s, sub=1, **ROT)},
        odd=["kb"], keyed=True, src="ina_i8_sr.hip")
    add("i8_sr_quantize", ["ina_quantize_sr_i8_wire"],                   # rounding stream sub 3, rotation sub 1
        lambda g, p: {"x": grads(g, p, 1, N_BLK)[0], "kb": scales(N_BLK, 4)}, {"q": (I8, N_BLK), "ovf": (U8, NBLK)},
        lambda m, t, s: m["i8"].quantize_sr(t["x"], t["kb"], V, SEED ^ 5, step=s, sub=3, rot_sub=1, out=t["q"],
                                            overflow=t["ovf"], **ROT),
        lambda h, s: dict(zip(("q", "ovf"), i8sref.quantize(h["x"], h["kb"], V, SEED ^ 5, step=s, sub=3, rot_sub=1, **ROT))),
        odd=["ovf"], flags="ovf", cap=True, keyed=True, src="ina_i8_sr.hip")
    add("i8_sum_requant_sr_w17", ["ina_sum_i8_slices_requant_sr"],
        lambda g, p: {"p": _bytes(g, p, 17, N_BLK)}, {"q": (I8, N_BLK), "shift": (U8, NBLK)},
        lambda m, t, s: m["i8"].sum_slices_requant_sr(t["p"], V, SEED, step=s, out=t["q"], shift=t["shift"], **RND),
        lambda h, s: dict(zip(("q", "shift"), i8sref.requant(h["p"], V, SEED, step=s, **RND))),
        odd=["shift"], shifts="shift", keyed=True, key_phase=1, src="ina_i8_sr.hip")
    add("i4_block_scales_w3", ["ina_block_scales_i4"],
        lambda g, p: {"x": _spread(grads(g, p, 3, N_BLK, torch.bfloat16))}, {"kb": (I8, NBLK)},
        lambda m, t, s: m["i4"].block_scales(t["x"], V, step=s, out=t["kb"], **ROT),
        lambda h, s: {"kb": i4ref.block_scales(h["x"], V, step=s, **ROT)},
        odd=["kb"], keyed=True, src="ina_i4.hip")
    add("i4_quantize", ["ina_quantize_i4_wire"],                         # nibbles clamp at 7: scales 0..2 for |r| < 1.7
        lambda g, p: {"x": grads(g, p, 1, N_BLK)[0], "kb": scales(N_BLK, 0)}, {"q": (U8, N_BLK // 2), "ovf": (U8, NBLK)},
        lambda m, t, s: m["i4"].quantize(t["x"], t["kb"], V, step=s, out=t["q"], overflow=t["ovf"], **ROT),
        lambda h, s: dict(zip(("q", "ovf"), i4ref.quantize(h["x"], h["kb"], V, step=s, **ROT))),
        odd=["ovf"], flags="ovf", cap=True, keyed=True, src="ina_i4.hip")
    add("i4_sum_slices_w17", ["ina_sum_i4_slices"],                      # a batch of 16 and one; -8 G = -136
        lambda g, p: {"p": _nibbles(g, p, 17, N_I4, 7, {1: {3: -8}, 2: {4: -8}, 3: {7: 7}})}, {"out": (I16, N_I4)},
        lambda m, t, s: m["i4"].sum_slices(t["p"], out=t["out"]),
        lambda h, s: {"out": i4ref.sum_slices(h["p"])}, src="ina_i4.hip")
    add("i4_sum_requant_w17", ["ina_sum_i4_slices_requant"],
        lambda g, p: {"p": _nibbles(g, p, 17, N_BLK, 7, PLANTS17)}, {"q": (I8, N_BLK), "shift": (U8, NBLK)},
        lambda m, t, s: m["i4"].sum_slices_requant(t["p"], V, out=t["q"], shift=t["shift"]),
        lambda h, s: dict(zip(("q", "shift"), i4ref.requant(h["p"], V))),
        odd=["shift"], cap=True, src="ina_i4.hip")
    add("i4_sum_requant_w33", ["ina_sum_i4_slices_requant"],
        lambda g, p: {"p": _nibbles(g, p, 33, N_BLK, 3, PLANTS33)}, {"q": (I8, N_BLK), "shift": (U8, NBLK)},
        lambda m, t, s: m["i4"].sum_slices_requant(t["p"], V, out=t["q"], shift=t["shift"]),
        lambda h, s: dict(zip(("q", "shift"), i4ref.requant(h["p"], V))),
        odd=["shift"], shifts="shift", src="ina_i4.hip")
    return R


ROWS = rows()
# the entry points behind a clear in front of the kernel: every one must have a row
CLEARING = {"ina_quantize_f32_i16_sat", "ina_sum_reduce_i16_sat", "ina_quantize_reduce_f32_i16_sat", "ina_absmax_f32",
            "ina_absmax_multi_f32", "ina_checksum_i32", "ina_quantize_x16_i16_sat", "ina_quantize_reduce_x16_i16_sat",
            "ina_absmax_multi_x16", "ina_quantize_sr_f32_i16_sat", "ina_quantize_reduce_sr_f32_i16_sat",
            "ina_i16_wire_finish", "ina_i16_wire_finish_blk"}
# sources that must have two single-launch rows; those with an entry point over W buckets must have one of them
SINGLE = {"ina_blk.hip": True, "ina_ef.hip": True, "ina_rot.hip": True, "ina_i8.hip": True, "ina_x16.hip": True,
          "ina_shard.hip": False, "ina_i8_gather.hip": True, "ina_i8_ef.hip": True, "ina_i8_sr.hip": True,
          "ina_i4.hip": True}
# the device entry points of the four newer wire sources: every one must appear in some row's protos
WIRES = {"ina_sum_i8_slices_requant", "ina_dequantize_i8_gather", "ina_block_scales_i8_ef", "ina_quantize_ef_i8_wire",
         "ina_block_scales_i8_sr", "ina_quantize_sr_i8_wire", "ina_sum_i8_slices_requant_sr", "ina_block_scales_i4",
         "ina_quantize_i4_wire", "ina_sum_i4_slices", "ina_sum_i4_slices_requant"}


# ---- device side ---------------------------------------------------------------------------------
class Stage:
    """A row's device buffers: every input and output a view into its own sentinel-filled allocation."""

    def __init__(self, row, like):
        self.row, self.bufs, self.t = row, {}, {}
        for name, h in like.items():
            self.t[name] = ([self._view(f"{name}{w}", x.dtype, x.numel(), name) for w, x in enumerate(h)]
                            if isinstance(h, list) else self._view(name, h.dtype, h.numel(), name))
        for name, (dt, numel) in row.outs.items():
            self.t[name] = self._view(name, dt, numel, name)

    def _view(self, key, dtype, numel, name):
        size = torch.empty(0, dtype=dtype).element_size()
        skew = size if name in self.row.mis else 1 if name in self.row.odd else 0   # 2 or 4 bytes past a 16-byte
        assert size == 1 or name not in self.row.odd                               # boundary; `odd`: one byte past
        off = GUARD + skew
        nbytes = numel * size
        buf = torch.full((off + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.bufs[key] = (buf, off, nbytes)
        v = buf[off:off + nbytes].view(dtype)
        assert v.data_ptr() % 16 == skew
        return v

    def load(self, hosts, skip=(), non_blocking=False):
        for name, h in hosts.items():
            if name in skip:
                continue
            for d, x in zip(*((self.t[name], h) if isinstance(h, list) else ([self.t[name]], [h]))):
                d.copy_(x, non_blocking=non_blocking)

    def sentinel_outputs(self):
        for name in self.row.outs:
            self.t[name].view(torch.uint8).fill_(SENTINEL)

    def names(self):
        return list(self.row.outs) + list(self.row.state)

    def check(self, got, want, tag):
        """got: {name: host tensor} of names(); bit for bit against want, and every guard byte intact."""
        for name in self.names():
            g, w = got[name].numpy(), np.ascontiguousarray(want[name])
            assert g.dtype.itemsize == w.dtype.itemsize and g.size == w.size, (tag, name, g.dtype, w.dtype, g.size, w.size)
            gb, wb = g.view(f"u{g.itemsize}"), w.view(f"u{w.itemsize}").ravel()
            bad = np.flatnonzero(gb != wb)
            assert bad.size == 0, f"{tag} {name}: {bad.size} of {g.size} differ, first at {bad[0]}: {g[bad[0]]!r} != {w.ravel()[bad[0]]!r}"
        for key, (buf, off, nbytes) in self.bufs.items():
            b = buf.cpu().numpy()
            assert (b[:off] == SENTINEL).all() and (b[off + nbytes:] == SENTINEL).all(), (tag, key, "guard bytes written")


def pinned(hosts):
    return {k: [x.pin_memory() for x in h] if isinstance(h, list) else h.pin_memory() for k, h in hosts.items()}


class Spy:
    """Stands in for the loaded library during one call and records the symbols looked up."""

    def __init__(self, lib):
        self._lib, self.seen = lib, set()

    def __getattr__(self, name):
        self.seen.add(name)
        return getattr(self._lib, name)


@contextlib.contextmanager
def spied():
    from ina_amd import _lib
    real = _lib.load()
    spy = Spy(real)
    _lib._lib = spy
    try:
        yield spy
    finally:
        _lib._lib = real


@contextlib.contextmanager
def capped(row):
    """Grid cap 1 around the warm-up and the queueing / capture of a `cap` row: several grid-stride passes."""
    from ina_amd import ops
    if row.cap:
        ops.set_tuning(max_blocks=1)
    try:
        yield
    finally:
        ops.set_tuning(max_blocks=16384)


def warm(row, st, hosts, stream):
    """One call on `stream` over `hosts`, the library's symbol look-ups checked against the row."""
    st.load(hosts)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream), spied() as spy:
        row.call(mods(), st.t, STEP)
    stream.synchronize()
    called = {n for n in spy.seen if n.startswith("ina_") and n not in ("ina_last_error_string", "ina_set_tuning")}
    assert called == set(row.protos), (row.name, called)


def sleep_cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond on this device, from one timed sleep."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(2_000_000)
    b.record()
    torch.cuda.synchronize()
    return 2_000_000 / a.elapsed_time(b)
