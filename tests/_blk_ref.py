"""The yardstick of the per-block-scale tests (include/ina_blk.h): the existing CPU oracle called
once per block with that block's k.  Nothing here touches the GPU or a block-scaled entry point."""
import numpy as np

from oracle import oracle as orc


def blocks(n: int, V: int):
    return [slice(s * V, min(n, (s + 1) * V)) for s in range((n + V - 1) // V)]


def keff(k) -> int:
    """A given scale of -127 / -128 is read as -126."""
    return max(int(k), -126)


def kblk_ref(xs, V: int, degree: int, bits: int, base=None) -> np.ndarray:
    """int8 [nblk]: ops.scale_for(max |xs[w][i] - base[i]| of the block, NaN ignored, degree, bits);
    a block holding +-inf gives -126."""
    from ina_amd import ops
    xs = np.stack([np.asarray(x, np.float32) for x in xs])
    d = np.abs(xs - np.asarray(base, np.float32)[None, :]) if base is not None else np.abs(xs)   # fp32 subtraction
    out = np.empty((xs.shape[1] + V - 1) // V, np.int8)
    for s, sl in enumerate(blocks(xs.shape[1], V)):
        b = d[:, sl].ravel()
        if np.isinf(b).any():
            out[s] = -126
        else:
            out[s] = ops.scale_for(float(np.fmax.reduce(b, initial=np.float32(0))), degree, bits)
    return out


def quantize_i32(x, kblk, V):
    x = np.asarray(x, np.float32)
    return np.concatenate([orc.quantize_i32(x[sl], keff(kblk[s])) for s, sl in enumerate(blocks(x.size, V))])


def quantize_i16(x, kblk, V):
    return quantize_reduce_i16([x], kblk, V)


def quantize_reduce_i32(bufs, kblk, V):
    bufs = [np.asarray(b, np.float32) for b in bufs]
    return np.concatenate([orc.quantize_reduce_i32([b[sl] for b in bufs], keff(kblk[s]))
                           for s, sl in enumerate(blocks(bufs[0].size, V))])


def quantize_reduce_i16(bufs, kblk, V):
    """(int16 sums, one overflow flag per block)"""
    bufs = [np.asarray(b, np.float32) for b in bufs]
    outs, flags = [], []
    for s, sl in enumerate(blocks(bufs[0].size, V)):
        o, f = orc.quantize_reduce_i16_sat([b[sl] for b in bufs], keff(kblk[s]), V)
        assert f.size == 1
        outs.append(o)
        flags.append(f)
    return np.concatenate(outs), np.concatenate(flags)


def dequantize(s_int, kblk, V):
    fn = orc.dequantize_i16 if s_int.dtype == np.int16 else orc.dequantize_i32
    return np.concatenate([fn(s_int[sl], keff(kblk[s])) for s, sl in enumerate(blocks(s_int.size, V))])


def ps_apply(local, sum_int, kblk, V, weight_step):
    """local + float(weight_step) * dequantise(sum_int): the oracle's dequantise, then the PS
    update's two unfused fp32 operations (oracle ps_combine_ina_f32's last line)."""
    y = dequantize(np.asarray(sum_int, np.int32), kblk, V)
    return (np.asarray(local, np.float32) + y * np.float32(weight_step)).astype(np.float32)


def ps_combine_ina(local, paras, kblk, V, weight_step):
    local = np.asarray(local, np.float32)
    paras = [np.asarray(p, np.float32) for p in paras]
    return np.concatenate([orc.ps_combine_ina_f32(local[sl], [p[sl] for p in paras], keff(kblk[s]), weight_step)
                           for s, sl in enumerate(blocks(local.size, V))])


def bucket(rng, W: int, n: int, V: int, lo=-9.0, hi=3.0) -> np.ndarray:
    """[W, n] fp32, block magnitudes log-uniform over 10^lo .. 10^hi: neighbouring blocks carry
    different k."""
    nblk = (n + V - 1) // V
    mag = np.repeat(10.0 ** rng.uniform(lo, hi, nblk), V)[:n]
    return (rng.standard_normal((W, n)) * mag).astype(np.float32)
