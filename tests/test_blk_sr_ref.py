"""The yardstick of the block-scaled stochastic-rounding tests (tests/_blk_sr_ref.py) pinned with no GPU:
it equals the global-k replay (tests/_sr_ref.py) called block by block with k = kblk[s] and e0 + s*V, it
equals the round-to-nearest block yardstick (tests/_blk_ref.py) wherever every t is an integer, and its
scales are ina_scale_for_sr called through the C ABI."""
import ctypes

import numpy as np
import pytest

from tests import _blk_ref as bref
from tests import _blk_sr_ref as bsr
from tests import _sr_ref as sref
from tests import _sr_reduce_ref as rref

SEED = 0x9E3779B97F4A7C15


def _bucket(rng, W, n, V):
    x = bref.bucket(rng, W, n, V, lo=-6.0, hi=2.0)
    x[0, 1], x[0, 5], x[-1, n - 1], x[0, 3 * V % n] = np.nan, np.inf, -np.inf, 3.0e38
    return x


@pytest.mark.parametrize("V", [8, 32, 256])
def test_replay_is_the_global_k_replay_block_by_block(V):
    rng = np.random.default_rng(V)
    W, n, e0, step, sub = 3, 5 * V + V // 2 + 1, 1 << 33, 7, 0xFFFFFFFF      # a short last block; sub + w wraps
    x = _bucket(rng, W, n, V)
    for bits in (32, 16):
        kblk = bsr.kblk_ref(x, V, 64, bits)
        kblk[2] = -128                                                         # a given scale, read as -126
        q32, w16, r32 = [], [], []
        r16, f16 = [], []
        for s, sl in enumerate(bref.blocks(n, V)):
            k, e = bref.keff(kblk[s]), e0 + s * V
            q32.append(sref.quantize(x[0, sl], k, SEED, step, sub, e))
            w16.append(sref.quantize_i16_wire(x[0, sl], k, SEED, step, sub, e))
            r32.append(rref.quantize_reduce(list(x[:, sl]), k, SEED, step, sub, e))
            o, f = rref.quantize_reduce_i16(list(x[:, sl]), k, V, SEED, step, sub, e)
            assert f.size == 1
            r16.append(o)
            f16.append(f)
        assert np.array_equal(bsr.quantize(x[0], kblk, V, SEED, step, sub, e0), np.concatenate(q32))
        assert np.array_equal(bsr.quantize_i16_wire(x[0], kblk, V, SEED, step, sub, e0), np.concatenate(w16))
        assert np.array_equal(bsr.quantize_reduce(list(x), kblk, V, SEED, step, sub, e0), np.concatenate(r32))
        o, f = bsr.quantize_reduce_i16(list(x), kblk, V, SEED, step, sub, e0)
        assert np.array_equal(o, np.concatenate(r16)) and np.array_equal(f, np.concatenate(f16))
        assert f.any() and (bits == 32 or not f.all())


@pytest.mark.parametrize("V", [12, 32])
def test_integers_round_as_the_nearest_yardstick_for_every_seed(V):
    rng = np.random.default_rng(100 + V)
    W, n = 4, 7 * V + 5
    nblk = (n + V - 1) // V
    kblk = rng.integers(-20, 20, nblk).astype(np.int8)
    scale = np.ldexp(np.float32(1), -np.repeat(kblk.astype(np.int32), V)[:n]).astype(np.float32)
    ints = rng.integers(-9000, 9000, (W, n)).astype(np.float32)
    ints[0, 0], ints[1, n - 1] = 40000.0, -70000.0                             # saturate int16, stay integers
    x = (ints * scale).astype(np.float32)                                      # t = ints exactly
    want32 = bref.quantize_reduce_i32(list(x), kblk, V)
    want16, wantf = bref.quantize_reduce_i16(list(x), kblk, V)
    for seed in (0, 1, SEED, (1 << 64) - 1):
        assert np.array_equal(bsr.quantize(x[0], kblk, V, seed), bref.quantize_i32(x[0], kblk, V))
        assert np.array_equal(bsr.quantize_reduce(list(x), kblk, V, seed, 3, 9, 8), want32)
        o, f = bsr.quantize_reduce_i16(list(x), kblk, V, seed, 3, 9, 8)
        assert np.array_equal(o, want16) and np.array_equal(f, wantf) and f[0] == 1 and f[-1] == 1


def test_scales_are_ina_scale_for_sr_through_the_c_abi():
    from ina_amd import _lib
    lib = _lib.load()
    tiny = np.float32(1e-45)
    amaxes = [0.0, float(tiny), float(np.float32(1.1754942e-38)), float(np.float32(1.17549435e-38)), 1e-30, 2.0 ** -20,
              0.3, 1.0, 1.5, 255.99, 32766.0, 32767.0, 1e9, 2.0 ** 100, 3.0e38, float(np.finfo(np.float32).max)]
    for bits, degrees in ((16, (1, 2, 16, 64, 16383)), (32, (1, 8, 64, 1 << 20))):
        for degree in degrees:
            x = np.array([[a, -a / 2] for a in amaxes], np.float32).ravel()    # blocks of V = 2, one amax each
            got = bsr.kblk_ref([x], 2, degree, bits)
            for a, k in zip(amaxes, got):
                out = ctypes.c_int(99)
                assert lib.ina_scale_for_sr(ctypes.c_float(a), degree, bits, ctypes.byref(out)) == _lib.INA_OK, a
                assert out.value == int(k), (a, degree, bits, out.value, int(k))
    # inf: the host function refuses it, a block holding it takes -126; NaN is ignored
    out = ctypes.c_int(0)
    assert lib.ina_scale_for_sr(ctypes.c_float(np.inf), 4, 16, ctypes.byref(out)) == _lib.INA_EINVAL
    x = np.array([1.0, np.inf, np.nan, 2.0, np.nan, np.nan, -np.inf, 0.0], np.float32)
    assert list(bsr.kblk_ref([x], 2, 4, 16)) == [-126, sref.scale_for_sr(2.0, 4, 16), 127, -126]
    # the degree the rule refuses: (2^15 - 1) / degree - 1 <= 0
    assert lib.ina_scale_for_sr(ctypes.c_float(1.0), 16384, 16, ctypes.byref(out)) == _lib.INA_OK
    assert lib.ina_scale_for_sr(ctypes.c_float(1.0), 32767, 16, ctypes.byref(out)) == _lib.INA_EINVAL
