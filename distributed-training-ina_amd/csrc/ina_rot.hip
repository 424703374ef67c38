// ina_rot.hip -- a randomised Hadamard rotation in front of the block-scaled quantise and reduce
// (include/ina_rot.h states the contract; the butterfly and the signs are in ina_rot_device.h).
//
// The lanes are ina_blk.hip's: a lane owns 16-byte chunks of 4 values, a block is V/4 adjacent lanes of one
// wave.  32-bit side (reduce to int32, both decodes, the PS combine, the scales): lane l of a wave owns
// values 4l..4l+3 of the wave's 256.  int16 out: a wave owns 512 values as two 256-value halves, lane l the
// 4 at 4l of each half, each half its own block group.  A wave's 256 values share two Philox calls for
// their signs, computed once per pass and used for all W workers.
//
// n is a multiple of V >= 8, so no chunk crosses n and no block is partial.  Every loop has a wave-uniform
// trip count; a lane past n reads zeros, takes part in every exchange and writes nothing.  Compile-time W
// (1, 2, 4, 8; int32 also 16) loads the lane's W chunks first and keeps their rotated images in registers
// between the max and the quantiser; any other W reads and rotates a second time in the same launch under
// AUTO.  A lane reads all of its chunks before it writes any, so out may alias an input of the same width.
// There is no value-by-value path: what the lanes cannot hold is refused.
#include <hip/hip_runtime.h>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"
#include "ina_rot_device.h"

namespace ina {
namespace {

constexpr int kBlk = 256;

// chunk i = values 4i..4i+3; base_ is the wave's first chunk (a multiple of 64)
#define INA_ROT_QUAD_LOOP(nq)                                    \
    const size_t tid_ = (size_t)blockIdx.x * kBlk + threadIdx.x; \
    const size_t stride_ = (size_t)gridDim.x * kBlk;             \
    for (size_t base_ = tid_ & ~(size_t)63; base_ < (nq); base_ += stride_)

template <typename X>
__global__ __launch_bounds__(kBlk) void k_rot_scales(PtrPack<X> xs, int W, size_t n, int shift, double lim, SrKey key,
                                                     int8_t* __restrict__ kblk) {
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_ROT_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        const u32x4 sg = rot_signs(key, 4 * base_, lane);
        uint32_t m = 0u;
        int w = 0;
        for (; w + 2 <= W; w += 2) {                                   // two workers' loads in flight
            const f32x4 a = ld4(xs.p[w], e, n), b = ld4(xs.p[w + 1], e, n);
            m = fold4(fold4(m, rot_fwd(a, sg, shift, lane)), rot_fwd(b, sg, shift, lane));
        }
        if (w < W) m = fold4(m, rot_fwd(ld4(xs.p[w], e, n), sg, shift, lane));
        m = group_max(m, 1 << shift);
        if (e < n && (lane & ((1 << shift) - 1)) == 0) kblk[i >> shift] = (int8_t)scale_of(m, lim);
    }
}

// rotate + quantise + W-way reduce to int32.  W > 0: compile-time worker count, rotated chunks held; W = 0:
// runtime count, read and rotated again under AUTO.
template <typename X, int W, bool AUTO>
__global__ __launch_bounds__(kBlk) void k_qr_rot_i32(PtrPack<X> in, int Wd, int8_t* __restrict__ kblk, double lim,
                                                     int32_t* out, size_t n, int shift, SrKey key) {
    const int nw = W > 0 ? W : Wd;
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_ROT_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        const u32x4 sg = rot_signs(key, 4 * base_, lane);
        [[maybe_unused]] f32x4 v[W > 0 ? W : 1];
        if constexpr (W > 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = ld4(in.p[w], e, n);
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = rot_fwd(v[w], sg, shift, lane);
        }
        int k = 0;
        if constexpr (AUTO) {
            uint32_t m = 0u;
            if constexpr (W > 0) {
#pragma unroll
                for (int w = 0; w < W; ++w) m = fold4(m, v[w]);
            } else {
                for (int w = 0; w < nw; ++w) m = fold4(m, rot_fwd(ld4(in.p[w], e, n), sg, shift, lane));
            }
            m = group_max(m, 1 << shift);
            k = scale_of(m, lim);
            if (e < n && (lane & ((1 << shift) - 1)) == 0) kblk[i >> shift] = (int8_t)k;
        } else {
            if (e < n) k = rd_k(kblk, i >> shift);
        }
        const float s = pow2f(k);
        u32x4 acc = {0u, 0u, 0u, 0u};
        if constexpr (W > 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) acc += q32x4(v[w], s);
        } else {
            for (int w = 0; w < nw; ++w) acc += q32x4(rot_fwd(ld4(in.p[w], e, n), sg, shift, lane), s);
        }
        if (e < n) st4(acc, out, e, n);
    }
}

// the int16 out may alias a 16-bit bucket (the same width), never an fp32 one
template <typename X>
struct Out16 {
    using P = int16_t*;
};
template <>
struct Out16<float> {
    using P = int16_t* __restrict__;
};

// the same to int16: the split halves, one flag per block from the one-writer ballot
template <typename X, int W, bool AUTO>
__global__ __launch_bounds__(kBlk) void k_qr_rot_i16(PtrPack<X> in, int Wd, int8_t* __restrict__ kblk, double lim,
                                                     typename Out16<X>::P out, size_t n, int shift, int V,
                                                     uint8_t* __restrict__ ovf, SrKey key) {
    const int nw = W > 0 ? W : Wd;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t nwaves = ((size_t)gridDim.x * kBlk) >> 6;
    const int lane = (int)(tid & 63), lanes = 1 << shift;
    const size_t nreg = (n + 511) / 512;
    for (size_t r = tid >> 6; r < nreg; r += nwaves) {          // wave-uniform
        const size_t eA = r * 512 + 4 * (size_t)lane, eB = eA + 256;
        const u32x4 sgA = rot_signs(key, r * 512, lane), sgB = rot_signs(key, r * 512 + 256, lane);
        [[maybe_unused]] f32x4 u[W > 0 ? W : 1], v[W > 0 ? W : 1];
        if constexpr (W > 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                u[w] = ld4(in.p[w], eA, n);
                v[w] = ld4(in.p[w], eB, n);
            }
#pragma unroll
            for (int w = 0; w < W; ++w) {
                u[w] = rot_fwd(u[w], sgA, shift, lane);
                v[w] = rot_fwd(v[w], sgB, shift, lane);
            }
        }
        int kA = 0, kB = 0;
        if constexpr (AUTO) {
            uint32_t mA = 0u, mB = 0u;
            if constexpr (W > 0) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    mA = fold4(mA, u[w]);
                    mB = fold4(mB, v[w]);
                }
            } else {
                for (int w = 0; w < nw; ++w) {
                    const f32x4 a = ld4(in.p[w], eA, n), b = ld4(in.p[w], eB, n);
                    mA = fold4(mA, rot_fwd(a, sgA, shift, lane));
                    mB = fold4(mB, rot_fwd(b, sgB, shift, lane));
                }
            }
            mA = group_max(mA, lanes);
            mB = group_max(mB, lanes);
            kA = scale_of(mA, lim);
            kB = scale_of(mB, lim);
            if ((lane & (lanes - 1)) == 0) {
                if (eA < n) kblk[eA >> (shift + 2)] = (int8_t)kA;
                if (eB < n) kblk[eB >> (shift + 2)] = (int8_t)kB;
            }
        } else {
            if (eA < n) kA = rd_k(kblk, eA >> (shift + 2));
            if (eB < n) kB = rd_k(kblk, eB >> (shift + 2));
        }
        const float sA = pow2f(kA), sB = pow2f(kB);
        bool sa = false, sb = false;
        int32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
        if constexpr (W > 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                q16x4_add(u[w], sA, a, sa);
                q16x4_add(v[w], sB, b, sb);
            }
        } else {
            for (int w = 0; w < nw; ++w) {
                const f32x4 x = ld4(in.p[w], eA, n), y = ld4(in.p[w], eB, n);
                q16x4_add(rot_fwd(x, sgA, shift, lane), sA, a, sa);
                q16x4_add(rot_fwd(y, sgB, shift, lane), sB, b, sb);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = sat16(a[j], sa);
            b[j] = sat16(b[j], sb);
        }
        if (eA < n) st4h(a, out, eA, n);
        if (eB < n) st4h(b, out, eB, n);
        const unsigned long long ma = __ballot(sa), mb = __ballot(sb);   // wave-convergent
        if (ovf) {
            write_slot_flags8(ma, eA < n, eA, V, lanes, ovf);
            write_slot_flags8(mb, eB < n, eB, V, lanes, ovf);
        }
    }
}

// dequantise + inverse rotation; T: int32_t or int16_t
template <typename T>
__global__ __launch_bounds__(kBlk) void k_dq_rot(const T* __restrict__ sv, const int8_t* __restrict__ kblk,
                                                 float* __restrict__ y, size_t n, int shift, SrKey key) {
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_ROT_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        const u32x4 sg = rot_signs(key, 4 * base_, lane);
        u32x4 q;
        if constexpr (sizeof(T) == 4) q = ld4i(sv, e, n);
        else q = ld4h(sv, e, n);
        const int k = e < n ? rd_k(kblk, i >> shift) : 0;
        const f32x4 x = rot_inv(deq4(q, pow2f(-k)), sg, shift, lane);
        if (e < n) st4(x, y, e, n);
    }
}

// the INA update in one pass: deltas -> rotate -> AUTO scale (degree = W, bits = 32) -> quantise -> sum ->
// dequantise -> inverse rotate -> local + xhat * ws
template <int W>
__global__ __launch_bounds__(kBlk) void k_ps_combine_rot(const float* local, PtrPack<float> paras, int Wd, double lim,
                                                         float ws, float* out, size_t n, int shift,
                                                         int8_t* __restrict__ kblk, SrKey key) {
    const int nw = W > 0 ? W : Wd;
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_ROT_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        const u32x4 sg = rot_signs(key, 4 * base_, lane);
        const f32x4 l = ld4<false>(local, e, n);
        [[maybe_unused]] f32x4 d[W > 0 ? W : 1];
        uint32_t m = 0u;
        if constexpr (W > 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) d[w] = ld4(paras.p[w], e, n);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                d[w] = rot_fwd(sub4(d[w], l), sg, shift, lane);
                m = fold4(m, d[w]);
            }
        } else {
            for (int w = 0; w < nw; ++w) m = fold4(m, rot_fwd(sub4(ld4(paras.p[w], e, n), l), sg, shift, lane));
        }
        m = group_max(m, 1 << shift);
        const int k = scale_of(m, lim);
        if (kblk && e < n && (lane & ((1 << shift) - 1)) == 0) kblk[i >> shift] = (int8_t)k;
        const float s = pow2f(k);
        u32x4 acc = {0u, 0u, 0u, 0u};
        if constexpr (W > 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) acc += q32x4(d[w], s);
        } else {
            for (int w = 0; w < nw; ++w) acc += q32x4(rot_fwd(sub4(ld4(paras.p[w], e, n), l), sg, shift, lane), s);
        }
        const f32x4 x = rot_inv(deq4(acc, pow2f(-k)), sg, shift, lane);
        if (e < n) st4(upd4(l, x, ws), out, e, n);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int launched() { return check_launch("rotation kernel launch"); }

using bf16_t = h16<INA_X16_BF16>;
using fp16_t = h16<INA_X16_F16>;

int check_xtype(int xtype) {
    if (xtype == INA_ROT_F32 || xtype == INA_X16_BF16 || xtype == INA_X16_F16) return INA_OK;
    return set_error(INA_EINVAL, "xtype must be INA_ROT_F32 (0), INA_X16_BF16 (1) or INA_X16_F16 (2)%s", "");
}
// V a power of two in [8, 256] and n a multiple of it; shift = log2(V) - 2
int check_rot_v(int V, int& shift) {
    if (!vec_v(V, shift)) return set_error(INA_EINVAL, "V must be a power of two in [8, 256]%s", "");
    return INA_OK;
}
int check_n(size_t n, int V) {
    return n % (size_t)V ? set_error(INA_EINVAL, "n must be a multiple of V%s", "") : INA_OK;
}
int misaligned() { return set_error(INA_EINVAL, "buffers must be 16-byte aligned%s", ""); }

// what the three W-way calls share, checked in the header's order up to the buckets
struct RotCall {
    int shift;
    double lim;
    SrKey key;
};

// F<X>(args) for a checked xtype
#define INA_ROT_X_CALL(xtype, F, ...)                          \
    ((xtype) == INA_X16_BF16  ? F<bf16_t>(__VA_ARGS__)         \
     : (xtype) == INA_X16_F16 ? F<fp16_t>(__VA_ARGS__)         \
                              : F<float>(__VA_ARGS__))

template <typename X>
int block_scales(const void* const* xs, int W, size_t n, int V, int degree, int bits, int8_t* kblk, const ina_sr_t* sr,
                 ina_stream_t stream) {
    int shift;
    double lim;
    if (int rc = check_rot_v(V, shift)) return rc;
    if (int rc = scale_lim(degree, bits, lim)) return rc;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    if (int rc = check_n(n, V)) return rc;
    if (n == 0) return INA_OK;
    PtrPack<X> pk;
    bool al;
    if (int rc = fill_pack(pk, xs, W, al)) return rc;
    if (!al) return misaligned();
    SrKey key;
    if (int rc = rot_key(sr, V, key)) return rc;
    hipLaunchKernelGGL(k_rot_scales<X>, dim3(grid_of(n / 4, default_grid_cap())), dim3(kBlk), 0, hs(stream), pk, W, n,
                       shift, lim, key, kblk);
    return launched();
}

// the checks of both fused reduces: everything but the launch
template <typename X>
int reduce_args(const void* const* bufs, int W, const int8_t* kblk, int mode, int degree, int bits, int V,
                const void* out, size_t n, const ina_sr_t* sr, PtrPack<X>& pk, RotCall& c, bool& go) {
    go = false;
    if (int rc = check_rot_v(V, c.shift)) return rc;
    if (int rc = check_mode(mode, kblk, degree, bits, c.lim)) return rc;
    if (int rc = check_n(n, V)) return rc;
    if (n == 0) return INA_OK;
    bool al;
    if (int rc = fill_pack(pk, bufs, W, al)) return rc;
    if (!out) return set_error(INA_EINVAL, "null out%s", "");
    if (!al || !aligned16(out)) return misaligned();
    if (int rc = rot_key(sr, V, c.key)) return rc;
    go = true;
    return INA_OK;
}

// compile-time worker counts of the fused kernels (others: the runtime-W instance); MAXW: the largest held
#define INA_ROT_W_SWITCH(W, MAXW, LAUNCH)                          \
    switch ((W) <= (MAXW) ? (W) : 0) {                             \
        case 1: LAUNCH(1); break;                                  \
        case 2: LAUNCH(2); break;                                  \
        case 4: LAUNCH(4); break;                                  \
        case 8: LAUNCH(8); break;                                  \
        case 16: LAUNCH(16); break;                                \
        default: LAUNCH(0);                                        \
    }

template <typename X>
int reduce_i32(const void* const* bufs, int W, int8_t* kblk, int mode, int degree, int V, int32_t* out, size_t n,
               const ina_sr_t* sr, ina_stream_t stream) {
    PtrPack<X> pk;
    RotCall c;
    bool go;
    if (int rc = reduce_args<X>(bufs, W, kblk, mode, degree, 32, V, out, n, sr, pk, c, go)) return rc;
    if (!go) return INA_OK;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
#define L(WW)                                                                                                          \
    do {                                                                                                               \
        if (mode == INA_BLK_AUTO) hipLaunchKernelGGL((k_qr_rot_i32<X, WW, true>), g, b, 0, s, pk, W, kblk, c.lim, out, n, c.shift, c.key); \
        else hipLaunchKernelGGL((k_qr_rot_i32<X, WW, false>), g, b, 0, s, pk, W, kblk, c.lim, out, n, c.shift, c.key); \
    } while (0)
    INA_ROT_W_SWITCH(W, 16, L)
#undef L
    return launched();
}

// (AUTO at W = 16 takes the re-read instance: two halves of 16 held chunks are 128 VGPRs before any
// temporaries.  Given scales at W = 8 take the runtime-W instance, which reads once all the same: the held
// one came out at 186 VGPRs, two waves a SIMD)
template <typename X>
int reduce_i16(const void* const* bufs, int W, int8_t* kblk, int mode, int degree, int V, int16_t* out, size_t n,
               uint8_t* ovf, const ina_sr_t* sr, ina_stream_t stream) {
    PtrPack<X> pk;
    RotCall c;
    bool go;
    if (int rc = reduce_args<X>(bufs, W, kblk, mode, degree, 16, V, out, n, sr, pk, c, go)) return rc;
    if (!go) return INA_OK;
    const dim3 g(grid_of((n + 511) / 512 * 64, default_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
#define L(WW)                                                                                                          \
    do {                                                                                                               \
        if (mode == INA_BLK_AUTO) hipLaunchKernelGGL((k_qr_rot_i16<X, (WW <= 8 ? WW : 0), true>), g, b, 0, s, pk, W, kblk, c.lim, out, n, c.shift, V, ovf, c.key); \
        else hipLaunchKernelGGL((k_qr_rot_i16<X, (WW <= 4 ? WW : 0), false>), g, b, 0, s, pk, W, kblk, c.lim, out, n, c.shift, V, ovf, c.key); \
    } while (0)
    INA_ROT_W_SWITCH(W, 8, L)
#undef L
    return launched();
}

template <typename T>
int dequantize(const T* sv, const int8_t* kblk, int V, float* y, size_t n, const ina_sr_t* sr, ina_stream_t stream) {
    int shift;
    if (int rc = check_rot_v(V, shift)) return rc;
    if (int rc = check_n(n, V)) return rc;
    if (n == 0) return INA_OK;
    if (!sv || !y || !kblk) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!aligned16(sv) || !aligned16(y)) return misaligned();
    SrKey key;
    if (int rc = rot_key(sr, V, key)) return rc;
    hipLaunchKernelGGL(k_dq_rot<T>, dim3(grid_of(n / 4, default_grid_cap())), dim3(kBlk), 0, hs(stream), sv, kblk, y, n,
                       shift, key);
    return launched();
}

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

int ina_block_scales_rot(const void* const* xs, int xtype, int W, size_t n, int V, int degree, int bits, int8_t* kblk,
                         const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_ROT_X_CALL(xtype, block_scales, xs, W, n, V, degree, bits, kblk, sr, stream);
}

int ina_quantize_reduce_rot_i32(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode, int degree, int V,
                                int32_t* out, size_t n, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_ROT_X_CALL(xtype, reduce_i32, bufs, W, kblk, mode, degree, V, out, n, sr, stream);
}

int ina_quantize_reduce_rot_i16_sat(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode, int degree,
                                    int V, int16_t* out, size_t n, uint8_t* overflow_per_slot, const ina_sr_t* sr,
                                    ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_ROT_X_CALL(xtype, reduce_i16, bufs, W, kblk, mode, degree, V, out, n, overflow_per_slot, sr, stream);
}

int ina_dequantize_rot_i32(const int32_t* sv, const int8_t* kblk, int V, float* y, size_t n, const ina_sr_t* sr,
                           ina_stream_t stream) {
    return dequantize(sv, kblk, V, y, n, sr, stream);
}

int ina_dequantize_rot_i16(const int16_t* sv, const int8_t* kblk, int V, float* y, size_t n, const ina_sr_t* sr,
                           ina_stream_t stream) {
    return dequantize(sv, kblk, V, y, n, sr, stream);
}

int ina_ps_combine_ina_rot_f32(const float* local, const float* const* paras, int W, int V, double weight_step,
                               float* out, size_t n, int8_t* kblk_out, const ina_sr_t* sr, ina_stream_t stream) {
    int shift;
    if (int rc = check_rot_v(V, shift)) return rc;
    if (int rc = check_n(n, V)) return rc;
    if (n == 0) return INA_OK;
    PtrPack<float> pk;
    bool al;
    if (int rc = fill_pack(pk, paras, W, al)) return rc;
    if (!local || !out) return set_error(INA_EINVAL, "null pointer%s", "");
    double lim;
    if (int rc = scale_lim(W, 32, lim)) return rc;
    if (!al || !aligned16(local) || !aligned16(out)) return misaligned();
    SrKey key;
    if (int rc = rot_key(sr, V, key)) return rc;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
    const float ws = (float)weight_step;
#define L(WW) hipLaunchKernelGGL(k_ps_combine_rot<WW>, g, b, 0, s, local, pk, W, lim, ws, out, n, shift, kblk_out, key)
    INA_ROT_W_SWITCH(W, 16, L)
#undef L
    return launched();
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_rot() { return take_store_violations(); }
#endif
