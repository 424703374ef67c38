// ina_x16.hip -- bf16 / fp16 gradient buckets on the quantise, fused-reduce, absmax and
// dequantise paths (include/ina.h, "bf16 / fp16 gradients").
//
// The reference names its data path "16bit float -> 32bit integer -> int(signed)"
// (src/p4/p4src/types.p4:10).  These kernels read the 16-bit bucket as it is, widen each
// value in registers (exact, ina_device.h widen16) and run the quantiser of the fp32 entry
// points (q32 / q16 / sat16, ina_device.h) on it, so every result is bit for bit the fp32
// sibling's on the widened buffer -- without the widening pass, the second copy in HBM and
// the doubled read.  The packs from 16-bit sources reuse the pack kernels of
// ina_kernels.hip through a 16-bit value source (SrcX16 there).
//
// Lane layout (HBM-streaming kernels, 256-thread workgroups, non-temporal loads,
// write-through stores, like their siblings).  A 16-bit value is half as wide as the
// int32 / fp32 word on the other side, so a lane that loaded 16 bytes would own 32 bytes of
// the wide side and its stores would sit 32 bytes apart.  Instead:
//   16-bit <-> 32-bit (quantise to int32, fused reduce to int32, dequantise from int32,
//     absmax against an fp32 base): a lane owns 4 values -- one 8-byte access on the 16-bit
//     side, one 16-byte access on the 32-bit side; a wave's instruction covers 512 B and
//     1 KiB contiguous (the layout of k_dequantize_i16).
//   16-bit <-> 16-bit (quantise to int16, fused reduce to int16, dequantise from int16):
//     a lane owns 8 values, 16 bytes on both sides, 1 KiB contiguous per instruction; a slot
//     of V values is V/8 adjacent lanes, so the one-writer ballot flags (write_slot_flags8)
//     apply as they are.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"

namespace ina {
namespace {

constexpr int kBlk = kHostBlock;

// ---------------------------------------------------------------------------
// quantise
// ---------------------------------------------------------------------------
template <int XT>
__global__ __launch_bounds__(kBlk) void k_quantize_x16_i32(const uint16_t* __restrict__ x,
                                                           int32_t* __restrict__ q, size_t n, float s,
                                                           int vec) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = tid; i < n4; i += stride) {
        const u32x2 h = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(x) + i);
        stream_store(q32x4(widen16x4<XT>(h), s), reinterpret_cast<u32x4*>(q) + i);
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) q[i] = q32(widen16<XT>(x[i]), s);
}

// the 8 values of one 16-byte load, quantised to int16 (widened to int32), sat |= any clamp / NaN
template <int XT>
__device__ __forceinline__ void q16x8_add(u32x4 h, float s, int32_t (&a)[8], bool& sat) {
    const f32x4 lo = widen16x4<XT>(u32x2{h.x, h.y}), hi = widen16x4<XT>(u32x2{h.z, h.w});
    a[0] += q16(lo.x, s, sat); a[1] += q16(lo.y, s, sat); a[2] += q16(lo.z, s, sat); a[3] += q16(lo.w, s, sat);
    a[4] += q16(hi.x, s, sat); a[5] += q16(hi.y, s, sat); a[6] += q16(hi.z, s, sat); a[7] += q16(hi.w, s, sat);
}
__device__ __forceinline__ u32x4 sat16x8(const int32_t (&a)[8], bool& sat) {
    u32x4 o;
    o.x = (uint32_t)(uint16_t)sat16(a[0], sat) | ((uint32_t)sat16(a[1], sat) << 16);
    o.y = (uint32_t)(uint16_t)sat16(a[2], sat) | ((uint32_t)sat16(a[3], sat) << 16);
    o.z = (uint32_t)(uint16_t)sat16(a[4], sat) | ((uint32_t)sat16(a[5], sat) << 16);
    o.w = (uint32_t)(uint16_t)sat16(a[6], sat) | ((uint32_t)sat16(a[7], sat) << 16);
    return o;
}

// fused quantise + W-way reduce to int16 (W = 1: the plain quantiser -- the final sat16 of
// one already-saturated value changes nothing).  W > 0: compile-time worker count.
template <int XT, int W>
__global__ __launch_bounds__(kBlk) void k_quant_reduce_x16_i16(PtrPack<uint16_t> in, int Wd,
                                                               int16_t* __restrict__ out, size_t n, float s,
                                                               int V, int lanes_per_slot,
                                                               uint8_t* __restrict__ ovf) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const int nw = W > 0 ? W : Wd;
    constexpr int UNR = W > 0 ? W : 1;
    const size_t n8 = (n + 7) / 8;
    // uniform trip count per wave so every lane reaches the ballot together
    const size_t wave0 = tid & ~(size_t)63;
    for (size_t base = wave0; base < n8; base += stride) {
        const size_t i = base + (tid & 63);
        bool sat = false;
        if (i < n8) {
            const size_t e = 8 * i;
            if (e + 8 <= n) {
                int32_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll UNR
                for (int w = 0; w < nw; ++w)
                    q16x8_add<XT>(__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in.p[w] + e)), s, a, sat);
                stream_store(sat16x8(a, sat), reinterpret_cast<u32x4*>(out + e));
            } else {
                for (size_t j = e; j < n; ++j) {
                    int32_t a = 0;
                    for (int w = 0; w < nw; ++w) a += q16(widen16<XT>(in.p[w][j]), s, sat);
                    out[j] = (int16_t)sat16(a, sat);
                }
            }
        }
        const unsigned long long m = __ballot(sat);   // wave-convergent: uniform trip count
        if (ovf) write_slot_flags8(m, i < n8, 8 * i, V, lanes_per_slot, ovf);
    }
}

// unaligned buffers or V without a ballot layout: byte flags in a pre-zeroed array,
// benign same-value stores
template <int XT>
__global__ __launch_bounds__(kBlk) void k_quant_reduce_x16_i16_scalar(PtrPack<uint16_t> in, int W,
                                                                      int16_t* __restrict__ out, size_t n,
                                                                      float s, int V,
                                                                      uint8_t* __restrict__ ovf) {
    const size_t stride = (size_t)gridDim.x * kBlk;
    for (size_t i = (size_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += stride) {
        bool sat = false;
        int32_t a = 0;
        for (int w = 0; w < W; ++w) a += q16(widen16<XT>(in.p[w][i]), s, sat);
        out[i] = (int16_t)sat16(a, sat);
        if (sat && ovf) ovf[i / (size_t)V] = 1;
    }
}

// fused quantise + W-way reduce to int32: every worker's 8-byte load in flight, one
// 16-byte store
template <int XT, int W>
__global__ __launch_bounds__(kBlk) void k_quant_reduce_x16_i32(PtrPack<uint16_t> in, int Wd,
                                                               int32_t* __restrict__ out, size_t n, float s,
                                                               int vec) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const int nw = W > 0 ? W : Wd;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = tid; i < n4; i += stride) {
        u32x4 acc = {0u, 0u, 0u, 0u};
        if constexpr (W > 0) {
            u32x2 h[W];
#pragma unroll
            for (int w = 0; w < W; ++w) h[w] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(in.p[w]) + i);
#pragma unroll
            for (int w = 0; w < W; ++w) acc += q32x4(widen16x4<XT>(h[w]), s);
        } else {
            for (int w = 0; w < nw; ++w)
                acc += q32x4(widen16x4<XT>(__builtin_nontemporal_load(reinterpret_cast<const u32x2*>(in.p[w]) + i)), s);
        }
        stream_store(acc, reinterpret_cast<u32x4*>(out) + i);
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) {
        uint32_t a = 0;
        for (int w = 0; w < nw; ++w) a += (uint32_t)q32(widen16<XT>(in.p[w][i]), s);
        out[i] = (int32_t)a;
    }
}

// ---------------------------------------------------------------------------
// absmax over W buckets against an fp32 base: the base chunk read once for all workers,
// 4 workers' loads in flight at a time; blocks combine with one atomicMax on the bits
// (non-negative floats order like their bit patterns; NaN is dropped by fmaxf)
// ---------------------------------------------------------------------------
template <int XT>
__global__ __launch_bounds__(kBlk) void k_absmax_multi_x16(PtrPack<uint16_t> xs, int W,
                                                           const float* __restrict__ base, size_t n, int vec,
                                                           uint32_t* __restrict__ out) {
    __shared__ float part[kBlk / 64];
    const size_t n4 = vec ? n / 4 : 0;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    float m = 0.0f;
    auto fold = [&](u32x2 h, f32x4 b) {
        const f32x4 a = widen16x4<XT>(h);
        m = fmaxf(m, fabsf(__fsub_rn(a.x, b.x)));
        m = fmaxf(m, fabsf(__fsub_rn(a.y, b.y)));
        m = fmaxf(m, fabsf(__fsub_rn(a.z, b.z)));
        m = fmaxf(m, fabsf(__fsub_rn(a.w, b.w)));
    };
    for (size_t i = tid; i < n4; i += stride) {
        const f32x4 b = base ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base) + i)
                             : f32x4{0.f, 0.f, 0.f, 0.f};
        int w = 0;
        for (; w + 4 <= W; w += 4) {
            u32x2 h[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) h[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(xs.p[w + u]) + i);
#pragma unroll
            for (int u = 0; u < 4; ++u) fold(h[u], b);
        }
        for (; w < W; ++w) fold(__builtin_nontemporal_load(reinterpret_cast<const u32x2*>(xs.p[w]) + i), b);
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride)
        for (int w = 0; w < W; ++w) {
            const float a = widen16<XT>(xs.p[w][i]);
            m = fmaxf(m, fabsf(base ? __fsub_rn(a, base[i]) : a));
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = part[0];
        for (int w = 1; w < kBlk / 64; ++w) r = fmaxf(r, part[w]);
        atomicMax(out, __float_as_uint(r));
    }
}

// ---------------------------------------------------------------------------
// dequantise: y = rne16((float)s * 2^-k)
// ---------------------------------------------------------------------------
template <int YT>
__global__ __launch_bounds__(kBlk) void k_dequantize_i32_x16(const int32_t* __restrict__ sv,
                                                             uint16_t* __restrict__ y, size_t n, float inv,
                                                             int vec) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = tid; i < n4; i += stride) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sv) + i);
        u32x2 r;
        r.x = rne16x2<YT>((float)(int32_t)v.x * inv, (float)(int32_t)v.y * inv);
        r.y = rne16x2<YT>((float)(int32_t)v.z * inv, (float)(int32_t)v.w * inv);
        stream_store(r, reinterpret_cast<u32x2*>(y) + i);
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) y[i] = (uint16_t)rne16<YT>((float)sv[i] * inv);
}

__device__ __forceinline__ float lo16f(uint32_t w) { return (float)(int16_t)(w & 0xFFFFu); }
__device__ __forceinline__ float hi16f(uint32_t w) { return (float)((int32_t)w >> 16); }

template <int YT>
__global__ __launch_bounds__(kBlk) void k_dequantize_i16_x16(const int16_t* __restrict__ sv,
                                                             uint16_t* __restrict__ y, size_t n, float inv,
                                                             int vec) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const size_t n8 = vec ? n / 8 : 0;
    for (size_t i = tid; i < n8; i += stride) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sv) + i);
        u32x4 r;
        r.x = rne16x2<YT>(lo16f(v.x) * inv, hi16f(v.x) * inv);
        r.y = rne16x2<YT>(lo16f(v.y) * inv, hi16f(v.y) * inv);
        r.z = rne16x2<YT>(lo16f(v.z) * inv, hi16f(v.z) * inv);
        r.w = rne16x2<YT>(lo16f(v.w) * inv, hi16f(v.w) * inv);
        stream_store(r, reinterpret_cast<u32x4*>(y) + i);
    }
    for (size_t i = 8 * n8 + tid; i < n; i += stride) y[i] = (uint16_t)rne16<YT>((float)sv[i] * inv);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int launched() { return check_launch("16-bit kernel launch"); }

// XT-dispatched launches (xtype already checked)
#define INA_X16_LAUNCH(xt, KERNEL, ...)                                                       \
    do {                                                                                      \
        if ((xt) == INA_X16_BF16) hipLaunchKernelGGL((KERNEL<INA_X16_BF16>), __VA_ARGS__);    \
        else hipLaunchKernelGGL((KERNEL<INA_X16_F16>), __VA_ARGS__);                          \
    } while (0)
#define INA_X16_LAUNCH_W(xt, KERNEL, WW, ...)                                                 \
    do {                                                                                      \
        if ((xt) == INA_X16_BF16) hipLaunchKernelGGL((KERNEL<INA_X16_BF16, WW>), __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<INA_X16_F16, WW>), __VA_ARGS__);                      \
    } while (0)

int reduce_i16(const void* const* bufs, int xtype, int W, int16_t* out, size_t n, int k, int V,
               uint8_t* ovf, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    PtrPack<uint16_t> pk;
    bool al;
    if (int rc = fill_pack(pk, bufs, W, al)) return rc;
    if (!out) return set_error(INA_EINVAL, "null out%s", "");
    hipStream_t s = hs(stream);
    const float sc = ldexpf(1.0f, k);
    if (al && aligned16(out) && (!ovf || slot_ballot_ok(V))) {
        const int lps = slot_ballot_ok(V) ? V / 8 : 1;
        const dim3 g(grid_of((n + 7) / 8, default_grid_cap())), b(kBlk);
        switch (W) {
            case 1: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i16, 1, g, b, 0, s, pk, W, out, n, sc, V, lps, ovf); break;
            case 4: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i16, 4, g, b, 0, s, pk, W, out, n, sc, V, lps, ovf); break;
            case 8: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i16, 8, g, b, 0, s, pk, W, out, n, sc, V, lps, ovf); break;
            case 16: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i16, 16, g, b, 0, s, pk, W, out, n, sc, V, lps, ovf); break;
            default: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i16, 0, g, b, 0, s, pk, W, out, n, sc, V, lps, ovf);
        }
    } else {
        if (ovf && hipMemsetAsync(ovf, 0, (n + V - 1) / V, s) != hipSuccess)
            return set_error(INA_EHIP, "memset overflow flags%s", "");
        INA_X16_LAUNCH(xtype, k_quant_reduce_x16_i16_scalar, dim3(grid_of(n, default_grid_cap())), dim3(kBlk), 0, s,
                       pk, W, out, n, sc, V, ovf);
    }
    return launched();
}

}  // namespace

int check_x16_type(int xtype) {
    if (xtype == INA_X16_BF16 || xtype == INA_X16_F16) return INA_OK;
    return set_error(INA_EINVAL, "16-bit type must be INA_X16_BF16 (1) or INA_X16_F16 (2)%s", "");
}

}  // namespace ina

using namespace ina;

extern "C" {

int ina_quantize_x16_i32(const void* x, int xtype, int32_t* q, size_t n, int k, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    if ((uintptr_t)x & 1u) return set_error(INA_EINVAL, "16-bit buffers must be 2-byte aligned%s", "");
    const int vec = aligned16(x) && aligned16(q);
    // one chunk per thread, the grid covering the bucket, like the fp32 quantiser
    INA_X16_LAUNCH(xtype, k_quantize_x16_i32, dim3(grid_of(vec ? n / 4 + 1 : n, ew_grid_cap())), dim3(kBlk), 0,
                   hs(stream), static_cast<const uint16_t*>(x), q, n, ldexpf(1.0f, k), vec);
    return launched();
}

int ina_quantize_x16_i16_sat(const void* x, int xtype, int16_t* q, size_t n, int k, int V, uint8_t* ovf,
                             ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    const void* one[1] = {x};
    return reduce_i16(one, xtype, 1, q, n, k, V, ovf, stream);
}

int ina_quantize_reduce_x16_i32(const void* const* bufs, int xtype, int W, int32_t* out, size_t n, int k,
                                ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    PtrPack<uint16_t> pk;
    bool al;
    if (int rc = fill_pack(pk, bufs, W, al)) return rc;
    if (!out) return set_error(INA_EINVAL, "null out%s", "");
    // one worker: the sum is the quantised buffer itself
    if (W == 1) return ina_quantize_x16_i32(bufs[0], xtype, out, n, k, stream);
    const int vec = al && aligned16(out);
    const float sc = ldexpf(1.0f, k);
    // the sibling's grids: covering for W <= 8, the streaming cap beyond
    const dim3 g(grid_of(vec ? n / 4 + 1 : n, W <= 8 ? ew_grid_cap() : stream_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
    switch (W) {
        case 2: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i32, 2, g, b, 0, s, pk, W, out, n, sc, vec); break;
        case 4: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i32, 4, g, b, 0, s, pk, W, out, n, sc, vec); break;
        case 8: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i32, 8, g, b, 0, s, pk, W, out, n, sc, vec); break;
        case 16: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i32, 16, g, b, 0, s, pk, W, out, n, sc, vec); break;
        default: INA_X16_LAUNCH_W(xtype, k_quant_reduce_x16_i32, 0, g, b, 0, s, pk, W, out, n, sc, vec);
    }
    return launched();
}

int ina_quantize_reduce_x16_i16_sat(const void* const* bufs, int xtype, int W, int16_t* out, size_t n, int k,
                                    int V, uint8_t* ovf, ina_stream_t stream) {
    return reduce_i16(bufs, xtype, W, out, n, k, V, ovf, stream);
}

int ina_absmax_multi_x16(const void* const* xs, int xtype, int W, const float* base, size_t n, float* out_dev,
                         ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (!out_dev) return set_error(INA_EINVAL, "null out%s", "");
    PtrPack<uint16_t> pk;
    bool al;
    if (int rc = fill_pack(pk, xs, W, al)) return rc;
    hipStream_t s = hs(stream);
    if (hipMemsetAsync(out_dev, 0, sizeof(float), s) != hipSuccess)
        return set_error(INA_EHIP, "memset absmax%s", "");
    if (n == 0) return INA_OK;
    const int vec = al && (!base || aligned16(base));
    // every block ends in one atomicMax on the same word, so the grid stays small (the
    // fp32 multi-bucket pass's 512 workgroups)
    INA_X16_LAUNCH(xtype, k_absmax_multi_x16, dim3(grid_of(vec ? n / 4 + 1 : n, 512)), dim3(kBlk), 0, s, pk, W,
                   base, n, vec, reinterpret_cast<uint32_t*>(out_dev));
    return launched();
}

int ina_dequantize_i32_x16(const int32_t* sv, void* y, int ytype, size_t n, int k, ina_stream_t stream) {
    if (int rc = check_x16_type(ytype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!sv || !y) return set_error(INA_EINVAL, "null pointer%s", "");
    if ((uintptr_t)y & 1u) return set_error(INA_EINVAL, "16-bit buffers must be 2-byte aligned%s", "");
    const int vec = aligned16(sv) && aligned16(y);
    INA_X16_LAUNCH(ytype, k_dequantize_i32_x16, dim3(grid_of(vec ? n / 4 + 1 : n, ew_grid_cap())), dim3(kBlk), 0,
                   hs(stream), sv, static_cast<uint16_t*>(y), n, ldexpf(1.0f, -k), vec);
    return launched();
}

int ina_dequantize_i16_x16(const int16_t* sv, void* y, int ytype, size_t n, int k, ina_stream_t stream) {
    if (int rc = check_x16_type(ytype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!sv || !y) return set_error(INA_EINVAL, "null pointer%s", "");
    if ((uintptr_t)y & 1u) return set_error(INA_EINVAL, "16-bit buffers must be 2-byte aligned%s", "");
    const int vec = aligned16(sv) && aligned16(y);
    INA_X16_LAUNCH(ytype, k_dequantize_i16_x16, dim3(grid_of(vec ? n / 8 + 1 : n, ew_grid_cap())), dim3(kBlk), 0,
                   hs(stream), sv, static_cast<uint16_t*>(y), n, ldexpf(1.0f, -k), vec);
    return launched();
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_x16() { return take_store_violations(); }
#endif
