// ina_reduce_sr.hip -- stochastic rounding in the fused quantise + reduce calls (include/ina_reduce_sr.h
// states the contract): W workers' buckets, fp32 or bf16 / fp16, rounded without bias and summed in one
// launch -- configs 2 and 4, and the whole compute of layout B of config 5.
//
// Per element and worker, fp32, unfused: y_w = sr_y(bufs[w][e], 2^k, word) (ina_sr_device.h), word from
// Philox4x32-10 at the counter ((e0 + e) >> 2, step, sub + w), output word (e0 + e) & 3; then
// out = sum_w q32_of(y_w) mod 2^32, or sat16(sum_w q16_of(y_w)) with the slot flags (ina_device.h).  One
// Philox call serves the 4 values of a lane's chunk of one worker, so a chunk costs W calls; the calls of
// a chunk differ in counter word 3 alone, and once the W loop is unrolled the compiler keeps one copy of
// round 1's two products for all of them.  The kernels are ALU-bound: no scratch, no LDS, the key in
// scalar registers.
//
// Lane layouts (256-thread workgroups, non-temporal loads, stream_store at ascending lane addresses), the
// round-to-nearest siblings' with ina_sr.hip's chunk.  The grids are ina_sr.hip's, not the siblings': every
// one is under default_grid_cap() (tuning key 0, which the product build accepts, so a test reaches every
// grid-stride loop), where the int32 siblings cover the bucket for W <= 8.  At config 2's size a covering
// grid measured 0-5 % faster from fp32 buckets and the same from bf16.
//   int32 out: lane i owns chunk i of every worker -- W 16-byte (fp32) or 8-byte (bf16 / fp16) loads in
//     flight, W Philox calls, one 16-byte store; the ragged tail value by value.
//   int16 out: a wave owns 512 values, lane l the 4 at 4l of each 256-value half (2W Philox calls), two
//     8-byte stores, the slot flags from two wave ballots; a wave's last, short region value by value.
//   Misaligned buffers, and slot flags with a V that has no ballot layout: one value per lane, its own
//     Philox call per worker and the word picked by (e0 + e) & 3 -- identical results.
// W is a template argument at the siblings' specialisations (int32: 2, 4, 8, 16; int16: 1, 4, 8, 16),
// 0 for any other W up to INA_MAX_WORKERS (a run-time loop, one worker's chunk at a time).
#include <hip/hip_runtime.h>

#include <cmath>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"
#include "ina_sr_device.h"

namespace ina {
namespace {

constexpr int kBlk = kHostBlock;

// (stream_of, worker w's stream, and q16x4_add_sr are in ina_sr_device.h: the block-scaled instances of
// ina_blk.hip run the same ones)

// one value of the sum at element j, every worker: the value-by-value paths
template <typename X>
__device__ __forceinline__ uint32_t sum1_q32(const PtrPack<X>& in, int nw, size_t j, float s, const SrKey& a) {
    uint32_t acc = 0;
    for (int w = 0; w < nw; ++w) acc += (uint32_t)q32_of(sr_y(ld1(in.p[w], j), s, word_of(stream_of(a, w), j)));
    return acc;
}
template <typename X>
__device__ __forceinline__ int16_t sum1_q16(const PtrPack<X>& in, int nw, size_t j, float s, const SrKey& a,
                                            bool& sat) {
    int32_t acc = 0;
    for (int w = 0; w < nw; ++w) acc += q16_of(sr_y(ld1(in.p[w], j), s, word_of(stream_of(a, w), j)), sat);
    return (int16_t)sat16(acc, sat);
}

// int32 out.  vec: every buffer takes the chunk accesses.
template <typename X, int W>
__global__ __launch_bounds__(kBlk) void k_qr_sr_i32(PtrPack<X> in, int Wd, int32_t* __restrict__ out, size_t n,
                                                    float s, int vec, SrKey a) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const int nw = W > 0 ? W : Wd;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = tid; i < n4; i += stride) {
        const uint64_t idx = a.i0 + i;
        u32x4 acc = {0u, 0u, 0u, 0u};
        if constexpr (W > 0) {
            f32x4 v[W];
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = ld4(in.p[w], 4 * i, 4 * i + 4);
#pragma unroll
            for (int w = 0; w < W; ++w) acc += sr_q32x4(v[w], s, philox(stream_of(a, w), idx));
        } else {
            for (int w = 0; w < nw; ++w)
                acc += sr_q32x4(ld4(in.p[w], 4 * i, 4 * i + 4), s, philox(stream_of(a, w), idx));
        }
        stream_store(acc, reinterpret_cast<u32x4*>(out) + i);
    }
    for (size_t j = 4 * n4 + tid; j < n; j += stride) out[j] = (int32_t)sum1_q32(in, nw, j, s, a);
}

// the 4 sums of every worker's chunk at element e
template <typename X, int W>
__device__ __forceinline__ void sum4_q16(const PtrPack<X>& in, int nw, size_t e, float s, const SrKey& a,
                                         int32_t* acc, bool& sat) {
    const uint64_t idx = a.i0 + (e >> 2);
    if constexpr (W > 0) {
        f32x4 v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) v[w] = ld4(in.p[w], e, e + 4);
#pragma unroll
        for (int w = 0; w < W; ++w) q16x4_add_sr(v[w], s, philox(stream_of(a, w), idx), acc, sat);
    } else {
        for (int w = 0; w < nw; ++w) q16x4_add_sr(ld4(in.p[w], e, e + 4), s, philox(stream_of(a, w), idx), acc, sat);
    }
}
__device__ __forceinline__ u32x2 sat16x4(const int32_t* acc, bool& sat) {
    u32x2 o;
    o.x = (uint32_t)(uint16_t)sat16(acc[0], sat) | ((uint32_t)sat16(acc[1], sat) << 16);
    o.y = (uint32_t)(uint16_t)sat16(acc[2], sat) | ((uint32_t)sat16(acc[3], sat) << 16);
    return o;
}

// int16 out, every buffer aligned for the chunk accesses and V with a ballot layout (or no flags)
template <typename X, int W>
__global__ __launch_bounds__(kBlk) void k_qr_sr_i16_vec(PtrPack<X> in, int Wd, int16_t* __restrict__ out, size_t n,
                                                        float s, int V, uint8_t* __restrict__ ovf, SrKey a) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const int nw = W > 0 ? W : Wd;
    const int lane = (int)(tid & 63);
    const size_t nreg = (n + 511) / 512;
    for (size_t r = tid >> 6; r < nreg; r += stride >> 6) {      // wave-uniform trip count
        const size_t eA = r * 512 + 4 * (size_t)lane, eB = eA + 256;
        bool sa = false, sb = false;
        if (r * 512 + 512 <= n) {                 // wave-uniform
            int32_t accA[4] = {0, 0, 0, 0}, accB[4] = {0, 0, 0, 0};
            sum4_q16<X, W>(in, nw, eA, s, a, accA, sa);
            sum4_q16<X, W>(in, nw, eB, s, a, accB, sb);
            const u32x2 oa = sat16x4(accA, sa), ob = sat16x4(accB, sb);
            stream_store(oa, reinterpret_cast<u32x2*>(out + eA));
            stream_store(ob, reinterpret_cast<u32x2*>(out + eB));
        } else {
            for (size_t j = eA; j < eA + 4 && j < n; ++j) out[j] = sum1_q16(in, nw, j, s, a, sa);
            for (size_t j = eB; j < eB + 4 && j < n; ++j) out[j] = sum1_q16(in, nw, j, s, a, sb);
        }
        const unsigned long long ma = __ballot(sa), mb = __ballot(sb);   // wave-convergent
        if (ovf) write_slot_flags_split(ma, mb, eA, eB, n, V, ovf);
    }
}

// any alignment and any V: byte flags in a pre-zeroed array, benign same-value stores
template <typename X>
__global__ __launch_bounds__(kBlk) void k_qr_sr_i16_scalar(PtrPack<X> in, int W, int16_t* __restrict__ out, size_t n,
                                                           float s, int V, uint8_t* __restrict__ ovf, SrKey a) {
    const size_t stride = (size_t)gridDim.x * kBlk;
    for (size_t j = (size_t)blockIdx.x * kBlk + threadIdx.x; j < n; j += stride) {
        bool sat = false;
        out[j] = sum1_q16(in, W, j, s, a, sat);
        if (sat && ovf) ovf[j / (size_t)V] = 1;
    }
}

inline bool al(const void* p, unsigned a) { return ((uintptr_t)p % a) == 0; }
// every worker's buffer takes the chunk loads
template <typename X>
bool chunk_aligned(const PtrPack<X>& pk, int W) {
    for (int w = 0; w < W; ++w)
        if (!al(pk.p[w], 4 * sizeof(X))) return false;
    return true;
}

template <typename X>
int launch_i32(const PtrPack<X>& pk, int W, int32_t* out, size_t n, int k, const SrKey& a, ina_stream_t stream) {
    const int vec = chunk_aligned(pk, W) && al(out, 16);
    const dim3 g(grid_of(vec ? n / 4 + 1 : n, default_grid_cap())), b(kBlk);
    const float sc = ldexpf(1.0f, k);
    hipStream_t s = hs(stream);
    switch (W) {
        case 2: hipLaunchKernelGGL((k_qr_sr_i32<X, 2>), g, b, 0, s, pk, W, out, n, sc, vec, a); break;
        case 4: hipLaunchKernelGGL((k_qr_sr_i32<X, 4>), g, b, 0, s, pk, W, out, n, sc, vec, a); break;
        case 8: hipLaunchKernelGGL((k_qr_sr_i32<X, 8>), g, b, 0, s, pk, W, out, n, sc, vec, a); break;
        case 16: hipLaunchKernelGGL((k_qr_sr_i32<X, 16>), g, b, 0, s, pk, W, out, n, sc, vec, a); break;
        default: hipLaunchKernelGGL((k_qr_sr_i32<X, 0>), g, b, 0, s, pk, W, out, n, sc, vec, a);
    }
    return check_launch("quantize_reduce_sr_i32");
}

template <typename X>
int launch_i16(const PtrPack<X>& pk, int W, int16_t* out, size_t n, int k, int V, uint8_t* ovf, const SrKey& a,
               ina_stream_t stream) {
    hipStream_t s = hs(stream);
    const float sc = ldexpf(1.0f, k);
    if (chunk_aligned(pk, W) && al(out, 8) && (!ovf || slot_ballot_ok(V))) {
        const dim3 g(grid_of((n + 511) / 512 * 64, default_grid_cap())), b(kBlk);
        switch (W) {
            case 1: hipLaunchKernelGGL((k_qr_sr_i16_vec<X, 1>), g, b, 0, s, pk, W, out, n, sc, V, ovf, a); break;
            case 4: hipLaunchKernelGGL((k_qr_sr_i16_vec<X, 4>), g, b, 0, s, pk, W, out, n, sc, V, ovf, a); break;
            case 8: hipLaunchKernelGGL((k_qr_sr_i16_vec<X, 8>), g, b, 0, s, pk, W, out, n, sc, V, ovf, a); break;
            case 16: hipLaunchKernelGGL((k_qr_sr_i16_vec<X, 16>), g, b, 0, s, pk, W, out, n, sc, V, ovf, a); break;
            default: hipLaunchKernelGGL((k_qr_sr_i16_vec<X, 0>), g, b, 0, s, pk, W, out, n, sc, V, ovf, a);
        }
    } else {
        if (ovf && hipMemsetAsync(ovf, 0, (n + (size_t)V - 1) / (size_t)V, s) != hipSuccess)
            return set_error(INA_EHIP, "memset overflow flags%s", "");
        hipLaunchKernelGGL(k_qr_sr_i16_scalar<X>, dim3(grid_of(n, default_grid_cap())), dim3(kBlk), 0, s, pk, W, out, n,
                           sc, V, ovf, a);
    }
    return check_launch("quantize_reduce_sr_i16");
}

// the siblings' checks in their order, then the stochastic ones; bits: the width of out.  n == 0 has
// returned INA_OK before this is reached.
template <typename X, typename B>
int reduce(const B* const* bufs, int W, void* out, int bits, size_t n, int k, int V, uint8_t* ovf, const ina_sr_t* sr,
           ina_stream_t stream) {
    PtrPack<X> pk;
    bool all16;
    if (int rc = fill_pack(pk, bufs, W, all16)) return rc;
    if (!out) return set_error(INA_EINVAL, "null out%s", "");
    SrKey a;
    if (int rc = sr_key(sr, a)) return rc;
    if (bits == 32) return launch_i32(pk, W, static_cast<int32_t*>(out), n, k, a, stream);
    return launch_i16(pk, W, static_cast<int16_t*>(out), n, k, V, ovf, a, stream);
}

using bf16 = h16<INA_X16_BF16>;
using f16 = h16<INA_X16_F16>;

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

int ina_quantize_reduce_sr_f32_i32(const float* const* bufs, int W, int32_t* out, size_t n, int k,
                                   const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    return reduce<float>(bufs, W, out, 32, n, k, 0, nullptr, sr, stream);
}

int ina_quantize_reduce_sr_f32_i16_sat(const float* const* bufs, int W, int16_t* out, size_t n, int k, int V,
                                       uint8_t* ovf, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    return reduce<float>(bufs, W, out, 16, n, k, V, ovf, sr, stream);
}

int ina_quantize_reduce_sr_x16_i32(const void* const* bufs, int xtype, int W, int32_t* out, size_t n, int k,
                                   const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (xtype == INA_X16_BF16) return reduce<bf16>(bufs, W, out, 32, n, k, 0, nullptr, sr, stream);
    return reduce<f16>(bufs, W, out, 32, n, k, 0, nullptr, sr, stream);
}

int ina_quantize_reduce_sr_x16_i16_sat(const void* const* bufs, int xtype, int W, int16_t* out, size_t n, int k,
                                       int V, uint8_t* ovf, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    if (xtype == INA_X16_BF16) return reduce<bf16>(bufs, W, out, 16, n, k, V, ovf, sr, stream);
    return reduce<f16>(bufs, W, out, 16, n, k, V, ovf, sr, stream);
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_reduce_sr() { return take_store_violations(); }
#endif
