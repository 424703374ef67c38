// ina_sr.hip -- unbiased stochastic rounding for the global-k quantisers and the sharded int16 wire's
// (include/ina_sr.h states the contract).
//
// Per element, fp32, unfused:  t = (x - base) * 2^k,  f = floorf(t),  p = t - f,  u = float(word >> 8) *
// 2^-24,  y = f + (u < p),  q = the sibling's clamp / NaN handling of y (q32_of / q16_of / q16w_of,
// ina_device.h).  word is Philox4x32-10 under the key (seed) at the counter ((e0 + e) >> 2, step,
// sub), output word (e0 + e) & 3: one call serves the 4 values a lane owns, and e0 % 4 == 0 keeps a
// lane's chunk inside one call.  Philox is ten rounds of two 32 x 32 -> 64-bit multiplies and three
// XORs on four registers, the key in scalar registers: no scratch, no LDS.
//
// Lane layouts (256-thread workgroups, non-temporal loads, stream_store at ascending lane addresses,
// every grid under default_grid_cap()):
//   int32 out and the wire words: lane i owns chunk i -- one 16-byte (fp32) or 8-byte (bf16 / fp16)
//     load, one 16-byte store; the ragged tail value by value.
//   int16 out: the split layout of k_quantize_i16_vec -- a wave owns 512 values, lane l the 4 at 4l of
//     each 256-value half (two Philox calls), two 8-byte stores, the slot flags from two wave
//     ballots; a wave's last, short region value by value.
//   Misaligned buffers, and slot flags with a V that has no ballot layout: one value per lane, its
//     own Philox call and the word picked by (e0 + e) & 3 -- identical results.
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

// (SrKey, philox, word_of, sr_y, sr_y4 and the host's sr_key are in ina_sr_device.h: the stochastic
// worker packs of ina_kernels.hip run the same ones)

// a whole chunk of the delta at element e (checked against n by the caller), and one value of it
template <typename X>
__device__ __forceinline__ f32x4 ldd4(const X* x, const float* base, size_t e) {
    const f32x4 v = ld4(x, e, e + 4);
    return base ? sub4(v, ld4(base, e, e + 4)) : v;
}
template <typename X>
__device__ __forceinline__ float ldd1(const X* x, const float* base, size_t j) {
    const float v = ld1(x, j);
    return base ? __fsub_rn(v, base[j]) : v;
}

// int32 out (WIRE: the int16 wire's words).  vec: every buffer takes the chunk accesses.
template <typename X, bool WIRE>
__global__ __launch_bounds__(kBlk) void k_sr_i32(const X* __restrict__ x, const float* __restrict__ base,
                                                 int32_t* __restrict__ q, size_t n, float s, int vec, SrKey a) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = tid; i < n4; i += stride) {
        const f32x4 y = sr_y4(ldd4(x, base, 4 * i), s, philox(a, a.i0 + i));
        u32x4 r;
        if constexpr (WIRE)
            r = u32x4{(uint32_t)q16w_of(y.x), (uint32_t)q16w_of(y.y), (uint32_t)q16w_of(y.z), (uint32_t)q16w_of(y.w)};
        else
            r = u32x4{(uint32_t)q32_of(y.x), (uint32_t)q32_of(y.y), (uint32_t)q32_of(y.z), (uint32_t)q32_of(y.w)};
        stream_store(r, reinterpret_cast<u32x4*>(q) + i);
    }
    for (size_t j = 4 * n4 + tid; j < n; j += stride) {
        const float y = sr_y(ldd1(x, base, j), s, word_of(a, j));
        q[j] = WIRE ? q16w_of(y) : q32_of(y);
    }
}

// 4 values of the int16 layout at element e of a whole region: quantised, packed, sat |= any clamp / NaN
template <typename X>
__device__ __forceinline__ u32x2 sr_q16x4(const X* x, const float* base, size_t e, float s, const SrKey& a,
                                          bool& sat) {
    const f32x4 y = sr_y4(ldd4(x, base, e), s, philox(a, a.i0 + (e >> 2)));
    u32x2 o;
    o.x = (uint32_t)(uint16_t)q16_of(y.x, sat) | ((uint32_t)q16_of(y.y, sat) << 16);
    o.y = (uint32_t)(uint16_t)q16_of(y.z, sat) | ((uint32_t)q16_of(y.w, sat) << 16);
    return o;
}

// int16 out, every buffer aligned for the chunk accesses and V with a ballot layout (or no flags)
template <typename X>
__global__ __launch_bounds__(kBlk) void k_sr_i16_vec(const X* __restrict__ x, const float* __restrict__ base,
                                                     int16_t* __restrict__ q, size_t n, float s, int V,
                                                     uint8_t* __restrict__ ovf, SrKey a) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const int lane = (int)(tid & 63);
    const size_t nreg = (n + 511) / 512;
    for (size_t r = tid >> 6; r < nreg; r += stride >> 6) {      // wave-uniform trip count
        const size_t eA = r * 512 + 4 * (size_t)lane, eB = eA + 256;
        bool sa = false, sb = false;
        if (r * 512 + 512 <= n) {                 // wave-uniform
            const u32x2 oa = sr_q16x4(x, base, eA, s, a, sa);
            const u32x2 ob = sr_q16x4(x, base, eB, s, a, sb);
            stream_store(oa, reinterpret_cast<u32x2*>(q + eA));
            stream_store(ob, reinterpret_cast<u32x2*>(q + eB));
        } else {
            for (size_t j = eA; j < eA + 4 && j < n; ++j)
                q[j] = (int16_t)q16_of(sr_y(ldd1(x, base, j), s, word_of(a, j)), sa);
            for (size_t j = eB; j < eB + 4 && j < n; ++j)
                q[j] = (int16_t)q16_of(sr_y(ldd1(x, base, j), s, word_of(a, j)), sb);
        }
        const unsigned long long ma = __ballot(sa), mb = __ballot(sb);   // wave-convergent
        if (ovf) write_slot_flags_split(ma, mb, eA, eB, n, V, ovf);
    }
}

// any alignment and any V: byte flags in a pre-zeroed array, benign same-value stores
template <typename X>
__global__ __launch_bounds__(kBlk) void k_sr_i16_scalar(const X* __restrict__ x, const float* __restrict__ base,
                                                        int16_t* __restrict__ q, size_t n, float s, int V,
                                                        uint8_t* __restrict__ ovf, SrKey a) {
    const size_t stride = (size_t)gridDim.x * kBlk;
    for (size_t j = (size_t)blockIdx.x * kBlk + threadIdx.x; j < n; j += stride) {
        bool sat = false;
        q[j] = (int16_t)q16_of(sr_y(ldd1(x, base, j), s, word_of(a, j)), sat);
        if (sat && ovf) ovf[j / (size_t)V] = 1;
    }
}

inline bool al(const void* p, unsigned a) { return ((uintptr_t)p % a) == 0; }

template <typename X, bool WIRE>
int launch_i32(const X* x, const float* base, int32_t* q, size_t n, int k, const ina_sr_t* sr, ina_stream_t stream) {
    SrKey a;
    if (int rc = sr_key(sr, a)) return rc;
    const int vec = al(x, 4 * sizeof(X)) && al(q, 16) && (!base || al(base, 16));
    hipLaunchKernelGGL((k_sr_i32<X, WIRE>), dim3(grid_of(vec ? n / 4 + 1 : n, default_grid_cap())), dim3(kBlk), 0,
                       hs(stream), x, base, q, n, ldexpf(1.0f, k), vec, a);
    return check_launch(WIRE ? "quantize_sr_i16_wire" : "quantize_sr_i32");
}

template <typename X>
int launch_i16(const X* x, const float* base, int16_t* q, size_t n, int k, int V, uint8_t* ovf, const ina_sr_t* sr,
               ina_stream_t stream) {
    SrKey a;
    if (int rc = sr_key(sr, a)) return rc;
    hipStream_t s = hs(stream);
    const float sc = ldexpf(1.0f, k);
    if (al(x, 4 * sizeof(X)) && al(q, 8) && (!base || al(base, 16)) && (!ovf || slot_ballot_ok(V))) {
        hipLaunchKernelGGL(k_sr_i16_vec<X>, dim3(grid_of((n + 511) / 512 * 64, default_grid_cap())), dim3(kBlk), 0, s, x,
                           base, q, n, sc, V, ovf, a);
    } else {
        if (ovf && hipMemsetAsync(ovf, 0, (n + (size_t)V - 1) / (size_t)V, s) != hipSuccess)
            return set_error(INA_EHIP, "memset overflow flags%s", "");
        hipLaunchKernelGGL(k_sr_i16_scalar<X>, dim3(grid_of(n, default_grid_cap())), dim3(kBlk), 0, s, x, base, q, n, sc,
                           V, ovf, a);
    }
    return check_launch("quantize_sr_i16");
}

inline int check_al2(const void* p) {
    if ((uintptr_t)p & 1u) return set_error(INA_EINVAL, "16-bit buffers must be 2-byte aligned%s", "");
    return INA_OK;
}
using bf16 = h16<INA_X16_BF16>;
using f16 = h16<INA_X16_F16>;

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

int ina_quantize_sr_f32_i32(const float* x, const float* base, int32_t* q, size_t n, int k, const ina_sr_t* sr,
                            ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    return launch_i32<float, false>(x, base, q, n, k, sr, stream);
}

int ina_quantize_sr_f32_i16_sat(const float* x, const float* base, int16_t* q, size_t n, int k, int V, uint8_t* ovf,
                                const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    return launch_i16(x, base, q, n, k, V, ovf, sr, stream);
}

int ina_quantize_sr_x16_i32(const void* x, int xtype, const float* base, int32_t* q, size_t n, int k,
                            const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    if (int rc = check_al2(x)) return rc;
    if (xtype == INA_X16_BF16) return launch_i32<bf16, false>(static_cast<const bf16*>(x), base, q, n, k, sr, stream);
    return launch_i32<f16, false>(static_cast<const f16*>(x), base, q, n, k, sr, stream);
}

int ina_quantize_sr_x16_i16_sat(const void* x, int xtype, const float* base, int16_t* q, size_t n, int k, int V,
                                uint8_t* ovf, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    if (int rc = check_al2(x)) return rc;
    if (xtype == INA_X16_BF16) return launch_i16(static_cast<const bf16*>(x), base, q, n, k, V, ovf, sr, stream);
    return launch_i16(static_cast<const f16*>(x), base, q, n, k, V, ovf, sr, stream);
}

int ina_quantize_sr_f32_i16_wire(const float* x, int32_t* wire, size_t n, int k, const ina_sr_t* sr,
                                 ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !wire) return set_error(INA_EINVAL, "null pointer%s", "");
    return launch_i32<float, true>(x, nullptr, wire, n, k, sr, stream);
}

int ina_quantize_sr_x16_i16_wire(const void* x, int xtype, int32_t* wire, size_t n, int k, const ina_sr_t* sr,
                                 ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !wire) return set_error(INA_EINVAL, "null pointer%s", "");
    if (int rc = check_al2(x)) return rc;
    if (xtype == INA_X16_BF16) return launch_i32<bf16, true>(static_cast<const bf16*>(x), nullptr, wire, n, k, sr, stream);
    return launch_i32<f16, true>(static_cast<const f16*>(x), nullptr, wire, n, k, sr, stream);
}

int ina_scale_for_sr(float absmax, int W, int bits, int* k_out) {
    return scale_for_round(absmax, W, bits, 1.0, k_out);
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_sr() { return take_store_violations(); }
#endif
