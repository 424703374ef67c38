// ina_i8_device.h -- what the byte wire's sources share (ina_i8.hip, ina_i8_ef.hip, ina_i8_sr.hip): the lanes'
// loop, the scale rule's limits and host loop, the byte quantiser of a lane's chunk, and the block calls' host
// checks and scales dispatch.
#pragma once
#include <cmath>

#include "ina_internal.h"
#include "ina_chunk.h"

namespace ina {

constexpr int kI8Blk = 256;
constexpr double kLimI8 = 126.5;   // ina_scale_for_i8: absmax * 2^k + 1/2 <= 127
constexpr double kLimI8Sr = 126.0; // ina_scale_for_i8_sr: absmax * 2^k + 1 <= 127 (include/ina_i8_sr.h)

// chunk i = values 4i..4i+3; base_ is the wave's first chunk (a multiple of 64)
#define INA_I8_QUAD_LOOP(nq)                                       \
    const size_t tid_ = (size_t)blockIdx.x * kI8Blk + threadIdx.x; \
    const size_t stride_ = (size_t)gridDim.x * kI8Blk;             \
    for (size_t base_ = tid_ & ~(size_t)63; base_ < (nq); base_ += stride_)

// clamp(y, -127, 127) as an int; NaN -> 0; sat |= clamped or NaN
__device__ __forceinline__ int q8_of(float y, bool& sat) {
    const float c = __builtin_amdgcn_fmed3f(y, -127.0f, 127.0f);       // one v_med3_f32
    sat |= !(c == y);
    return (y != y) ? 0 : (int)c;
}
__device__ __forceinline__ float q8_round(float v, float s) { return __builtin_rintf(__fmul_rn(v, s)); }
// 4 values in [-128, 127] as 4 bytes, the first in the low byte: two v_cvt_pk_i16_i32 and one v_perm_b32
__device__ __forceinline__ uint32_t q8_pack(int a, int b, int c, int d) {
    const uint32_t lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(a, b));
    const uint32_t hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(c, d));
    return __builtin_amdgcn_perm(hi, lo, 0x06040200u);                 // the low byte of each int16
}
// clamp(rne(v * s), -127, 127) of 4 values as 4 bytes; NaN -> 0; sat |= clamped or NaN
__device__ __forceinline__ uint32_t q8x4(f32x4 v, float s, bool& sat) {
    const int a = q8_of(q8_round(v.x, s), sat), b = q8_of(q8_round(v.y, s), sat);
    const int c = q8_of(q8_round(v.z, s), sat), d = q8_of(q8_round(v.w, s), sat);
    return q8_pack(a, b, c, d);
}

// ---------------------------------------------------------------------------
// host side: the block calls' checks and the dispatch on the bucket's type
// ---------------------------------------------------------------------------
using bf16_t = h16<INA_X16_BF16>;
using fp16_t = h16<INA_X16_F16>;

inline int check_xtype(int xtype) {
    if (xtype == INA_ROT_F32 || xtype == INA_X16_BF16 || xtype == INA_X16_F16) return INA_OK;
    return set_error(INA_EINVAL, "xtype must be INA_ROT_F32 (0), INA_X16_BF16 (1) or INA_X16_F16 (2)%s", "");
}
inline int misaligned() { return set_error(INA_EINVAL, "buffers must be 16-byte aligned%s", ""); }

// the block calls' checks up to n == 0, in the header's order; shift = log2(V) - 2
inline int check_blocks(int V, const int8_t* kblk, size_t n, int& shift) {
    if (!vec_v(V, shift)) return set_error(INA_EINVAL, "V must be a power of two in [8, 256]%s", "");
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    if (n % (size_t)V) return set_error(INA_EINVAL, "n must be a multiple of V%s", "");
    return INA_OK;
}

// the host scale rule under a limit: the largest k in [-126, 127] with absmax * 2^k <= lim
inline int scale_for_lim(float absmax, int* k_out, double lim) {
    if (!k_out) return set_error(INA_EINVAL, "null k_out%s", "");
    if (!(absmax >= 0.0f) || std::isinf(absmax)) return set_error(INA_EINVAL, "absmax must be finite and >= 0%s", "");
    int k = 127;
    if (absmax != 0.0f)                                 // exact: a float times a power of two, as a double
        while (k > -126 && (double)absmax * std::ldexp(1.0, k) > lim) --k;
    *k_out = k;
    return INA_OK;
}
// ina_block_scales_i8 under the limit `lim` (ina_i8.hip: the checks, then k_i8_scales)
int block_scales_i8(const void* const* xs, int xtype, int W, size_t n, int V, int8_t* kblk, const ina_sr_t* sr,
                    double lim, ina_stream_t stream);

#define INA_I8_X_CALL(xtype, F, ...)                           \
    ((xtype) == INA_X16_BF16  ? F<bf16_t>(__VA_ARGS__)         \
     : (xtype) == INA_X16_F16 ? F<fp16_t>(__VA_ARGS__)         \
                              : F<float>(__VA_ARGS__))

}  // namespace ina
