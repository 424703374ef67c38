// ina_i8_sum_device.h -- what the byte wire's requantising slice sums share (ina_i8_gather.hip, ina_i8_sr.hip):
// the loads and the byte adds into 16-bit fields, the block maximum in packed 16-bit arithmetic and row-level DPP,
// and the host checks of the sum's arguments.
#pragma once
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"
#include "ina_rot_device.h"

namespace ina {

constexpr uint32_t kTop16 = 0x80008000u, kLow8 = 0x00FF00FFu;
// DPP controls beyond ina_rot_device.h's: a row of 16 reversed, each half row of 8 reversed
constexpr int kDppRowMirror = 0x140, kDppHalfMirror = 0x141;

typedef int16_t s16x2 __attribute__((ext_vector_type(2)));   // the two 16-bit fields of a word
__device__ __forceinline__ s16x2 fields(uint32_t w) { return __builtin_bit_cast(s16x2, w); }
__device__ __forceinline__ uint32_t word(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }

// the lane's chunk i of B slices: a whole chunk is one 16-byte load; the half chunk of a V = 8 tail is 8 bytes
// and 8 zeros; a lane past n holds zeros
template <int B>
__device__ __forceinline__ void ld_chunks(const PtrPack<int8_t>& in, int g0, size_t i, size_t nfull, bool half,
                                          u32x4* w) {
    if (i < nfull) {
#pragma unroll
        for (int j = 0; j < B; ++j) w[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in.p[g0 + j]) + i);
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j) w[j] = u32x4{0u, 0u, 0u, 0u};
        if (half) {
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const u32x2 h = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(in.p[g0 + j] + 16 * i));
                w[j].x = h.x;
                w[j].y = h.y;
            }
        }
    }
}
__device__ __forceinline__ void add_bytes(u32x4 w, u32x4& ev, u32x4& od) {
    w ^= 0x80808080u;
    ev += w & kLow8;
    od += (w >> 8) & kLow8;
}

// max |field| over 4 words, as one number
__device__ __forceinline__ int absmax4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    auto ab = [](uint32_t w) { return __builtin_elementwise_abs(fields(w)); };
    const s16x2 m = __builtin_elementwise_max(__builtin_elementwise_max(ab(a), ab(b)),
                                              __builtin_elementwise_max(ab(c), ab(d)));
    return max((int)m.x, (int)m.y);
}
template <int CTRL>
__device__ __forceinline__ int dpp_max(int m) {
    return max(m, __builtin_amdgcn_update_dpp(0, m, CTRL, 0xf, 0xf, true));
}
// the max over the 1 << steps adjacent lanes of a group (steps <= 4: inside one row); every lane of the wave
// must reach it; steps is wave-uniform
__device__ __forceinline__ int row_group_max(int m, int steps) {
    if (steps >= 1) m = dpp_max<kDppXor1>(m);
    if (steps >= 2) m = dpp_max<kDppXor2>(m);
    if (steps >= 3) m = dpp_max<kDppHalfMirror>(m);
    if (steps >= 4) m = dpp_max<kDppRowMirror>(m);
    return m;
}
// ---------------------------------------------------------------------------
// host side: the sum's checks in the header's order; lv = log2 V.  INA_OK with n == 0 is the no-op
// ---------------------------------------------------------------------------
inline int check_sum_rq(const int8_t* const* slices, int G, int V, const int8_t* q8, const uint8_t* shift, size_t n,
                        PtrPack<int8_t>& pk, int& lv) {
    if (!slices || G < 1 || G > INA_MAX_WORKERS) return set_error(INA_EINVAL, "G must be in [1, %s]", "64");
    int qs;                                             // log2(V) - 2
    if (!vec_v(V, qs)) return set_error(INA_EINVAL, "V must be a power of two in [8, 256]%s", "");
    lv = qs + 2;
    if (!shift) return set_error(INA_EINVAL, "null shift%s", "");
    if (n % (size_t)V) return set_error(INA_EINVAL, "n must be a multiple of V%s", "");
    if (n == 0) return INA_OK;
    bool al;
    if (int rc = fill_pack(pk, slices, G, al)) return rc;
    if (!q8) return set_error(INA_EINVAL, "null q8%s", "");
    if (!al || !aligned16(q8)) return set_error(INA_EINVAL, "buffers must be 16-byte aligned%s", "");
    return INA_OK;
}

}  // namespace ina
