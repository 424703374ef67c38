// ina_rot_device.h -- the randomised Hadamard rotation of a block held in V/4 adjacent lanes of one wave
// (include/ina_rot.h states the contract): the signs, the m butterfly stages and the two normalisations.
//
// A lane holds the chunk t = (t0, t1, t2, t3) of 4 adjacent values; lane l of a group holds values
// 4l .. 4l+3 of the block.  Stage i pairs value j with j + 2^i:
//   stages 0, 1   inside the chunk: 8 adds.
//   stage i >= 2  with lane l ^ (1 << (i - 2)): the lane whose bit is clear keeps own + partner, the other
//                 partner - own.  Every add is one fp32 round-to-nearest add of the contract's two operands,
//                 so the result does not depend on which instruction moved them:
//     xor 1, 2    quad-perm DPP folded into the add: r = (upper ? -own : own) + dpp(own).  The negation is
//                 one v_xor with a per-lane mask (x + (-y) is x - y bit for bit); 2 VALU a value.
//     xor 8       the same with row_ror:8 (a rotation by 8 in a row of 16 is lane ^ 8).
//     xor 4       no single DPP control is lane ^ 4.  Two values a and b of the lane trade places instead:
//                 bank-masked row_shr:4 / row_shl:4 moves leave the lower lane with a of both lanes and the
//                 upper lane with b of both, one add and one subtract serve both pairs, and the same two
//                 moves carry the results home; 6 VALU for 2 values.
//     xor 16, 32  the same trade with gfx950's v_permlane16_swap / v_permlane32_swap, which exchange the
//                 odd rows (the upper half) of one register with the even rows (the lower half) of another:
//                 swap, add, subtract, swap; 4 VALU for 2 values, no LDS and no bpermute.
// All exchanges are compiler builtins (update_dpp, permlane*_swap), so the compiler owns their wait states.
// Every lane of the wave must reach rot_stages: callers loop with wave-uniform trip counts and lanes past n
// carry zeros.  `shift` (log2 V - 2, the number of cross-lane stages) is wave-uniform: its branches are
// scalar.
//
// Signs: the 256 values a wave holds in one pass start at a stream index that is a multiple of 128, so
// their 256 sign bits are the 8 output words of two Philox calls at wave-uniform counters.  The counter is
// passed through readfirstlane, which lets the compiler run both calls on the scalar unit (s_mul_i32 /
// s_mul_hi_u32); a lane then selects its word (lane >> 3) and extracts its 4 bits (4 * (lane & 7)).
#pragma once
#include "ina_chunk.h"
#include "ina_sr_device.h"

namespace ina {

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "v_permlane16_swap / v_permlane32_swap are gfx950 instructions"
#endif

// *sr as the rotating kernels take it: the key, counter words 2 and 3, and e0 / 128 (the counter of value 0)
inline int rot_key(const ina_sr_t* sr, int V, SrKey& a) {
    if (!sr) return set_error(INA_EINVAL, "null sr%s", "");
    if (sr->e0 % 128u || sr->e0 % (uint64_t)V) return set_error(INA_EINVAL, "e0 must be a multiple of 128 and of V%s", "");
    a = SrKey{(uint32_t)sr->seed, (uint32_t)(sr->seed >> 32), sr->step, sr->sub, sr->e0 >> 7};
    return INA_OK;
}

__device__ __forceinline__ uint64_t wave_uniform(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
}

// the sign-bit masks (0 or 0x80000000) of the lane's chunk; e256: the wave-uniform index in the bucket of
// the first of the wave's 256 values (a multiple of 256)
__device__ __forceinline__ u32x4 rot_signs(const SrKey& key, size_t e256, int lane) {
    const uint64_t c = key.i0 + wave_uniform((uint64_t)e256 >> 7);
    const u32x4 a = philox(key, c), b = philox(key, c + 1);            // lanes 0-31, lanes 32-63
    const int j = lane >> 3;
    const uint32_t w01 = (j & 1) ? a.y : a.x, w23 = (j & 1) ? a.w : a.z;
    const uint32_t w45 = (j & 1) ? b.y : b.x, w67 = (j & 1) ? b.w : b.z;
    const uint32_t lo = (j & 2) ? w23 : w01, hi = (j & 2) ? w67 : w45;
    const uint32_t nib = __builtin_amdgcn_ubfe((j & 4) ? hi : lo, 4u * (uint32_t)(lane & 7), 4u);
    return u32x4{nib << 31, (nib << 30) & 0x80000000u, (nib << 29) & 0x80000000u, (nib << 28) & 0x80000000u};
}
__device__ __forceinline__ float flip(float v, uint32_t mask) { return __uint_as_float(__float_as_uint(v) ^ mask); }
__device__ __forceinline__ f32x4 flip4(f32x4 v, u32x4 sg) {
    return f32x4{flip(v.x, sg.x), flip(v.y, sg.y), flip(v.z, sg.z), flip(v.w, sg.w)};
}

// DPP controls: quad_perm [1,0,3,2] and [2,3,0,1], row_shl:4, row_shr:4, row_ror:8
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppShl4 = 0x104, kDppShr4 = 0x114, kDppRor8 = 0x128;

// a stage whose partner a single full-wave DPP control reaches; neg: 0x80000000 in the upper lane, else 0
template <int CTRL>
__device__ __forceinline__ float dpp_stage1(float own, uint32_t neg) {
    const float p = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(own), CTRL, 0xf, 0xf, true));
    return __fadd_rn(flip(own, neg), p);
}
template <int CTRL>
__device__ __forceinline__ f32x4 dpp_stage(f32x4 t, uint32_t neg) {
    return f32x4{dpp_stage1<CTRL>(t.x, neg), dpp_stage1<CTRL>(t.y, neg), dpp_stage1<CTRL>(t.z, neg),
                 dpp_stage1<CTRL>(t.w, neg)};
}
// old where the bank mask leaves a lane out, else src moved by CTRL
template <int CTRL, int BANKS>
__device__ __forceinline__ float dpp_into(float old, float src) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, 0xf, BANKS, false));
}
// lane ^ 4 for two values of the lane: banks 0 and 2 (0x5) are the lower lanes, banks 1 and 3 (0xa) the upper
__device__ __forceinline__ void trade4_stage(float& a, float& b) {
    const float lo = dpp_into<kDppShr4, 0xa>(a, b);      // lower lane: own a; upper: the lower lane's b
    const float hi = dpp_into<kDppShl4, 0x5>(b, a);      // lower lane: the upper lane's a; upper: own b
    const float s = __fadd_rn(lo, hi), d = __fsub_rn(lo, hi);
    a = dpp_into<kDppShr4, 0xa>(s, d);
    b = dpp_into<kDppShl4, 0x5>(d, s);
}
// lane ^ 16 and lane ^ 32 likewise: {a', b'} = swap(a, b) leaves a of both lanes in the lower lane, b of
// both in the upper one
template <int H>
__device__ __forceinline__ void swap_stage(float& a, float& b) {
    static_assert(H == 16 || H == 32, "rows of 16 or halves of 32");
    auto swp = [](float x, float y) {
        if constexpr (H == 16) return __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
        else return __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    };
    const auto p = swp(a, b);
    const float lo = __uint_as_float(p[0]), hi = __uint_as_float(p[1]);
    const auto q = swp(__fadd_rn(lo, hi), __fsub_rn(lo, hi));
    a = __uint_as_float(q[0]);
    b = __uint_as_float(q[1]);
}

// the m = shift + 2 stages of the contract, in its order
__device__ __forceinline__ f32x4 rot_stages(f32x4 t, int shift, int lane) {
    const float a = __fadd_rn(t.x, t.y), b = __fsub_rn(t.x, t.y), c = __fadd_rn(t.z, t.w), d = __fsub_rn(t.z, t.w);
    t = f32x4{__fadd_rn(a, c), __fadd_rn(b, d), __fsub_rn(a, c), __fsub_rn(b, d)};
    const uint32_t l = (uint32_t)lane;
    if (shift >= 1) t = dpp_stage<kDppXor1>(t, (l & 1u) << 31);
    if (shift >= 2) t = dpp_stage<kDppXor2>(t, (l & 2u) << 30);
    float x = t.x, y = t.y, z = t.z, w = t.w;          // (a vector's elements do not bind to references)
    if (shift >= 3) {
        trade4_stage(x, y);
        trade4_stage(z, w);
    }
    if (shift >= 4) {
        const f32x4 r = dpp_stage<kDppRor8>(f32x4{x, y, z, w}, (l & 8u) << 28);
        x = r.x, y = r.y, z = r.z, w = r.w;
    }
    if (shift >= 5) {
        swap_stage<16>(x, y);
        swap_stage<16>(z, w);
    }
    if (shift >= 6) {
        swap_stage<32>(x, y);
        swap_stage<32>(z, w);
    }
    return f32x4{x, y, z, w};
}

// 2^-ceil(m/2) and 2^-floor(m/2) for m = shift + 2
__device__ __forceinline__ float rot_fwd_norm(int shift) { return pow2f(-((shift + 3) >> 1)); }
__device__ __forceinline__ float rot_inv_norm(int shift) { return pow2f(-((shift + 2) >> 1)); }
__device__ __forceinline__ f32x4 mul4(f32x4 v, float s) {
    return f32x4{__fmul_rn(v.x, s), __fmul_rn(v.y, s), __fmul_rn(v.z, s), __fmul_rn(v.w, s)};
}

// r of the contract from the chunk x; sg: the chunk's sign masks
__device__ __forceinline__ f32x4 rot_fwd(f32x4 x, u32x4 sg, int shift, int lane) {
    return mul4(rot_stages(flip4(x, sg), shift, lane), rot_fwd_norm(shift));
}
// xhat of the contract from the chunk y = float(sum) * 2^-k
__device__ __forceinline__ f32x4 rot_inv(f32x4 y, u32x4 sg, int shift, int lane) {
    return flip4(mul4(rot_stages(y, shift, lane), rot_inv_norm(shift)), sg);
}

}  // namespace ina
