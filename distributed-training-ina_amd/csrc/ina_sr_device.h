// ina_sr_device.h -- the generator and the rounding step of stochastic rounding (include/ina_sr.h
// states the contract): the one copy, run by the quantisers of ina_sr.hip, by the stochastic worker
// packs of ina_kernels.hip (include/ina_pkt_sr.h), by the fused reduces of ina_reduce_sr.hip and by the
// stochastic instances of the block kernels of ina_blk.hip (include/ina_blk_sr.h).
//
// word is Philox4x32-10 under the key (seed) at the counter ((e0 + e) >> 2, step, sub), output word
// (e0 + e) & 3: one call serves the 4 values a lane owns, and e0 % 4 == 0 keeps a lane's chunk inside
// one call.  Philox is ten rounds of two 32 x 32 -> 64-bit multiplies and three XORs on four
// registers, the key in scalar registers: no scratch, no LDS.
#pragma once
#include "ina_internal.h"
#include "ina_chunk.h"

namespace ina {

// *sr as the kernels take it: the key, counter words 2 and 3, and e0 / 4 (the counter of chunk 0)
struct SrKey {
    uint32_t k0, k1, step, sub;
    uint64_t i0;
};

// Philox4x32-10 at counter (idx, step, sub)
__device__ __forceinline__ u32x4 philox(const SrKey& a, uint64_t idx) {
    uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = a.step, c3 = a.sub;
    uint32_t k0 = a.k0, k1 = a.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    return u32x4{c0, c1, c2, c3};
}
// the word of element e (its index in the bucket), for the value-by-value paths; picked with
// selects, so the four words stay in registers
__device__ __forceinline__ uint32_t word_of(const SrKey& a, size_t e) {
    const u32x4 w = philox(a, a.i0 + (e >> 2));
    const uint32_t lo = (e & 1) ? w.y : w.x, hi = (e & 1) ? w.w : w.z;
    return (e & 2) ? hi : lo;
}

// y of the contract: explicit roundings, no FMA
__device__ __forceinline__ float sr_y(float d, float s, uint32_t word) {
    const float t = __fmul_rn(d, s);
    const float f = __builtin_floorf(t);
    const float p = __fsub_rn(t, f);
    const float u = __fmul_rn((float)(word >> 8), 0x1p-24f);    // exact
    return __fadd_rn(f, u < p ? 1.0f : 0.0f);
}
__device__ __forceinline__ f32x4 sr_y4(f32x4 d, float s, u32x4 w) {
    return f32x4{sr_y(d.x, s, w.x), sr_y(d.y, s, w.y), sr_y(d.z, s, w.z), sr_y(d.w, s, w.w)};
}
// the int32 words of a chunk of deltas rounded with the words of one Philox call
__device__ __forceinline__ u32x4 sr_q32x4(f32x4 d, float s, u32x4 w) {
    const f32x4 y = sr_y4(d, s, w);
    return u32x4{(uint32_t)q32_of(y.x), (uint32_t)q32_of(y.y), (uint32_t)q32_of(y.z), (uint32_t)q32_of(y.w)};
}

// the int16 wire's words (q16 + (sat << 22)) of the same
__device__ __forceinline__ u32x4 sr_q16wx4(f32x4 d, float s, u32x4 w) {
    const f32x4 y = sr_y4(d, s, w);
    return u32x4{(uint32_t)q16w_of(y.x), (uint32_t)q16w_of(y.y), (uint32_t)q16w_of(y.z), (uint32_t)q16w_of(y.w)};
}
// one worker's chunk rounded with the words of one Philox call and added to the 4 widened int16 sums
__device__ __forceinline__ void q16x4_add_sr(f32x4 v, float s, u32x4 word, int32_t* acc, bool& sat) {
    const f32x4 y = sr_y4(v, s, word);
    acc[0] += q16_of(y.x, sat); acc[1] += q16_of(y.y, sat); acc[2] += q16_of(y.z, sat); acc[3] += q16_of(y.w, sat);
}
// worker w's stream of a fused call: counter word 3 is sub + w (mod 2^32)
__device__ __forceinline__ SrKey stream_of(const SrKey& a, int w) {
    SrKey b = a;
    b.sub = a.sub + (uint32_t)w;
    return b;
}

// the checks every stochastic call ends with, then *sr as the kernels take it
inline int sr_key(const ina_sr_t* sr, SrKey& a) {
    if (!sr) return set_error(INA_EINVAL, "null sr%s", "");
    if (sr->e0 & 3u) return set_error(INA_EINVAL, "e0 must be a multiple of 4%s", "");
    a = SrKey{(uint32_t)sr->seed, (uint32_t)(sr->seed >> 32), sr->step, sr->sub, sr->e0 >> 2};
    return INA_OK;
}

}  // namespace ina
