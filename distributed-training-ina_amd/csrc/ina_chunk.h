// ina_chunk.h -- a lane's chunk of 4 values: the one copy of its loads, stores, quantise steps and
// of the error-feedback step, shared by ina_blk.hip, ina_x16.hip and the packs of ina_kernels.hip.
#pragma once
#include "ina_device.h"

namespace ina {

using u32x4 = u32x4_t;
using u32x2 = u32x2_t;
using f32x4 = f32x4_t;

// one bf16 / fp16 value of a bucket (X of a kernel: float, or h16<XT>)
template <int XT>
struct h16 {
    uint16_t v;
};

// ---------------------------------------------------------------------------
// the chunk at element e; a chunk that crosses n is read and written value by value (values past n
// read as 0)
// ---------------------------------------------------------------------------
template <bool NT = true>
__device__ __forceinline__ f32x4 ld4(const float* p, size_t e, size_t n) {
    if (e + 4 <= n) {
        if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + e));
        else return *reinterpret_cast<const f32x4*>(p + e);
    }
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (e < n) v.x = p[e];
    if (e + 1 < n) v.y = p[e + 1];
    if (e + 2 < n) v.z = p[e + 2];
    return v;
}
// a bf16 / fp16 bucket (include/ina_x16_blk.h): one 8-byte load, widened in registers (exact)
template <int XT>
__device__ __forceinline__ f32x4 ld4(const h16<XT>* p, size_t e, size_t n) {
    if (e + 4 <= n) return widen16x4<XT>(__builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p + e)));
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (e < n) v.x = widen16<XT>(p[e].v);
    if (e + 1 < n) v.y = widen16<XT>(p[e + 1].v);
    if (e + 2 < n) v.z = widen16<XT>(p[e + 2].v);
    return v;
}
// one value of a bucket, and one decoded value into one (16-bit: rounded once to nearest even)
__device__ __forceinline__ float ld1(const float* p, size_t j) { return p[j]; }
template <int XT>
__device__ __forceinline__ float ld1(const h16<XT>* p, size_t j) { return widen16<XT>(p[j].v); }
__device__ __forceinline__ void st1(float v, float* p, size_t j) { p[j] = v; }
template <int XT>
__device__ __forceinline__ void st1(float v, h16<XT>* p, size_t j) { p[j].v = (uint16_t)rne16<XT>(v); }
__device__ __forceinline__ u32x4 ld4i(const int32_t* p, size_t e, size_t n) {
    if (e + 4 <= n) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + e));
    u32x4 v = {0u, 0u, 0u, 0u};
    if (e < n) v.x = (uint32_t)p[e];
    if (e + 1 < n) v.y = (uint32_t)p[e + 1];
    if (e + 2 < n) v.z = (uint32_t)p[e + 2];
    return v;
}
// 4 int16 values, sign-extended
__device__ __forceinline__ u32x4 ld4h(const int16_t* p, size_t e, size_t n) {
    if (e + 4 <= n) {
        const u32x2 h = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p + e));
        return u32x4{(uint32_t)(int32_t)(int16_t)(h.x & 0xFFFFu), (uint32_t)((int32_t)h.x >> 16),
                     (uint32_t)(int32_t)(int16_t)(h.y & 0xFFFFu), (uint32_t)((int32_t)h.y >> 16)};
    }
    u32x4 v = {0u, 0u, 0u, 0u};
    if (e < n) v.x = (uint32_t)(int32_t)p[e];
    if (e + 1 < n) v.y = (uint32_t)(int32_t)p[e + 1];
    if (e + 2 < n) v.z = (uint32_t)(int32_t)p[e + 2];
    return v;
}
// (the element is passed by value: __builtin_bit_cast applied to a vector element itself reads
// element 0 whichever is named)
template <typename T, typename S>
__device__ __forceinline__ T bits_as(S s) {
    return __builtin_bit_cast(T, s);
}
template <typename V4, typename T>
__device__ __forceinline__ void st4(V4 v, T* p, size_t e, size_t n) {
    static_assert(sizeof(V4) == 4 * sizeof(T), "4 values");
    if (e + 4 <= n) {
        stream_store(v, reinterpret_cast<V4*>(p + e));
    } else {
        if (e < n) p[e] = bits_as<T>(v.x);
        if (e + 1 < n) p[e + 1] = bits_as<T>(v.y);
        if (e + 2 < n) p[e + 2] = bits_as<T>(v.z);
    }
}
// 4 decoded values into a 16-bit buffer: one 8-byte store
template <int XT>
__device__ __forceinline__ void st4(f32x4 v, h16<XT>* p, size_t e, size_t n) {
    if (e + 4 <= n) {
        stream_store(u32x2{rne16x2<XT>(v.x, v.y), rne16x2<XT>(v.z, v.w)}, reinterpret_cast<u32x2*>(p + e));
    } else {
        if (e < n) st1(v.x, p, e);
        if (e + 1 < n) st1(v.y, p, e + 1);
        if (e + 2 < n) st1(v.z, p, e + 2);
    }
}
// 4 int16 (held widened) as one 8-byte store
__device__ __forceinline__ void st4h(const int32_t* a, int16_t* p, size_t e, size_t n) {
    if (e + 4 <= n) {
        u32x2 o;
        o.x = (uint32_t)(uint16_t)a[0] | ((uint32_t)a[1] << 16);
        o.y = (uint32_t)(uint16_t)a[2] | ((uint32_t)a[3] << 16);
        stream_store(o, reinterpret_cast<u32x2*>(p + e));
    } else {
        for (int j = 0; j < 3; ++j)
            if (e + j < n) p[e + j] = (int16_t)a[j];
    }
}

// ---------------------------------------------------------------------------
// the chunk's arithmetic: explicit roundings, no FMA
// ---------------------------------------------------------------------------
__device__ __forceinline__ u32x4 q32x4(f32x4 v, float s) {
    return u32x4{(uint32_t)q32(v.x, s), (uint32_t)q32(v.y, s), (uint32_t)q32(v.z, s), (uint32_t)q32(v.w, s)};
}
// the sharded int16 wire's words (q16w), and the q16 of each back out of them
__device__ __forceinline__ u32x4 q16wx4(f32x4 v, float s) {
    return u32x4{(uint32_t)q16w(v.x, s), (uint32_t)q16w(v.y, s), (uint32_t)q16w(v.z, s), (uint32_t)q16w(v.w, s)};
}
__device__ __forceinline__ u32x4 wire_q16x4(u32x4 w) {
    return u32x4{(uint32_t)wire_q16((int32_t)w.x), (uint32_t)wire_q16((int32_t)w.y),
                 (uint32_t)wire_q16((int32_t)w.z), (uint32_t)wire_q16((int32_t)w.w)};
}
// (int16 sums are held widened, as int32_t[4])
__device__ __forceinline__ void q16x4_add(f32x4 v, float s, int32_t* a, bool& sat) {
    a[0] += q16(v.x, s, sat); a[1] += q16(v.y, s, sat); a[2] += q16(v.z, s, sat); a[3] += q16(v.w, s, sat);
}
__device__ __forceinline__ f32x4 deq4(u32x4 q, float inv) {
    return f32x4{__fmul_rn((float)(int32_t)q.x, inv), __fmul_rn((float)(int32_t)q.y, inv),
                 __fmul_rn((float)(int32_t)q.z, inv), __fmul_rn((float)(int32_t)q.w, inv)};
}
// local + ws * y, the PS update's unfused fp32 sequence
__device__ __forceinline__ f32x4 upd4(f32x4 l, f32x4 y, float ws) {
    return f32x4{__fadd_rn(l.x, __fmul_rn(y.x, ws)), __fadd_rn(l.y, __fmul_rn(y.y, ws)),
                 __fadd_rn(l.z, __fmul_rn(y.z, ws)), __fadd_rn(l.w, __fmul_rn(y.w, ws))};
}
// a worker's delta x - b
__device__ __forceinline__ f32x4 sub4(f32x4 a, f32x4 b) {
    return f32x4{__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z), __fsub_rn(a.w, b.w)};
}

// The error-feedback step (include/ina_ef.h).  v = d + r, d the worker's delta x - base (x where
// the call has no base); r' = isfinite(v) ? v - float(q) * 2^-k : +0 once v is quantised to q.
__device__ __forceinline__ float ef_v(float d, float r) { return __fadd_rn(d, r); }
__device__ __forceinline__ f32x4 ef_v4(f32x4 d, f32x4 r) {
    return f32x4{ef_v(d.x, r.x), ef_v(d.y, r.y), ef_v(d.z, r.z), ef_v(d.w, r.w)};
}
__device__ __forceinline__ float ef_r(float v, int32_t q, float inv) {
    const bool finite = (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u;
    return finite ? __fsub_rn(v, __fmul_rn((float)q, inv)) : 0.0f;
}
__device__ __forceinline__ f32x4 ef_r4(f32x4 v, u32x4 q, float inv) {
    return f32x4{ef_r(v.x, (int32_t)q.x, inv), ef_r(v.y, (int32_t)q.y, inv), ef_r(v.z, (int32_t)q.z, inv),
                 ef_r(v.w, (int32_t)q.w, inv)};
}

}  // namespace ina
