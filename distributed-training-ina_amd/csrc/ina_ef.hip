// ina_ef.hip -- error feedback for the quantiser (include/ina_ef.h states the contract): the
// residual a worker carries from step to step is added, the sum quantised and the new residual
// written back in the quantiser's own launch.
//
// Per element, fp32, unfused:  v = (x - base) + r,  q = Q(v, k),  r' = isfinite(v) ? v - float(q) *
// 2^-k : +0.  Q is the siblings' quantiser (q32 / q16, ina_device.h) and float(q) * 2^-k their
// dequantiser's arithmetic, so every result is the siblings' on v, and with r = 0 on x - base.
// Composed from the existing ops the step is four launches and 36 bytes a value on the int16
// wire; here it is one launch and 14 (x 4, r 4, q 2, r' 4).
//
// Lane layout (vector path, 256-thread workgroups, non-temporal loads of x and r, the shared base
// with the default policy as in the packs, write-through stores of q and r' -- a non-temporal r' is
// not measured).  A lane always holds 4 values, so r and r' are 16-byte accesses whatever x and q
// are, and a block of V values is V/4 adjacent lanes of one wave:
//   int32 out: lane l of a wave owns values 4l..4l+3 of the wave's 256 (16-byte q store).
//   int16 out: the INA_Q16_SPLIT layout of the siblings -- a wave owns 512 values as two 256-value
//     halves, lane l the 4 at 4l of each half, one 8-byte q store per half; each half has its own
//     group, scale and flag ballot.
//   16-bit sources: the same lanes, one 8-byte load of x per 4 values, widened in registers.
// A chunk that crosses n is read and written value by value (values past n read as 0 and are not
// written).  Every loop has a wave-uniform trip count: lanes past n take part in the block max
// (AUTO) and the flag ballots with 0 / false.  A lane reads its r before it writes r', and no other
// lane touches those 16 bytes, so the update is in place.
//
// One kernel per output width serves the global-k calls (KG), given block scales (KGIVEN) and
// scales computed in the launch from |v| (KAUTO: the block's max is the cross-lane unsigned max of
// the fp32 bit patterns, ina_blk.hip's butterfly; the lane's chunks stay in registers between the
// max and the quantiser, so nothing is read twice).
//
// Scalar path (unaligned buffers, a V without a ballot layout): one wave per block of V values
// (the global-k int32 call: per 256), lanes striding over the block, the same helpers, identical
// results; the block's flag is one ballot, so nothing is pre-zeroed.
//
// The EF worker packs are instances of the split multi pack kernels of ina_kernels.hip (their EF
// template parameter); their entry points are there.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"

namespace ina {
namespace {

using u32x4 = u32x4_t;
using u32x2 = u32x2_t;
using f32x4 = f32x4_t;

constexpr int kBlk = kHostBlock;

enum { KG, KGIVEN, KAUTO };      // where k comes from: the call, kblk[block], this launch's |v|

// one bf16 / fp16 value of a bucket
template <int XT>
struct h16 {
    uint16_t v;
};

// ---------------------------------------------------------------------------
// a lane's chunk of 4 values at element e (values past n read as 0)
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
template <int XT>
__device__ __forceinline__ f32x4 ld4(const h16<XT>* p, size_t e, size_t n) {
    if (e + 4 <= n) return widen16x4<XT>(__builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p + e)));
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (e < n) v.x = widen16<XT>(p[e].v);
    if (e + 1 < n) v.y = widen16<XT>(p[e + 1].v);
    if (e + 2 < n) v.z = widen16<XT>(p[e + 2].v);
    return v;
}
__device__ __forceinline__ float ld1(const float* p, size_t j) { return p[j]; }
template <int XT>
__device__ __forceinline__ float ld1(const h16<XT>* p, size_t j) { return widen16<XT>(p[j].v); }

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
// 4 int16 (held widened in a u32x4) as one 8-byte store
__device__ __forceinline__ void st4h(u32x4 a, int16_t* p, size_t e, size_t n) {
    if (e + 4 <= n) {
        stream_store(u32x2{(a.x & 0xFFFFu) | (a.y << 16), (a.z & 0xFFFFu) | (a.w << 16)},
                     reinterpret_cast<u32x2*>(p + e));
    } else {
        if (e < n) p[e] = (int16_t)a.x;
        if (e + 1 < n) p[e + 1] = (int16_t)a.y;
        if (e + 2 < n) p[e + 2] = (int16_t)a.z;
    }
}

// ---------------------------------------------------------------------------
// the step (include/ina_ef.h): explicit roundings, no FMA
// ---------------------------------------------------------------------------
// v = (x - base) + r
__device__ __forceinline__ float ef_v(float x, float b, bool has_base, float r) {
    return __fadd_rn(has_base ? __fsub_rn(x, b) : x, r);
}
__device__ __forceinline__ f32x4 ef_v4(f32x4 x, f32x4 b, bool has_base, f32x4 r) {
    return f32x4{ef_v(x.x, b.x, has_base, r.x), ef_v(x.y, b.y, has_base, r.y), ef_v(x.z, b.z, has_base, r.z),
                 ef_v(x.w, b.w, has_base, r.w)};
}
// r' = v - float(q) * 2^-k, +0 for a NaN or infinite v
__device__ __forceinline__ float ef_r(float v, int32_t q, float inv) {
    const bool finite = (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u;
    return finite ? __fsub_rn(v, __fmul_rn((float)q, inv)) : 0.0f;
}
__device__ __forceinline__ f32x4 ef_r4(f32x4 v, u32x4 q, float inv) {
    return f32x4{ef_r(v.x, (int32_t)q.x, inv), ef_r(v.y, (int32_t)q.y, inv), ef_r(v.z, (int32_t)q.z, inv),
                 ef_r(v.w, (int32_t)q.w, inv)};
}
__device__ __forceinline__ u32x4 q32x4(f32x4 v, float s) {
    return u32x4{(uint32_t)q32(v.x, s), (uint32_t)q32(v.y, s), (uint32_t)q32(v.z, s), (uint32_t)q32(v.w, s)};
}
__device__ __forceinline__ u32x4 q16x4(f32x4 v, float s, bool& sat) {
    return u32x4{(uint32_t)q16(v.x, s, sat), (uint32_t)q16(v.y, s, sat), (uint32_t)q16(v.z, s, sat),
                 (uint32_t)q16(v.w, s, sat)};
}
// the lane's v at element e (0 for a lane past n)
template <typename X>
__device__ __forceinline__ f32x4 load_v(const X* x, const float* base, const float* resid, size_t e, size_t n) {
    if (e >= n) return f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 a = ld4(x, e, n), r = ld4(resid, e, n);
    const f32x4 b = base ? ld4<false>(base, e, n) : f32x4{0.f, 0.f, 0.f, 0.f};   // shared: default policy
    return ef_v4(a, b, base != nullptr, r);
}

// what a call's kernels share: buffers, and where k comes from
template <typename X, typename Q>
struct EfArgs {
    const X* x;
    const float* base;     // may be null
    float* resid;          // read, then written
    Q* q;
    size_t n;
    int k;                 // KG
    int8_t* kblk;          // KGIVEN: read; KAUTO: written
    double lim;            // KAUTO
    int shift;             // vector path, block modes: a block is 1 << shift lanes
    size_t V;              // int16 flags; scalar path: the block
    uint8_t* ovf;          // int16 out: may be null
};

// ---------------------------------------------------------------------------
// vector path, int32 out: chunk i = values 4i..4i+3, block of chunk i = i >> shift
// ---------------------------------------------------------------------------
template <typename X, int MODE>
__global__ __launch_bounds__(kBlk) void k_ef_i32(EfArgs<X, int32_t> a) {
    const size_t n = a.n, nq = (n + 3) / 4;
    const int lane = threadIdx.x & 63;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    for (size_t c0 = tid & ~(size_t)63; c0 < nq; c0 += stride) {          // wave-uniform
        const size_t i = c0 + lane, e = 4 * i;
        const f32x4 v = load_v(a.x, a.base, a.resid, e, n);
        int k = a.k;
        if constexpr (MODE == KAUTO) {
            const uint32_t m = group_max(fold4(0u, v), 1 << a.shift);
            k = scale_of(m, a.lim);
            if (e < n && (lane & ((1 << a.shift) - 1)) == 0) a.kblk[i >> a.shift] = (int8_t)k;
        } else if constexpr (MODE == KGIVEN) {
            if (e < n) k = rd_k(a.kblk, i >> a.shift);
        }
        if (e >= n) continue;
        const u32x4 q = q32x4(v, pow2f(k));
        st4(q, a.q, e, n);
        st4(ef_r4(v, q, pow2f(-k)), a.resid, e, n);
    }
}

// ---------------------------------------------------------------------------
// vector path, int16 out: a wave owns 512 values, lane l the 4 at 4l of each 256-value half
// ---------------------------------------------------------------------------
template <typename X, int MODE>
__global__ __launch_bounds__(kBlk) void k_ef_i16(EfArgs<X, int16_t> a) {
    const size_t n = a.n;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t nwaves = ((size_t)gridDim.x * kBlk) >> 6;
    const int lane = (int)(tid & 63);
    const size_t nreg = (n + 511) / 512;
    for (size_t r = tid >> 6; r < nreg; r += nwaves) {                    // wave-uniform
        const size_t eA = r * 512 + 4 * (size_t)lane, eB = eA + 256;
        const f32x4 u = load_v(a.x, a.base, a.resid, eA, n);
        const f32x4 v = load_v(a.x, a.base, a.resid, eB, n);
        int kA = a.k, kB = a.k;
        if constexpr (MODE == KAUTO) {
            const int lanes = 1 << a.shift;
            kA = scale_of(group_max(fold4(0u, u), lanes), a.lim);
            kB = scale_of(group_max(fold4(0u, v), lanes), a.lim);
            if ((lane & (lanes - 1)) == 0) {
                if (eA < n) a.kblk[eA >> (a.shift + 2)] = (int8_t)kA;
                if (eB < n) a.kblk[eB >> (a.shift + 2)] = (int8_t)kB;
            }
        } else if constexpr (MODE == KGIVEN) {
            if (eA < n) kA = rd_k(a.kblk, eA >> (a.shift + 2));
            if (eB < n) kB = rd_k(a.kblk, eB >> (a.shift + 2));
        }
        bool sa = false, sb = false;
        const u32x4 qa = q16x4(u, pow2f(kA), sa), qb = q16x4(v, pow2f(kB), sb);
        if (eA < n) {
            st4h(qa, a.q, eA, n);
            st4(ef_r4(u, qa, pow2f(-kA)), a.resid, eA, n);
        }
        if (eB < n) {
            st4h(qb, a.q, eB, n);
            st4(ef_r4(v, qb, pow2f(-kB)), a.resid, eB, n);
        }
        const unsigned long long ma = __ballot(sa), mb = __ballot(sb);   // wave-convergent
        if (a.ovf) write_slot_flags_split(ma, mb, eA, eB, n, (int)a.V, a.ovf);
    }
}

// ---------------------------------------------------------------------------
// scalar path: any V, any alignment.  One wave per block of a.V values (wave-uniform block loop),
// lanes striding over the block; Q = int32_t or int16_t.
// ---------------------------------------------------------------------------
template <typename X, typename Q, int MODE>
__global__ __launch_bounds__(kBlk) void k_ef_scalar(EfArgs<X, Q> a) {
    const size_t wave = ((size_t)blockIdx.x * kBlk + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * kBlk) >> 6;
    const int lane = threadIdx.x & 63;
    const size_t nblk = (a.n + a.V - 1) / a.V;
    auto value = [&](size_t j) {
        return ef_v(ld1(a.x, j), a.base ? a.base[j] : 0.f, a.base != nullptr, a.resid[j]);
    };
    for (size_t s = wave; s < nblk; s += nwaves) {                        // wave-uniform
        const size_t j0 = s * a.V, j1 = (j0 + a.V < a.n) ? j0 + a.V : a.n;
        int k = a.k;
        if constexpr (MODE == KAUTO) {
            uint32_t m = 0u;
            for (size_t j = j0 + lane; j < j1; j += 64) m = umax(m, absbits(value(j)));
            k = scale_of(group_max(m, 64), a.lim);
            if (lane == 0) a.kblk[s] = (int8_t)k;
        } else if constexpr (MODE == KGIVEN) {
            k = rd_k(a.kblk, s);
        }
        const float sc = pow2f(k), inv = pow2f(-k);
        [[maybe_unused]] bool sat = false;
        for (size_t j = j0 + lane; j < j1; j += 64) {
            const float v = value(j);
            int32_t q;
            if constexpr (sizeof(Q) == 4) q = q32(v, sc);
            else q = q16(v, sc, sat);
            a.q[j] = (Q)q;
            a.resid[j] = ef_r(v, q, inv);
        }
        if constexpr (sizeof(Q) == 2) {
            const unsigned long long m = __ballot(sat);                   // wave-convergent
            if (a.ovf && lane == 0) a.ovf[s] = m ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------
// scales alone, over |(xs[w] - base) + resids[w]|: 2W + 1 streams, nothing written but kblk
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlk) void k_ef_scales(PtrPack<float> xs, PtrPack<float> rs, int W,
                                                    const float* __restrict__ base, size_t n, int shift, double lim,
                                                    int8_t* __restrict__ kblk) {
    const size_t nq = (n + 3) / 4;
    const int lane = threadIdx.x & 63;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    for (size_t c0 = tid & ~(size_t)63; c0 < nq; c0 += stride) {          // wave-uniform
        const size_t i = c0 + lane, e = 4 * i;
        uint32_t m = 0u;
        for (int w = 0; w < W; ++w) m = fold4(m, load_v(xs.p[w], base, rs.p[w], e, n));
        m = group_max(m, 1 << shift);
        if (e < n && (lane & ((1 << shift) - 1)) == 0) kblk[i >> shift] = (int8_t)scale_of(m, lim);
    }
}
__global__ __launch_bounds__(kBlk) void k_ef_scales_scalar(PtrPack<float> xs, PtrPack<float> rs, int W,
                                                           const float* __restrict__ base, size_t n, size_t V,
                                                           double lim, int8_t* __restrict__ kblk) {
    const size_t wave = ((size_t)blockIdx.x * kBlk + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * kBlk) >> 6;
    const int lane = threadIdx.x & 63;
    const size_t nblk = (n + V - 1) / V;
    for (size_t s = wave; s < nblk; s += nwaves) {                        // wave-uniform
        const size_t j0 = s * V, j1 = (j0 + V < n) ? j0 + V : n;
        uint32_t m = 0u;
        for (size_t j = j0 + lane; j < j1; j += 64)
            for (int w = 0; w < W; ++w)
                m = umax(m, absbits(ef_v(xs.p[w][j], base ? base[j] : 0.f, base != nullptr, rs.p[w][j])));
        m = group_max(m, 64);
        if (lane == 0) kblk[s] = (int8_t)scale_of(m, lim);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int launched() { return check_launch("error-feedback kernel launch"); }

using bf16_t = h16<INA_X16_BF16>;
using fp16_t = h16<INA_X16_F16>;

// the vector path reads a lane's 4 values of x in one load and its r, base and q chunks likewise
template <typename X, typename Q>
bool vec_ok(const EfArgs<X, Q>& a) {
    return (uintptr_t)a.x % (4 * sizeof(X)) == 0 && aligned16(a.resid) && (!a.base || aligned16(a.base)) &&
           (uintptr_t)a.q % (4 * sizeof(Q)) == 0;
}

// one call: the vector kernel where `vec` (the layout fits V and the buffers), else a wave per
// block of V values
template <int MODE, typename X, typename Q>
int launch_ef(EfArgs<X, Q> a, bool vec, ina_stream_t stream) {
    hipStream_t s = hs(stream);
    const dim3 b(kBlk);
    if (vec && vec_ok(a)) {
        if constexpr (sizeof(Q) == 4) {
            hipLaunchKernelGGL((k_ef_i32<X, MODE>), dim3(grid_of((a.n + 3) / 4, default_grid_cap())), b, 0, s, a);
        } else {
            hipLaunchKernelGGL((k_ef_i16<X, MODE>), dim3(grid_of((a.n + 511) / 512 * 64, default_grid_cap())), b, 0, s,
                               a);
        }
    } else {
        const size_t nblk = (a.n + a.V - 1) / a.V;
        hipLaunchKernelGGL((k_ef_scalar<X, Q, MODE>), dim3(grid_of(nblk * 64, default_grid_cap())), b, 0, s, a);
    }
    return launched();
}

// the global-k calls; X: float or h16<XT>.  V = 0: int32 out (no slots)
template <typename X, typename Q>
int quantize_ef(const void* x, const float* base, float* resid, Q* q, size_t n, int k, int V, uint8_t* ovf,
                ina_stream_t stream) {
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!resid) return set_error(INA_EINVAL, "null resid%s", "");
    if (sizeof(X) == 2 && ((uintptr_t)x & 1u)) return set_error(INA_EINVAL, "16-bit buffers must be 2-byte aligned%s", "");
    EfArgs<X, Q> a{static_cast<const X*>(x), base, resid, q, n, k, nullptr, 1.0, 0, (size_t)(V ? V : 256), ovf};
    return launch_ef<KG>(a, sizeof(Q) == 4 || !ovf || slot_ballot_ok(V), stream);
}

template <typename Q>
int quantize_ef_blk(const float* x, const float* base, float* resid, int8_t* kblk, int mode, int degree, int V, Q* q,
                    size_t n, uint8_t* ovf, ina_stream_t stream) {
    double lim;
    if (int rc = check_v(V)) return rc;
    if (int rc = check_mode(mode, kblk, degree, 8 * (int)sizeof(Q), lim)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!resid) return set_error(INA_EINVAL, "null resid%s", "");
    int shift = 0;
    const bool vec = vec_v(V, shift);
    EfArgs<float, Q> a{x, base, resid, q, n, 0, kblk, lim, shift, (size_t)V, ovf};
    if (mode == INA_BLK_AUTO) return launch_ef<KAUTO>(a, vec, stream);
    return launch_ef<KGIVEN>(a, vec, stream);
}

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

int ina_quantize_ef_f32_i32(const float* x, const float* base, float* resid, int32_t* q, size_t n, int k,
                            ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    return quantize_ef<float>(x, base, resid, q, n, k, 0, nullptr, stream);
}

int ina_quantize_ef_f32_i16_sat(const float* x, const float* base, float* resid, int16_t* q, size_t n, int k, int V,
                                uint8_t* ovf, ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    return quantize_ef<float>(x, base, resid, q, n, k, V, ovf, stream);
}

int ina_quantize_ef_x16_i32(const void* x, int xtype, const float* base, float* resid, int32_t* q, size_t n, int k,
                            ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (xtype == INA_X16_BF16) return quantize_ef<bf16_t>(x, base, resid, q, n, k, 0, nullptr, stream);
    return quantize_ef<fp16_t>(x, base, resid, q, n, k, 0, nullptr, stream);
}

int ina_quantize_ef_x16_i16_sat(const void* x, int xtype, const float* base, float* resid, int16_t* q, size_t n,
                                int k, int V, uint8_t* ovf, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    if (xtype == INA_X16_BF16) return quantize_ef<bf16_t>(x, base, resid, q, n, k, V, ovf, stream);
    return quantize_ef<fp16_t>(x, base, resid, q, n, k, V, ovf, stream);
}

int ina_block_scales_ef_f32(const float* const* xs, const float* const* resids, int W, const float* base, size_t n,
                            int V, int degree, int bits, int8_t* kblk, ina_stream_t stream) {
    double lim;
    if (int rc = check_v(V)) return rc;
    if (int rc = scale_lim(degree, bits, lim)) return rc;
    if (n == 0) return INA_OK;
    PtrPack<float> px, pr;
    bool alx, alr;
    if (int rc = fill_pack(px, xs, W, alx)) return rc;
    if (!resids) return set_error(INA_EINVAL, "null resid%s", "");
    if (int rc = fill_pack(pr, resids, W, alr)) return rc;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    hipStream_t s = hs(stream);
    int shift;
    if (vec_v(V, shift) && alx && alr && (!base || aligned16(base))) {
        hipLaunchKernelGGL(k_ef_scales, dim3(grid_of((n + 3) / 4, default_grid_cap())), dim3(kBlk), 0, s, px, pr, W,
                           base, n, shift, lim, kblk);
    } else {
        const size_t nblk = (n + (size_t)V - 1) / (size_t)V;
        hipLaunchKernelGGL(k_ef_scales_scalar, dim3(grid_of(nblk * 64, default_grid_cap())), dim3(kBlk), 0, s, px, pr,
                           W, base, n, (size_t)V, lim, kblk);
    }
    return launched();
}

int ina_quantize_ef_blk_f32_i32(const float* x, const float* base, float* resid, int8_t* kblk, int mode, int degree,
                                int V, int32_t* q, size_t n, ina_stream_t stream) {
    return quantize_ef_blk(x, base, resid, kblk, mode, degree, V, q, n, nullptr, stream);
}

int ina_quantize_ef_blk_f32_i16_sat(const float* x, const float* base, float* resid, int8_t* kblk, int mode,
                                    int degree, int V, int16_t* q, size_t n, uint8_t* ovf, ina_stream_t stream) {
    return quantize_ef_blk(x, base, resid, kblk, mode, degree, V, q, n, ovf, stream);
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_ef() { return take_store_violations(); }
#endif
