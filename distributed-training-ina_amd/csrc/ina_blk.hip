// ina_blk.hip -- per-block scales (block floating point) for the quantiser, the fused reduces
// and the PS update (include/ina_blk.h states the contract).
//
// One int8 exponent per block of V values.  Every kernel here runs the quantiser of the global-k
// entry points (q32 / q16 / sat16, ina_device.h) with the block's own 2^k, so a block's result is
// bit for bit the sibling's on that block alone.
//
// Lane layout (vector path: V a power of two in [8, 256], 16-byte aligned buffers, 256-thread
// workgroups, non-temporal loads, write-through stores, like the siblings).  A lane always holds
// 16-byte chunks of 4 fp32 / int32 values, so a block is V/4 adjacent lanes of one wave:
//   32-bit side (quantise / reduce to int32, both dequantises, PS apply, PS combine, scales):
//     lane l of a wave owns values 4l..4l+3 of the wave's 256 -- the siblings' layout.
//   int16 out (quantise / reduce to int16): a wave owns 512 values as two 256-value halves, lane l
//     the 4 at 4l of each half (16 B per lane per load, 1 KiB contiguous per instruction: the
//     layout k_quant_reduce_i16 measured 13 % faster than 8 consecutive values per lane), one
//     8-byte store per half.  Each half has its own group and its own scale.
// kblk[s] is one byte load per lane of the group (the same address across the group), and the slot
// flag comes from the one-writer ballot (write_slot_flags8) with V/4 lanes per slot.
//
// AUTO (scales computed in the pass): the block's max |value| is a cross-lane unsigned max of the
// fp32 bit patterns over the group (non-negative floats order as their bits; NaN mapped to 0
// first), butterfly over lane ^ 1, 2, ... < V/4.  It runs wave-convergent: every loop has a
// wave-uniform trip count, lanes past n contribute 0 and take part.  Compile-time W (1, 2, 4, 8,
// 16) keeps the lane's W chunks in registers between the max and the quantiser (one read of the
// inputs); any other W reads them a second time in the same launch (the lane's own chunks, so the
// second read is the one the first brought in).  A lane reads all of its chunks before it writes
// any, so out may alias an input of the same width.
//
// Scalar path (any other V or alignment): one wave per block, lanes striding over the block,
// the same helpers, identical results.
//
// bf16 / fp16 buckets (include/ina_x16_blk.h): every kernel that reads or writes a bucket takes its
// element type X, float or h16<XT>.  Only the chunk's load (ld4: one 8-byte load, widened in
// registers, exact) and the decode's store (st4: rounded once to nearest even, one 8-byte store)
// differ; a lane still owns 4 values, a block is still V/4 lanes, and everything after the load is
// the fp32 kernel's code on the widened chunk, so held chunks cost the fp32 kernel's registers.
// The vector path needs the 16-bit side 8-byte aligned.
//
// Error feedback (include/ina_ef.h; entry points in ina_ef.hip): the same kernels at W = 1 with the
// SrcEf value source, which reads v = (x - base) + r where the plain source reads x and stores r'
// once v is quantised, and a third scale mode, the call's one k.  No kernel of its own.  The EF
// quantisers of the sharded int16 wire (include/ina_shard_ef.h) are the int32 instances with the
// SrcEfWire source: the wire word q16 + (sat << 22) where those run q32, q16 into the carry.
//
// Stochastic rounding (include/ina_blk_sr.h): the same kernels with the SrcSr value source, which reads
// what the plain source reads and carries the call's Philox key.  Where the source says kSr, a chunk is
// rounded by sr_y4 (ina_sr_device.h) with the words of one Philox call at the chunk's counter, worker w
// on stream sub + w, in place of rintf; the clamps, the sums, the scales, the flags and every load and
// store are the round-to-nearest instances'.  No kernel of its own; the sharded int16 wire's stochastic
// block quantiser is the int32 instance at W = 1 with the wire word, as the error-feedback one is.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"
#include "ina_sr_device.h"

namespace ina {

// ina_scale_for's rule for the number of summands
int scale_lim(int degree, int bits, double& lim, double round) {
    if (bits != 16 && bits != 32) return set_error(INA_EINVAL, "bits must be 16 or 32%s", "");
    if (degree < 1) return set_error(INA_EINVAL, "degree must be >= 1%s", "");
    lim = (bits == 32 ? 2147483647.0 : 32767.0) / (double)degree - round;
    if (lim <= 0.0) return set_error(INA_EINVAL, "too many summands (degree) for this width%s", "");
    return INA_OK;
}

namespace {

constexpr int kBlk = 256;

// (rd_k, pow2f, absbits, umax, fold4, scale_of and group_max are in ina_device.h, a lane's chunk of
// 4 values -- ld4, st4, q32x4, ... -- in ina_chunk.h: the block-scaled packet kernels of
// ina_kernels.hip run the same ones)

// ---------------------------------------------------------------------------
// Value sources: what the quantising kernels read as worker w's chunk (four) or value (one) at an
// element.  X: the element type of a call's buckets -- float, or h16<XT>.
// ---------------------------------------------------------------------------
template <typename X>
struct SrcPlain {
    static constexpr bool kEf = false;
    static constexpr bool kWire = false;
    static constexpr bool kSr = false;
    using Elem = X;
    PtrPack<X> in;
    __device__ __forceinline__ f32x4 four(int w, size_t e, size_t n) const { return ld4(in.p[w], e, n); }
    __device__ __forceinline__ float one(int w, size_t j) const { return ld1(in.p[w], j); }
    __device__ __forceinline__ void carry(int, f32x4, u32x4, float, size_t, size_t) const {}
    __device__ __forceinline__ void carry1(int, float, int32_t, float, size_t) const {}
};
// Error feedback (include/ina_ef.h): the value is v = (x - base) + r, and once it is quantised to q
// the kernel hands it back (carry) for r' = v - float(q) * 2^-k to go where r was.  A lane reads its
// r before it writes r' and no other lane touches those 16 bytes, so the update is in place.  x and
// r are read once (non-temporal), the base is shared between a step's calls (default policy, as in
// the packs).  N pointer pairs: 1 for the quantisers, INA_MAX_WORKERS for the scales.
template <typename X, int N>
struct SrcEf {
    static constexpr bool kEf = true;
    static constexpr bool kWire = false;
    static constexpr bool kSr = false;
    using Elem = X;
    const X* x[N];
    float* resid[N];
    const float* base;     // may be null
    __device__ __forceinline__ f32x4 four(int w, size_t e, size_t n) const {
        if (e >= n) return f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 a = ld4(x[w], e, n), r = ld4(resid[w], e, n);
        return ef_v4(base ? sub4(a, ld4<false>(base, e, n)) : a, r);
    }
    __device__ __forceinline__ float one(int w, size_t j) const {
        const float a = ld1(x[w], j);
        return ef_v(base ? __fsub_rn(a, base[j]) : a, resid[w][j]);
    }
    __device__ __forceinline__ void carry(int w, f32x4 v, u32x4 q, float inv, size_t e, size_t n) const {
        st4(ef_r4(v, q, inv), resid[w], e, n);
    }
    __device__ __forceinline__ void carry1(int w, float v, int32_t q, float inv, size_t j) const {
        resid[w][j] = ef_r(v, q, inv);
    }
};
// Error feedback on the sharded int16 wire (include/ina_shard_ef.h): the same source, and the int32
// kernels quantise what it reads to the wire word q16 + (sat << 22) (q16w) where they run q32.  The
// carry is handed the word's q16, never the word with its count bits.
struct SrcEfWire : SrcEf<float, 1> {
    static constexpr bool kWire = true;
};
// Stochastic rounding (include/ina_blk_sr.h): the plain source's values, and the random words that round
// them -- Philox4x32-10 under the call's key at the counter of the chunk at element e (i0 + e / 4),
// worker w on stream sub + w.  The block's scale has no part in them.  WIRE: the int32 kernels write
// the sharded int16 wire's word.
template <typename X, bool WIRE = false>
struct SrcSr : SrcPlain<X> {
    static constexpr bool kWire = WIRE;
    static constexpr bool kSr = true;
    SrKey key;
    __device__ __forceinline__ u32x4 words(int w, size_t e) const { return philox(stream_of(key, w), key.i0 + (e >> 2)); }
    __device__ __forceinline__ uint32_t word(int w, size_t j) const { return word_of(stream_of(key, w), j); }
};

// ---------------------------------------------------------------------------
// vector path, 32-bit side: chunk i = values 4i..4i+3, block of chunk i = i >> shift
// (shift = log2(V) - 2, a group is 1 << shift lanes).  Every loop below has a wave-uniform trip
// count.
// ---------------------------------------------------------------------------
#define INA_BLK_QUAD_LOOP(nq)                                                      \
    const size_t tid_ = (size_t)blockIdx.x * kBlk + threadIdx.x;                   \
    const size_t stride_ = (size_t)gridDim.x * kBlk;                               \
    for (size_t base_ = tid_ & ~(size_t)63; base_ < (nq); base_ += stride_)

// scales alone: W + 1 streams, 4 workers' loads in flight (k_absmax_multi_f32's loop).  (An EF source
// brings its own base and residuals, 2W + 1 streams; `base` is then null.)
template <typename Src>
__global__ __launch_bounds__(kBlk) void k_blk_scales(Src xs, int W, const float* __restrict__ base,
                                                     size_t n, int shift, double lim,
                                                     int8_t* __restrict__ kblk) {
    const size_t nq = (n + 3) / 4;
    const int lane = threadIdx.x & 63;
    INA_BLK_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        uint32_t m = 0u;
        if (e < n) {
            const f32x4 b = base ? ld4(base, e, n) : f32x4{0.f, 0.f, 0.f, 0.f};
            int w = 0;
            for (; w + 4 <= W; w += 4) {
                f32x4 a[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = xs.four(w + u, e, n);
#pragma unroll
                for (int u = 0; u < 4; ++u) m = fold4(m, sub4(a[u], b));
            }
            for (; w < W; ++w) m = fold4(m, sub4(xs.four(w, e, n), b));
        }
        m = group_max(m, 1 << shift);
        if (e < n && (lane & ((1 << shift) - 1)) == 0) kblk[i >> shift] = (int8_t)scale_of(m, lim);
    }
}

// fused quantise + W-way reduce to int32 (W = 1: the plain quantiser).  W > 0: compile-time worker
// count, chunks held in registers; W = 0: runtime count, re-read under AUTO.  KM, where a block's k
// comes from: K_GLOBAL (the call's kg for every block; the EF calls only), K_GIVEN (kblk read),
// K_AUTO (the block's max |value|, kblk written).
template <typename Src, int W, int KM>
__global__ __launch_bounds__(kBlk) void k_qr_blk_i32(Src in, int Wd, int kg, int8_t* __restrict__ kblk,
                                                     double lim, int32_t* out, size_t n, int shift) {
    constexpr bool AUTO = KM == K_AUTO;
    static_assert(!Src::kEf || W == 1, "one residual: one bucket");
    const int nw = W > 0 ? W : Wd;
    // given scales: a chunk is quantised as it arrives (an EF source: held, so that its three loads
    // are in flight beside the scale's and not behind it)
    constexpr bool HOLD = (AUTO && W > 0) || Src::kEf;
    constexpr int UNR = W > 0 ? W : 1;
    const size_t nq = (n + 3) / 4;
    const int lane = threadIdx.x & 63;
    INA_BLK_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        if constexpr (Src::kEf && !AUTO) {
            if (e >= n) continue;                  // no cross-lane step below: the loads wait once
        }
        [[maybe_unused]] f32x4 v[HOLD ? W : 1];
        if constexpr (HOLD) {
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = in.four(w, e, n);
        }
        int k = KM == K_GLOBAL ? kg : 0;
        if constexpr (AUTO) {
            uint32_t m = 0u;
            if constexpr (HOLD) {
#pragma unroll
                for (int w = 0; w < W; ++w) m = fold4(m, v[w]);
            } else {
                for (int w = 0; w < nw; ++w) m = fold4(m, in.four(w, e, n));
            }
            m = group_max(m, 1 << shift);
            k = scale_of(m, lim);
            if (e < n && (lane & ((1 << shift) - 1)) == 0) kblk[i >> shift] = (int8_t)k;
        } else if constexpr (KM == K_GIVEN) {
            if (e < n) k = rd_k(kblk, i >> shift);
        }
        const float s = pow2f(k);
        [[maybe_unused]] const float inv = pow2f(-k);         // the EF carry's
        u32x4 acc = {0u, 0u, 0u, 0u};
        // worker w's chunk: quantised, summed, and handed back to the source
        auto add = [&](int w, f32x4 x) {
            if constexpr (Src::kSr) {
                const u32x4 r = in.words(w, e);
                if constexpr (Src::kWire) acc += sr_q16wx4(x, s, r);
                else acc += sr_q32x4(x, s, r);
            } else if constexpr (Src::kWire) {
                const u32x4 word = q16wx4(x, s);
                acc += word;
                in.carry(w, x, wire_q16x4(word), inv, e, n);
            } else {
                const u32x4 q = q32x4(x, s);
                acc += q;
                in.carry(w, x, q, inv, e, n);
            }
        };
        if constexpr (HOLD) {
#pragma unroll
            for (int w = 0; w < W; ++w) add(w, v[w]);
        } else {
#pragma unroll UNR
            for (int w = 0; w < nw; ++w) add(w, in.four(w, e, n));
        }
        if (e < n) st4(acc, out, e, n);
    }
}

template <typename T, typename Y>
__global__ __launch_bounds__(kBlk) void k_dq_blk(const T* __restrict__ sv, const int8_t* __restrict__ kblk,
                                                 Y* __restrict__ y, size_t n, int shift) {
    const size_t nq = (n + 3) / 4;
    const int lane = threadIdx.x & 63;
    INA_BLK_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        if (e >= n) continue;
        u32x4 q;
        if constexpr (sizeof(T) == 4) q = ld4i(sv, e, n);
        else q = ld4h(sv, e, n);
        st4(deq4(q, pow2f(-rd_k(kblk, i >> shift))), y, e, n);
    }
}

__global__ __launch_bounds__(kBlk) void k_ps_apply_blk(const float* local, const int32_t* __restrict__ sum,
                                                       const int8_t* __restrict__ kblk, float ws, float* out,
                                                       size_t n, int shift) {
    const size_t nq = (n + 3) / 4;
    const int lane = threadIdx.x & 63;
    INA_BLK_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        if (e >= n) continue;
        const f32x4 l = ld4<false>(local, e, n);
        const u32x4 q = ld4i(sum, e, n);
        st4(upd4(l, deq4(q, pow2f(-rd_k(kblk, i >> shift))), ws), out, e, n);
    }
}

// INA update in one pass, scales on the fly from the W deltas (degree = W, bits = 32)
template <int W>
__global__ __launch_bounds__(kBlk) void k_ps_combine_ina_blk(const float* local, PtrPack<float> paras, int Wd,
                                                             double lim, float ws, float* out, size_t n,
                                                             int shift, int8_t* __restrict__ kblk) {
    const int nw = W > 0 ? W : Wd;
    const size_t nq = (n + 3) / 4;
    const int lane = threadIdx.x & 63;
    INA_BLK_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        const f32x4 l = ld4<false>(local, e, n);
        [[maybe_unused]] f32x4 d[W > 0 ? W : 1];
        uint32_t m = 0u;
        if constexpr (W > 0) {
#pragma unroll
            for (int w = 0; w < W; ++w) d[w] = ld4(paras.p[w], e, n);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                d[w] = sub4(d[w], l);
                m = fold4(m, d[w]);
            }
        } else {
            for (int w = 0; w < nw; ++w) m = fold4(m, sub4(ld4(paras.p[w], e, n), l));
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
            for (int w = 0; w < nw; ++w) acc += q32x4(sub4(ld4(paras.p[w], e, n), l), s);
        }
        if (e < n) st4(upd4(l, deq4(acc, pow2f(-k)), ws), out, e, n);
    }
}

// ---------------------------------------------------------------------------
// vector path, int16 out: a wave owns 512 values, lane l the 4 at 4l of each 256-value half
// ---------------------------------------------------------------------------
// the int16 out: it may alias a 16-bit bucket (the same width), never an fp32 one
template <typename X>
struct Out16 {
    using P = int16_t*;
};
template <>
struct Out16<float> {
    using P = int16_t* __restrict__;
};
// (an EF source holds its chunks under every KM, as above: and both halves' loads are issued before
// the first r' store, which they may not pass.  K_GLOBAL: V is any size with a ballot layout, up to a slot of both
// halves at 512, and shift is unused)
template <typename Src, int W, int KM>
__global__ __launch_bounds__(kBlk) void k_qr_blk_i16(Src in, int Wd, int kg, int8_t* __restrict__ kblk, double lim,
                                                     typename Out16<typename Src::Elem>::P out, size_t n, int shift,
                                                     int V, uint8_t* __restrict__ ovf) {
    constexpr bool AUTO = KM == K_AUTO;
    static_assert(!Src::kEf || W == 1, "one residual: one bucket");
    const int nw = W > 0 ? W : Wd;
    constexpr bool HOLD = (AUTO && W > 0) || Src::kEf;
    constexpr int UNR = W > 0 ? W : 1;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t nwaves = ((size_t)gridDim.x * kBlk) >> 6;
    const int lane = (int)(tid & 63), lanes = 1 << shift;
    const size_t nreg = (n + 511) / 512;
    for (size_t r = tid >> 6; r < nreg; r += nwaves) {          // wave-uniform
        const size_t eA = r * 512 + 4 * (size_t)lane, eB = eA + 256;
        [[maybe_unused]] f32x4 u[HOLD ? W : 1], v[HOLD ? W : 1];
        if constexpr (HOLD) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                u[w] = in.four(w, eA, n);
                v[w] = in.four(w, eB, n);
            }
        }
        int kA = KM == K_GLOBAL ? kg : 0, kB = kA;
        if constexpr (AUTO) {
            uint32_t mA = 0u, mB = 0u;
            if constexpr (HOLD) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    mA = fold4(mA, u[w]);
                    mB = fold4(mB, v[w]);
                }
            } else {
                for (int w = 0; w < nw; ++w) {
                    mA = fold4(mA, in.four(w, eA, n));
                    mB = fold4(mB, in.four(w, eB, n));
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
        } else if constexpr (KM == K_GIVEN) {
            if (eA < n) kA = rd_k(kblk, eA >> (shift + 2));
            if (eB < n) kB = rd_k(kblk, eB >> (shift + 2));
        }
        const float sA = pow2f(kA), sB = pow2f(kB);
        [[maybe_unused]] const float invA = pow2f(-kA), invB = pow2f(-kB);   // the EF carry's
        bool sa = false, sb = false;
        int32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
        // worker w's chunk at element e: quantised and added to the half's sums
        auto add = [&](int w, f32x4 x, size_t e, float s, int32_t* acc, bool& sat) {
            if constexpr (Src::kSr) q16x4_add_sr(x, s, in.words(w, e), acc, sat);
            else q16x4_add(x, s, acc, sat);
        };
        if constexpr (HOLD) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                add(w, u[w], eA, sA, a, sa);
                add(w, v[w], eB, sB, b, sb);
            }
        } else {
#pragma unroll UNR
            for (int w = 0; w < nw; ++w) {
                add(w, in.four(w, eA, n), eA, sA, a, sa);
                add(w, in.four(w, eB, n), eB, sB, b, sb);
            }
        }
        if constexpr (!Src::kEf) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = sat16(a[j], sa);
                b[j] = sat16(b[j], sb);
            }
        }
        // (an EF source, W = 1: the sums are the bucket's own q, in range as they are; clamping them
        // again cost the EF instances 8 VGPRs and a wave per SIMD)
        if (eA < n) st4h(a, out, eA, n);
        if constexpr (Src::kEf)
            in.carry(0, u[0], u32x4{(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]}, invA, eA, n);
        if (eB < n) st4h(b, out, eB, n);
        if constexpr (Src::kEf)
            in.carry(0, v[0], u32x4{(uint32_t)b[0], (uint32_t)b[1], (uint32_t)b[2], (uint32_t)b[3]}, invB, eB, n);
        const unsigned long long ma = __ballot(sa), mb = __ballot(sb);   // wave-convergent
        if (ovf) {
            if constexpr (KM == K_GLOBAL) {
                write_slot_flags_split(ma, mb, eA, eB, n, V, ovf);
            } else {
                write_slot_flags8(ma, eA < n, eA, V, lanes, ovf);
                write_slot_flags8(mb, eB < n, eB, V, lanes, ovf);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// scalar path: any V, any alignment.  One wave per block (wave-uniform block loop), lanes
// striding over the block's values; one kernel for every entry point.
// ---------------------------------------------------------------------------
enum { S_SCALES, S_Q32, S_Q16, S_DQ32, S_DQ16, S_APPLY, S_COMB };
template <typename Src>
struct ScalarArgs {
    Src in;                // worker buffers (S_SCALES, S_Q32, S_Q16, S_COMB)
    int W;
    int kg;                // K_GLOBAL: the call's k
    const float* base;     // S_SCALES: base or null; S_APPLY, S_COMB: local
    const void* src;       // S_DQ32, S_DQ16, S_APPLY: the integers
    int8_t* kblk;          // read (GIVEN) or written (AUTO; may be null for S_COMB)
    double lim;
    void* out;             // S_DQ32, S_DQ16: X values; otherwise the mode's own type
    size_t n;
    size_t V;
    uint8_t* ovf;
    float ws;
};

template <typename Src, int MODE, int KM>
__global__ __launch_bounds__(kBlk) void k_blk_scalar(ScalarArgs<Src> a) {
    using X = typename Src::Elem;
    const size_t wave = ((size_t)blockIdx.x * kBlk + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * kBlk) >> 6;
    const int lane = threadIdx.x & 63;
    const size_t nblk = (a.n + a.V - 1) / a.V;
    constexpr bool kDelta = MODE == S_SCALES || MODE == S_COMB;     // values are in[w][j] - base[j]
    for (size_t s = wave; s < nblk; s += nwaves) {                  // wave-uniform
        const size_t j0 = s * a.V, j1 = (j0 + a.V < a.n) ? j0 + a.V : a.n;
        int k = a.kg;
        if constexpr (KM == K_AUTO) {
            uint32_t m = 0u;
            for (size_t j = j0 + lane; j < j1; j += 64)
                for (int w = 0; w < a.W; ++w) {
                    const float x = a.in.one(w, j);
                    m = umax(m, absbits((kDelta && a.base) ? __fsub_rn(x, a.base[j]) : x));
                }
            m = group_max(m, 64);
            k = scale_of(m, a.lim);
            if (lane == 0 && a.kblk) a.kblk[s] = (int8_t)k;
        } else if constexpr (KM == K_GIVEN) {
            k = rd_k(a.kblk, s);
        }
        if constexpr (MODE == S_SCALES) continue;
        [[maybe_unused]] const float sc = pow2f(k), inv = pow2f(-k);
        [[maybe_unused]] bool sat = false;
        for (size_t j = j0 + lane; j < j1; j += 64) {
            if constexpr (MODE == S_Q32) {
                uint32_t acc = 0u;
                for (int w = 0; w < a.W; ++w) {
                    const float x = a.in.one(w, j);
                    if constexpr (Src::kSr) {
                        const float y = sr_y(x, sc, a.in.word(w, j));
                        acc += (uint32_t)(Src::kWire ? q16w_of(y) : q32_of(y));
                    } else if constexpr (Src::kWire) {
                        const int32_t word = q16w(x, sc);
                        acc += (uint32_t)word;
                        a.in.carry1(w, x, wire_q16(word), inv, j);
                    } else {
                        const int32_t q = q32(x, sc);
                        acc += (uint32_t)q;
                        a.in.carry1(w, x, q, inv, j);
                    }
                }
                static_cast<int32_t*>(a.out)[j] = (int32_t)acc;
            } else if constexpr (MODE == S_Q16) {
                int32_t acc = 0;
                for (int w = 0; w < a.W; ++w) {
                    const float x = a.in.one(w, j);
                    int32_t q;
                    if constexpr (Src::kSr) q = q16_of(sr_y(x, sc, a.in.word(w, j)), sat);
                    else q = q16(x, sc, sat);
                    acc += q;
                    a.in.carry1(w, x, q, inv, j);
                }
                static_cast<int16_t*>(a.out)[j] = (int16_t)sat16(acc, sat);
            } else if constexpr (MODE == S_DQ32) {
                st1(__fmul_rn((float)static_cast<const int32_t*>(a.src)[j], inv), static_cast<X*>(a.out), j);
            } else if constexpr (MODE == S_DQ16) {
                st1(__fmul_rn((float)static_cast<const int16_t*>(a.src)[j], inv), static_cast<X*>(a.out), j);
            } else if constexpr (MODE == S_APPLY) {
                const float y = __fmul_rn((float)static_cast<const int32_t*>(a.src)[j], inv);
                static_cast<float*>(a.out)[j] = __fadd_rn(a.base[j], __fmul_rn(y, a.ws));
            } else {
                const float l = a.base[j];
                uint32_t acc = 0u;
                for (int w = 0; w < a.W; ++w) acc += (uint32_t)q32(__fsub_rn(a.in.one(w, j), l), sc);
                const float y = __fmul_rn((float)(int32_t)acc, inv);
                static_cast<float*>(a.out)[j] = __fadd_rn(l, __fmul_rn(y, a.ws));
            }
        }
        if constexpr (MODE == S_Q16) {
            const unsigned long long m = __ballot(sat);               // wave-convergent
            if (a.ovf && lane == 0) a.ovf[s] = m ? 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// (vec_v, the vector path's block sizes, is in ina_internal.h; check_v and check_mode are declared
// there for ina_ef.hip)
}  // namespace
int check_v(int V) { return V < 1 ? set_error(INA_EINVAL, "V must be >= 1%s", "") : INA_OK; }
int check_mode(int mode, const int8_t* kblk, int degree, int bits, double& lim, double round) {
    lim = 1.0;
    if (mode != INA_BLK_GIVEN && mode != INA_BLK_AUTO)
        return set_error(INA_EINVAL, "mode must be INA_BLK_GIVEN (0) or INA_BLK_AUTO (1)%s", "");
    if (mode == INA_BLK_AUTO) {
        if (int rc = scale_lim(degree, bits, lim, round)) return rc;
    }
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    return INA_OK;
}
namespace {
int launched() { return check_launch("block-scale kernel launch"); }

template <int MODE, int KM, typename Src>
void launch_scalar(const ScalarArgs<Src>& a, hipStream_t s) {
    const size_t nblk = (a.n + a.V - 1) / a.V;
    hipLaunchKernelGGL((k_blk_scalar<Src, MODE, KM>), dim3(grid_of(nblk * 64, default_grid_cap())), dim3(kBlk), 0, s, a);
}

// compile-time worker counts of the fused kernels (others: the runtime-W instance)
#define INA_BLK_W_SWITCH(W, LAUNCH) \
    switch (W) {                    \
        case 1: LAUNCH(1); break;   \
        case 2: LAUNCH(2); break;   \
        case 4: LAUNCH(4); break;   \
        case 8: LAUNCH(8); break;   \
        case 16: LAUNCH(16); break; \
        default: LAUNCH(0);         \
    }

// the vector path reads a lane's 4 values in one load: 16 bytes of an fp32 bucket, 8 of a 16-bit one
template <typename X>
bool src_aligned(const PtrPack<X>& pk, int W) {
    for (int w = 0; w < W; ++w)
        if ((uintptr_t)pk.p[w] % (4 * sizeof(X))) return false;
    return true;
}
using bf16_t = h16<INA_X16_BF16>;
using fp16_t = h16<INA_X16_F16>;
// F<h16<xtype>>(args) for a checked xtype
#define INA_BLK_X16_CALL(xtype, F, ...) \
    ((xtype) == INA_X16_BF16 ? F<bf16_t>(__VA_ARGS__) : F<fp16_t>(__VA_ARGS__))

// X: float (B = float) or h16<XT> (B = void, include/ina_x16_blk.h); round: scale_lim's
template <typename X, typename B>
int block_scales(const B* const* xs, int W, const float* base, size_t n, int V, int degree, int bits, int8_t* kblk,
                 ina_stream_t stream, double round = 0.5) {
    double lim;
    if (int rc = check_v(V)) return rc;
    if (int rc = scale_lim(degree, bits, lim, round)) return rc;
    if (n == 0) return INA_OK;
    SrcPlain<X> src;
    bool al;
    if (int rc = fill_pack(src.in, xs, W, al)) return rc;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    hipStream_t s = hs(stream);
    int shift;
    if (vec_v(V, shift) && src_aligned(src.in, W) && (!base || aligned16(base))) {
        hipLaunchKernelGGL(k_blk_scales<SrcPlain<X>>, dim3(grid_of((n + 3) / 4, stream_grid_cap())), dim3(kBlk), 0, s,
                           src, W, base, n, shift, lim, kblk);
    } else {
        ScalarArgs<SrcPlain<X>> a{src, W, 0, base, nullptr, kblk, lim, nullptr, n, (size_t)V, nullptr, 0.f};
        launch_scalar<S_SCALES, K_AUTO>(a, s);
    }
    return launched();
}

// SR (include/ina_blk_sr.h): every summand rounded stochastically under *sr, the scales under
// ina_scale_for_sr's rule, the stochastic checks after the sibling's, every grid under the default cap
template <typename X, bool SR = false, typename B>
int reduce_i32(const B* const* bufs, int W, int8_t* kblk, int mode, int degree, int V, int32_t* out, size_t n,
               ina_stream_t stream, const ina_sr_t* sr = nullptr) {
    using Src = std::conditional_t<SR, SrcSr<X>, SrcPlain<X>>;
    double lim;
    if (int rc = check_v(V)) return rc;
    if (int rc = check_mode(mode, kblk, degree, 32, lim, SR ? 1.0 : 0.5)) return rc;
    if (n == 0) return INA_OK;
    Src src;
    bool al;
    if (int rc = fill_pack(src.in, bufs, W, al)) return rc;
    if (!out) return set_error(INA_EINVAL, "null out%s", "");
    if constexpr (SR) {
        if (int rc = sr_key(sr, src.key)) return rc;
    }
    hipStream_t s = hs(stream);
    const bool autok = mode == INA_BLK_AUTO;
    int shift;
    if (vec_v(V, shift) && src_aligned(src.in, W) && aligned16(out)) {
        // the sibling's grids: covering for W <= 8, the streaming cap beyond
        const dim3 g(grid_of((n + 3) / 4, SR ? default_grid_cap() : W <= 8 ? ew_grid_cap() : stream_grid_cap())), b(kBlk);
#define L(WW)                                                                                                 \
    do {                                                                                                      \
        if (autok) hipLaunchKernelGGL((k_qr_blk_i32<Src, WW, K_AUTO>), g, b, 0, s, src, W, 0, kblk, lim, out, n, shift); \
        else hipLaunchKernelGGL((k_qr_blk_i32<Src, WW, K_GIVEN>), g, b, 0, s, src, W, 0, kblk, lim, out, n, shift); \
    } while (0)
        INA_BLK_W_SWITCH(W, L)
#undef L
    } else {
        ScalarArgs<Src> a{src, W, 0, nullptr, nullptr, kblk, lim, out, n, (size_t)V, nullptr, 0.f};
        if (autok) launch_scalar<S_Q32, K_AUTO>(a, s);
        else launch_scalar<S_Q32, K_GIVEN>(a, s);
    }
    return launched();
}

template <typename X, bool SR = false, typename B>
int reduce_i16(const B* const* bufs, int W, int8_t* kblk, int mode, int degree, int V, int16_t* out, size_t n,
               uint8_t* ovf, ina_stream_t stream, const ina_sr_t* sr = nullptr) {
    using Src = std::conditional_t<SR, SrcSr<X>, SrcPlain<X>>;
    double lim;
    if (int rc = check_v(V)) return rc;
    if (int rc = check_mode(mode, kblk, degree, 16, lim, SR ? 1.0 : 0.5)) return rc;
    if (n == 0) return INA_OK;
    Src src;
    bool al;
    if (int rc = fill_pack(src.in, bufs, W, al)) return rc;
    if (!out) return set_error(INA_EINVAL, "null out%s", "");
    if constexpr (SR) {
        if (int rc = sr_key(sr, src.key)) return rc;
    }
    hipStream_t s = hs(stream);
    const bool autok = mode == INA_BLK_AUTO;
    int shift;
    // (out is stored 8 bytes a lane; beside fp32 buckets it keeps the 16-byte rule it always had)
    // W = 16: AUTO takes the re-read instance, for its registers; under stochastic rounding so do the
    // given scales, whose unrolled W = 16 instance with its 32 Philox calls came out at one wave a SIMD
    if (vec_v(V, shift) && src_aligned(src.in, W) && (uintptr_t)out % (4 * sizeof(X)) == 0) {
        const dim3 g(grid_of((n + 511) / 512 * 64, default_grid_cap())), b(kBlk);
#define L(WW)                                                                                                          \
    do {                                                                                                               \
        if (autok) hipLaunchKernelGGL((k_qr_blk_i16<Src, (WW <= 8 ? WW : 0), K_AUTO>), g, b, 0, s, src, W, 0, kblk, lim, out, n, shift, V, ovf); \
        else hipLaunchKernelGGL((k_qr_blk_i16<Src, ((SR && WW > 8) ? 0 : WW), K_GIVEN>), g, b, 0, s, src, W, 0, kblk, lim, out, n, shift, V, ovf); \
    } while (0)
        INA_BLK_W_SWITCH(W, L)
#undef L
    } else {
        ScalarArgs<Src> a{src, W, 0, nullptr, nullptr, kblk, lim, out, n, (size_t)V, ovf, 0.f};
        if (autok) launch_scalar<S_Q16, K_AUTO>(a, s);
        else launch_scalar<S_Q16, K_GIVEN>(a, s);
    }
    return launched();
}

// one bucket with given scales: the reduce of one
template <typename X, bool SR = false, typename B>
int quantize_i32(const B* x, const int8_t* kblk, int V, int32_t* q, size_t n, ina_stream_t stream,
                 const ina_sr_t* sr = nullptr) {
    if (int rc = check_v(V)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q || !kblk) return set_error(INA_EINVAL, "null pointer%s", "");
    const B* one[1] = {x};
    return reduce_i32<X, SR>(one, 1, const_cast<int8_t*>(kblk), INA_BLK_GIVEN, 1, V, q, n, stream, sr);
}
// the sharded int16 wire's words of one bucket, rounded stochastically (include/ina_blk_sr.h): the
// round-to-nearest sibling's checks (ina_shard.hip), then the stochastic ones
template <typename X, typename B>
int quantize_wire_sr(const B* x, const int8_t* kblk, int V, int32_t* wire, size_t n, const ina_sr_t* sr,
                     ina_stream_t stream) {
    using Src = SrcSr<X, true>;
    if (int rc = check_v(V)) return rc;
    if (n == 0) return INA_OK;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    if (!x || !wire) return set_error(INA_EINVAL, "null pointer%s", "");
    Src src;
    bool al;
    const B* one[1] = {x};
    if (int rc = fill_pack(src.in, one, 1, al)) return rc;
    if (int rc = sr_key(sr, src.key)) return rc;
    hipStream_t s = hs(stream);
    int8_t* kb = const_cast<int8_t*>(kblk);
    int shift;
    if (vec_v(V, shift) && src_aligned(src.in, 1) && aligned16(wire)) {
        hipLaunchKernelGGL((k_qr_blk_i32<Src, 1, K_GIVEN>), dim3(grid_of((n + 3) / 4, default_grid_cap())), dim3(kBlk), 0,
                           s, src, 1, 0, kb, 1.0, wire, n, shift);
    } else {
        ScalarArgs<Src> a{src, 1, 0, nullptr, nullptr, kb, 1.0, wire, n, (size_t)V, nullptr, 0.f};
        launch_scalar<S_Q32, K_GIVEN>(a, s);
    }
    return launched();
}
template <typename X, typename B>
int quantize_i16(const B* x, const int8_t* kblk, int V, int16_t* q, size_t n, uint8_t* ovf, ina_stream_t stream) {
    if (int rc = check_v(V)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q || !kblk) return set_error(INA_EINVAL, "null pointer%s", "");
    const B* one[1] = {x};
    return reduce_i16<X>(one, 1, const_cast<int8_t*>(kblk), INA_BLK_GIVEN, 1, V, q, n, ovf, stream);
}

// T: int32_t or int16_t; Y: float or h16<YT>.  The vector path loads and stores a lane's 4 values at once.
template <typename Y, typename T, typename B>
int dequantize(const T* sv, const int8_t* kblk, int V, B* y, size_t n, ina_stream_t stream) {
    if (int rc = check_v(V)) return rc;
    if (n == 0) return INA_OK;
    if (!sv || !y || !kblk) return set_error(INA_EINVAL, "null pointer%s", "");
    if (sizeof(Y) == 2 && ((uintptr_t)y & 1u)) return set_error(INA_EINVAL, "16-bit buffers must be 2-byte aligned%s", "");
    int shift;
    if (vec_v(V, shift) && (uintptr_t)sv % (4 * sizeof(T)) == 0 && (uintptr_t)y % (4 * sizeof(Y)) == 0) {
        hipLaunchKernelGGL((k_dq_blk<T, Y>), dim3(grid_of((n + 3) / 4, ew_grid_cap())), dim3(kBlk), 0, hs(stream), sv,
                           kblk, static_cast<Y*>(y), n, shift);
    } else {
        ScalarArgs<SrcPlain<Y>> a{{}, 0, 0, nullptr, sv, const_cast<int8_t*>(kblk), 1.0, y, n, (size_t)V, nullptr, 0.f};
        if constexpr (sizeof(T) == 4) launch_scalar<S_DQ32, K_GIVEN>(a, hs(stream));
        else launch_scalar<S_DQ16, K_GIVEN>(a, hs(stream));
    }
    return launched();
}

}  // namespace

// ---------------------------------------------------------------------------
// error feedback (include/ina_ef.h): the EF instances of the kernels above, W = 1.  The entry
// points and their checks are in ina_ef.hip.  Every launch is under the default grid cap.
// ---------------------------------------------------------------------------
namespace {
int launched_ef() { return check_launch("error-feedback kernel launch"); }

// WIRE: q holds the sharded int16 wire's int32 words (fp32 bucket, no base)
template <typename X, typename Q, int KM, bool WIRE = false>
int ef_launch(const EfQuant& c, hipStream_t s) {
    using Src = std::conditional_t<WIRE, SrcEfWire, SrcEf<X, 1>>;
    static_assert(!WIRE || (std::is_same_v<X, float> && sizeof(Q) == 4 && KM != K_AUTO), "fp32 -> int32 words, k given");
    Src src;
    src.x[0] = static_cast<const X*>(c.x);
    src.resid[0] = c.resid;
    src.base = c.base;
    Q* q = static_cast<Q*>(c.q);
    // the vector path where the lane layout fits V (global k: the slots of the int16 flags, if any
    // are asked for), and a lane's 4 values of x, r, base and q are one load or store each
    int shift = 0;
    const bool fits = KM == K_GLOBAL ? (sizeof(Q) == 4 || !c.ovf || slot_ballot_ok(c.V)) : vec_v(c.V, shift);
    if (fits && (uintptr_t)c.x % (4 * sizeof(X)) == 0 && aligned16(c.resid) && (!c.base || aligned16(c.base)) &&
        (uintptr_t)q % (4 * sizeof(Q)) == 0) {
        const dim3 b(kBlk);
        if constexpr (sizeof(Q) == 4) {
            hipLaunchKernelGGL((k_qr_blk_i32<Src, 1, KM>), dim3(grid_of((c.n + 3) / 4, default_grid_cap())), b, 0, s, src,
                               1, c.k, c.kblk, c.lim, q, c.n, shift);
        } else {
            hipLaunchKernelGGL((k_qr_blk_i16<Src, 1, KM>), dim3(grid_of((c.n + 511) / 512 * 64, default_grid_cap())), b,
                               0, s, src, 1, c.k, c.kblk, c.lim, q, c.n, shift, c.V, c.ovf);
        }
    } else {
        ScalarArgs<Src> a{src, 1, c.k, nullptr, nullptr, c.kblk, c.lim, q, c.n, (size_t)c.V, c.ovf, 0.f};
        launch_scalar<sizeof(Q) == 4 ? S_Q32 : S_Q16, KM>(a, s);
    }
    return launched_ef();
}
// block scales are for fp32 buckets only (include/ina_ef.h)
template <typename X, typename Q>
int ef_launch_km(const EfQuant& c, hipStream_t s) {
    if constexpr (std::is_same_v<X, float>) {
        if (c.km == K_GIVEN) return ef_launch<X, Q, K_GIVEN>(c, s);
        if (c.km == K_AUTO) return ef_launch<X, Q, K_AUTO>(c, s);
    }
    return ef_launch<X, Q, K_GLOBAL>(c, s);
}
template <typename X>
int ef_launch_q(const EfQuant& c, hipStream_t s) {
    return c.bits == 32 ? ef_launch_km<X, int32_t>(c, s) : ef_launch_km<X, int16_t>(c, s);
}
}  // namespace

int ef_quantize(const EfQuant& c, ina_stream_t stream) {
    hipStream_t s = hs(stream);
    if (c.wire)
        return c.km == K_GIVEN ? ef_launch<float, int32_t, K_GIVEN, true>(c, s)
                               : ef_launch<float, int32_t, K_GLOBAL, true>(c, s);
    if (c.xtype == INA_X16_BF16) return ef_launch_q<bf16_t>(c, s);
    if (c.xtype == INA_X16_F16) return ef_launch_q<fp16_t>(c, s);
    return ef_launch_q<float>(c, s);
}

int ef_block_scales(const PtrPack<float>& xs, const PtrPack<float>& rs, int W, bool aligned, const float* base,
                    size_t n, int V, double lim, int8_t* kblk, ina_stream_t stream) {
    using Src = SrcEf<float, INA_MAX_WORKERS>;
    Src src;
    for (int w = 0; w < INA_MAX_WORKERS; ++w) {
        src.x[w] = xs.p[w];
        src.resid[w] = const_cast<float*>(rs.p[w]);
    }
    src.base = base;
    hipStream_t s = hs(stream);
    int shift;
    if (vec_v(V, shift) && aligned && (!base || aligned16(base))) {
        hipLaunchKernelGGL(k_blk_scales<Src>, dim3(grid_of((n + 3) / 4, default_grid_cap())), dim3(kBlk), 0, s, src, W,
                           nullptr, n, shift, lim, kblk);
    } else {
        ScalarArgs<Src> a{src, W, 0, nullptr, nullptr, kblk, lim, nullptr, n, (size_t)V, nullptr, 0.f};
        launch_scalar<S_SCALES, K_AUTO>(a, s);
    }
    return launched_ef();
}

}  // namespace ina

using namespace ina;

extern "C" {

int ina_block_scales_f32(const float* const* xs, int W, const float* base, size_t n, int V, int degree, int bits,
                         int8_t* kblk, ina_stream_t stream) {
    return block_scales<float>(xs, W, base, n, V, degree, bits, kblk, stream);
}

// the same kernels with ina_scale_for_sr's lim (include/ina_pkt_sr.h)
int ina_block_scales_sr_f32(const float* const* xs, int W, const float* base, size_t n, int V, int degree, int bits,
                            int8_t* kblk, ina_stream_t stream) {
    return block_scales<float>(xs, W, base, n, V, degree, bits, kblk, stream, 1.0);
}

int ina_quantize_blk_f32_i32(const float* x, const int8_t* kblk, int V, int32_t* q, size_t n, ina_stream_t stream) {
    return quantize_i32<float>(x, kblk, V, q, n, stream);
}

int ina_quantize_blk_f32_i16_sat(const float* x, const int8_t* kblk, int V, int16_t* q, size_t n, uint8_t* ovf,
                                 ina_stream_t stream) {
    return quantize_i16<float>(x, kblk, V, q, n, ovf, stream);
}

int ina_quantize_reduce_blk_f32_i32(const float* const* bufs, int W, int8_t* kblk, int mode, int degree, int V,
                                    int32_t* out, size_t n, ina_stream_t stream) {
    return reduce_i32<float>(bufs, W, kblk, mode, degree, V, out, n, stream);
}

int ina_quantize_reduce_blk_f32_i16_sat(const float* const* bufs, int W, int8_t* kblk, int mode, int degree, int V,
                                        int16_t* out, size_t n, uint8_t* ovf, ina_stream_t stream) {
    return reduce_i16<float>(bufs, W, kblk, mode, degree, V, out, n, ovf, stream);
}

int ina_dequantize_blk_i32_f32(const int32_t* sv, const int8_t* kblk, int V, float* y, size_t n,
                               ina_stream_t stream) {
    return dequantize<float>(sv, kblk, V, y, n, stream);
}

int ina_dequantize_blk_i16_f32(const int16_t* sv, const int8_t* kblk, int V, float* y, size_t n,
                               ina_stream_t stream) {
    return dequantize<float>(sv, kblk, V, y, n, stream);
}

// ---- bf16 / fp16 buckets (include/ina_x16_blk.h): the type code first, then the fp32 sibling's checks ----
int ina_block_scales_x16(const void* const* xs, int xtype, int W, const float* base, size_t n, int V, int degree,
                         int bits, int8_t* kblk, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    return INA_BLK_X16_CALL(xtype, block_scales, xs, W, base, n, V, degree, bits, kblk, stream);
}

int ina_quantize_blk_x16_i32(const void* x, int xtype, const int8_t* kblk, int V, int32_t* q, size_t n,
                             ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    return INA_BLK_X16_CALL(xtype, quantize_i32, x, kblk, V, q, n, stream);
}

int ina_quantize_blk_x16_i16_sat(const void* x, int xtype, const int8_t* kblk, int V, int16_t* q, size_t n,
                                 uint8_t* ovf, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    return INA_BLK_X16_CALL(xtype, quantize_i16, x, kblk, V, q, n, ovf, stream);
}

int ina_quantize_reduce_blk_x16_i32(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode, int degree,
                                    int V, int32_t* out, size_t n, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    return INA_BLK_X16_CALL(xtype, reduce_i32, bufs, W, kblk, mode, degree, V, out, n, stream);
}

int ina_quantize_reduce_blk_x16_i16_sat(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode, int degree,
                                        int V, int16_t* out, size_t n, uint8_t* ovf, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    return INA_BLK_X16_CALL(xtype, reduce_i16, bufs, W, kblk, mode, degree, V, out, n, ovf, stream);
}

int ina_dequantize_blk_i32_x16(const int32_t* sv, const int8_t* kblk, int V, void* y, int ytype, size_t n,
                               ina_stream_t stream) {
    if (int rc = check_x16_type(ytype)) return rc;
    return INA_BLK_X16_CALL(ytype, dequantize, sv, kblk, V, y, n, stream);
}

int ina_dequantize_blk_i16_x16(const int16_t* sv, const int8_t* kblk, int V, void* y, int ytype, size_t n,
                               ina_stream_t stream) {
    if (int rc = check_x16_type(ytype)) return rc;
    return INA_BLK_X16_CALL(ytype, dequantize, sv, kblk, V, y, n, stream);
}

// ---- stochastic rounding (include/ina_blk_sr.h): the siblings above with the ina_sr_t before the stream ----
int ina_block_scales_sr_x16(const void* const* xs, int xtype, int W, const float* base, size_t n, int V, int degree,
                            int bits, int8_t* kblk, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    return INA_BLK_X16_CALL(xtype, block_scales, xs, W, base, n, V, degree, bits, kblk, stream, 1.0);
}

int ina_quantize_blk_sr_f32_i32(const float* x, const int8_t* kblk, int V, int32_t* q, size_t n, const ina_sr_t* sr,
                                ina_stream_t stream) {
    return quantize_i32<float, true>(x, kblk, V, q, n, stream, sr);
}

int ina_quantize_blk_sr_x16_i32(const void* x, int xtype, const int8_t* kblk, int V, int32_t* q, size_t n,
                                const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (xtype == INA_X16_BF16) return quantize_i32<bf16_t, true>(x, kblk, V, q, n, stream, sr);
    return quantize_i32<fp16_t, true>(x, kblk, V, q, n, stream, sr);
}

int ina_quantize_blk_sr_f32_i16_wire(const float* x, const int8_t* kblk, int V, int32_t* wire, size_t n,
                                     const ina_sr_t* sr, ina_stream_t stream) {
    return quantize_wire_sr<float>(x, kblk, V, wire, n, sr, stream);
}

int ina_quantize_blk_sr_x16_i16_wire(const void* x, int xtype, const int8_t* kblk, int V, int32_t* wire, size_t n,
                                     const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (xtype == INA_X16_BF16) return quantize_wire_sr<bf16_t>(x, kblk, V, wire, n, sr, stream);
    return quantize_wire_sr<fp16_t>(x, kblk, V, wire, n, sr, stream);
}

int ina_quantize_reduce_blk_sr_f32_i32(const float* const* bufs, int W, int8_t* kblk, int mode, int degree, int V,
                                       int32_t* out, size_t n, const ina_sr_t* sr, ina_stream_t stream) {
    return reduce_i32<float, true>(bufs, W, kblk, mode, degree, V, out, n, stream, sr);
}

int ina_quantize_reduce_blk_sr_f32_i16_sat(const float* const* bufs, int W, int8_t* kblk, int mode, int degree, int V,
                                           int16_t* out, size_t n, uint8_t* ovf, const ina_sr_t* sr,
                                           ina_stream_t stream) {
    return reduce_i16<float, true>(bufs, W, kblk, mode, degree, V, out, n, ovf, stream, sr);
}

int ina_quantize_reduce_blk_sr_x16_i32(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode, int degree,
                                       int V, int32_t* out, size_t n, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (xtype == INA_X16_BF16) return reduce_i32<bf16_t, true>(bufs, W, kblk, mode, degree, V, out, n, stream, sr);
    return reduce_i32<fp16_t, true>(bufs, W, kblk, mode, degree, V, out, n, stream, sr);
}

int ina_quantize_reduce_blk_sr_x16_i16_sat(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode,
                                           int degree, int V, int16_t* out, size_t n, uint8_t* ovf,
                                           const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (xtype == INA_X16_BF16) return reduce_i16<bf16_t, true>(bufs, W, kblk, mode, degree, V, out, n, ovf, stream, sr);
    return reduce_i16<fp16_t, true>(bufs, W, kblk, mode, degree, V, out, n, ovf, stream, sr);
}

int ina_ps_apply_blk_i32(const float* local, const int32_t* sum_int, const int8_t* kblk, int V, double weight_step,
                         float* out, size_t n, ina_stream_t stream) {
    if (int rc = check_v(V)) return rc;
    if (n == 0) return INA_OK;
    if (!local || !sum_int || !out || !kblk) return set_error(INA_EINVAL, "null pointer%s", "");
    int shift;
    if (vec_v(V, shift) && aligned16(local) && aligned16(sum_int) && aligned16(out)) {
        hipLaunchKernelGGL(k_ps_apply_blk, dim3(grid_of((n + 3) / 4, ew_grid_cap())), dim3(kBlk), 0, hs(stream), local,
                           sum_int, kblk, (float)weight_step, out, n, shift);
    } else {
        ScalarArgs<SrcPlain<float>> a{{}, 0, 0, local, sum_int, const_cast<int8_t*>(kblk), 1.0, out, n, (size_t)V, nullptr,
                                      (float)weight_step};
        launch_scalar<S_APPLY, K_GIVEN>(a, hs(stream));
    }
    return launched();
}

int ina_ps_combine_ina_blk_f32(const float* local, const float* const* paras, int W, int V, double weight_step,
                               float* out, size_t n, int8_t* kblk_out, ina_stream_t stream) {
    if (int rc = check_v(V)) return rc;
    if (n == 0) return INA_OK;
    PtrPack<float> pk;
    bool al;
    if (int rc = fill_pack(pk, paras, W, al)) return rc;
    if (!local || !out) return set_error(INA_EINVAL, "null pointer%s", "");
    double lim;
    if (int rc = scale_lim(W, 32, lim)) return rc;
    hipStream_t s = hs(stream);
    const float ws = (float)weight_step;
    int shift;
    if (vec_v(V, shift) && al && aligned16(local) && aligned16(out)) {
        const dim3 g(grid_of((n + 3) / 4, combine_ina_grid_cap())), b(kBlk);
#define L(WW) hipLaunchKernelGGL(k_ps_combine_ina_blk<WW>, g, b, 0, s, local, pk, W, lim, ws, out, n, shift, kblk_out)
        INA_BLK_W_SWITCH(W, L)
#undef L
    } else {
        ScalarArgs<SrcPlain<float>> a{{pk}, W, 0, local, nullptr, kblk_out, lim, out, n, (size_t)V, nullptr, ws};
        launch_scalar<S_COMB, K_AUTO>(a, s);
    }
    return launched();
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_blk() { return take_store_violations(); }
#endif
