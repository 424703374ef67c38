// ina_shard.hip -- the int16 saturating wire under slot-range sharding (SURVEY.md 8e,
// BASELINE config 4 semantics carried across GPUs).
//
// The switch's narrow path marks a slot whose sum does not fit with the ngaa_h overflow
// bit (headers.p4:30) while the Processor add itself is a plain register add
// (processor.p4:14-24).  On one GPU the int16 path accumulates the W workers exactly in
// int32 and saturates once (ina_quantize_reduce_f32_i16_sat).  Across GPUs the sum goes
// through an RCCL reduce-scatter, and saturation is not associative, so the ranks never
// reduce int16 values: each rank widens its saturated int16 quantisation into one int32
// "wire" word
//
//     wire = q16(x) + (sat(x) << 22)      sat = 1 when x clamped or was NaN
//
// and the wires are summed by an ordinary int32 SUM.  With at most 64 ranks the low 22
// bits carry sum q16 in [-2^21, 2^21) exactly and the bits above count the ranks whose
// value saturated, so one collective carries both the sum and the per-element saturation
// flags.  The owner of a shard decodes it once: out = sat16(sum q16), flag = any
// saturation, and the result equals the single-GPU path bit for bit.
//
// Both kernels stream 16 B per lane (global_load_dwordx4, non-temporal: every byte is
// touched once) over a grid-stride loop; HBM-bound at 8 B/value (quantise: 4 in, 4 out)
// and 4 + 2 + 4 B/value (finish: wire in, int16 + fp32 out).  Each has a sibling that takes one
// scale per block of V values (include/ina_shard_blk.h) and reads 1/V byte more per value.
//
// bf16 / fp16 buckets (include/ina_shard_x16.h): every kernel here takes its bucket's element type --
// X of a quantiser's source, Y of a finish's y: float, or ina_chunk.h's h16<XT>.  A lane still owns 4
// values: one 8-byte access on the 16-bit side (512 B contiguous per wave instruction), one 16-byte
// access on the 32-bit side, so a 16-bit quantiser moves 6 B/value and a finish 4 + 2 + 2.  Widening
// is exact and y is rounded once (rne16), so the words are the fp32 instances' on the widened bucket
// and y is theirs rounded.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"

namespace ina {
namespace {

constexpr int kBlk = kHostBlock;
constexpr int32_t kWireHalf = 1 << (kWireShift - 1);

// (q16w, the wire word of one value, and kWireShift are in ina_device.h: the error-feedback wire
// quantisers of include/ina_shard_ef.h, instances of the kernels of ina_blk.hip, run the same one)

// decoded shard value: sum q16 and whether anything saturated (a rank, or the sum)
__device__ __forceinline__ int32_t finish1(uint32_t w, bool& sat) {
    const int32_t s = (int32_t)w;
    const int32_t c = (s + kWireHalf) >> kWireShift;     // ranks that saturated (>= 0)
    const int32_t v = s - (int32_t)((uint32_t)c << kWireShift);
    sat |= c != 0;
    const bool hi = v > 32767, lo = v < -32768;
    sat |= hi | lo;
    return hi ? 32767 : (lo ? -32768 : v);
}

// a whole chunk at element e, checked against n by the caller: ina_chunk.h's load and store (float:
// 16 bytes; h16: 8 bytes, widened / rounded in registers) with their test against n folded away
template <typename X>
__device__ __forceinline__ f32x4 ldw(const X* p, size_t e) {
    return ld4(p, e, e + 4);
}
template <typename Y>
__device__ __forceinline__ void stw(f32x4 f, Y* p, size_t e) {
    st4(f, p, e, e + 4);
}

template <typename X>
__global__ __launch_bounds__(kBlk) void k_quantize_i16_wire(const X* __restrict__ x,
                                                            int32_t* __restrict__ wire, size_t n,
                                                            float s, int vec) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const size_t n4 = vec ? n / 4 : 0;
    u32x4* w4 = reinterpret_cast<u32x4*>(wire);
    for (size_t i = tid; i < n4; i += stride) {
        const f32x4 v = ldw(x, 4 * i);
        u32x4 r;
        r.x = (uint32_t)q16w(v.x, s); r.y = (uint32_t)q16w(v.y, s);
        r.z = (uint32_t)q16w(v.z, s); r.w = (uint32_t)q16w(v.w, s);
        stream_store(r, w4 + i);
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) wire[i] = q16w(ld1(x, i), s);
}

// Summed wire shard -> int16 (out16) and/or dequantised fp32 (y), per-slot flags.
// Lane l of a wave holds the 4 values at 4(base + l); with V/4 a power of two <= 64 a
// slot is V/4 adjacent lanes, and the group's first lane writes the slot's flag from a
// wave ballot (one writer per slot: no atomics, no pre-zeroing).  The trip count is
// uniform per wave so the ballot is convergent.
template <typename Y>
__global__ __launch_bounds__(kBlk) void k_i16_wire_finish_vec(const int32_t* __restrict__ wsum,
                                                              size_t n, float inv, int lps, int V,
                                                              int16_t* __restrict__ out16,
                                                              Y* __restrict__ y,
                                                              uint8_t* __restrict__ ovf) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const int lane = threadIdx.x & 63;
    const size_t nch = (n + 3) / 4;
    for (size_t base = tid & ~(size_t)63; base < nch; base += stride) {
        const size_t i = base + lane;
        const size_t e = 4 * i;
        bool sat = false;
        if (e + 4 <= n) {
            const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wsum) + i);
            const int32_t a = finish1(w.x, sat), b = finish1(w.y, sat);
            const int32_t c = finish1(w.z, sat), d = finish1(w.w, sat);
            if (out16) {
                u32x2 o;
                o.x = (uint32_t)(uint16_t)a | ((uint32_t)b << 16);
                o.y = (uint32_t)(uint16_t)c | ((uint32_t)d << 16);
                stream_store(o, reinterpret_cast<u32x2*>(out16 + e));
            }
            if (y) {
                f32x4 f;
                f.x = (float)a * inv; f.y = (float)b * inv; f.z = (float)c * inv; f.w = (float)d * inv;
                stw(f, y, e);
            }
        } else if (e < n) {
            for (size_t j = e; j < n; ++j) {
                const int32_t r = finish1((uint32_t)wsum[j], sat);
                if (out16) out16[j] = (int16_t)r;
                if (y) st1((float)r * inv, y, j);
            }
        }
        const unsigned long long m = __ballot(sat);
        if (ovf && e < n && (lane & (lps - 1)) == 0) {
            const int g0 = lane & ~(lps - 1);
            const unsigned long long gm = (lps == 64) ? ~0ull : (((1ull << lps) - 1ull) << g0);
            ovf[e / (size_t)V] = (m & gm) ? 1 : 0;
        }
    }
}

// any alignment / any V: flags pre-zeroed by the caller, saturating elements store 1
template <typename Y>
__global__ __launch_bounds__(kBlk) void k_i16_wire_finish_scalar(const int32_t* __restrict__ wsum,
                                                                 size_t n, float inv, int V,
                                                                 int16_t* __restrict__ out16,
                                                                 Y* __restrict__ y,
                                                                 uint8_t* __restrict__ ovf) {
    const size_t stride = (size_t)gridDim.x * kBlk;
    for (size_t i = (size_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += stride) {
        bool sat = false;
        const int32_t r = finish1((uint32_t)wsum[i], sat);
        if (out16) out16[i] = (int16_t)r;
        if (y) st1((float)r * inv, y, i);
        if (sat && ovf) ovf[i / (size_t)V] = 1;
    }
}

// ---------------------------------------------------------------------------
// per-block scales (include/ina_shard_blk.h): the two kernels above with 2^kblk[e / V] for element
// e.  Vector path: V a power of two in [8, 256], so a lane's 16-byte chunk i lies inside block
// i >> shift (shift = log2 V - 2) and the scale is one byte load per chunk, one address per V/4
// adjacent lanes.  The loops are the siblings': whole chunks first, the ragged tail value by value.
// A scale is read only for an element below n, so nothing outside kblk[0 .. ceil(n / V)) is touched.
// ---------------------------------------------------------------------------
template <typename X>
__global__ __launch_bounds__(kBlk) void k_quantize_i16_wire_blk(const X* __restrict__ x,
                                                                const int8_t* __restrict__ kblk,
                                                                int32_t* __restrict__ wire, size_t n,
                                                                int shift) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const size_t n4 = n / 4;
    u32x4* w4 = reinterpret_cast<u32x4*>(wire);
    for (size_t i = tid; i < n4; i += stride) {
        const float s = pow2f(rd_k(kblk, i >> shift));
        const f32x4 v = ldw(x, 4 * i);
        u32x4 r;
        r.x = (uint32_t)q16w(v.x, s); r.y = (uint32_t)q16w(v.y, s);
        r.z = (uint32_t)q16w(v.z, s); r.w = (uint32_t)q16w(v.w, s);
        stream_store(r, w4 + i);
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride)
        wire[i] = q16w(ld1(x, i), pow2f(rd_k(kblk, i >> (shift + 2))));
}

// any alignment / any V
template <typename X>
__global__ __launch_bounds__(kBlk) void k_quantize_i16_wire_blk_scalar(const X* __restrict__ x,
                                                                       const int8_t* __restrict__ kblk,
                                                                       int32_t* __restrict__ wire, size_t n,
                                                                       int V) {
    const size_t stride = (size_t)gridDim.x * kBlk;
    for (size_t i = (size_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += stride)
        wire[i] = q16w(ld1(x, i), pow2f(rd_k(kblk, i / (size_t)V)));
}

// one whole chunk of the finish: 4 wire words at element e -> out16 / y
template <typename Y>
__device__ __forceinline__ void finish4(u32x4 w, float inv, size_t e, int16_t* __restrict__ out16,
                                        Y* __restrict__ y, bool& sat) {
    const int32_t a = finish1(w.x, sat), b = finish1(w.y, sat);
    const int32_t c = finish1(w.z, sat), d = finish1(w.w, sat);
    if (out16) {
        u32x2 o;
        o.x = (uint32_t)(uint16_t)a | ((uint32_t)b << 16);
        o.y = (uint32_t)(uint16_t)c | ((uint32_t)d << 16);
        stream_store(o, reinterpret_cast<u32x2*>(out16 + e));
    }
    if (y) {
        f32x4 f;
        f.x = (float)a * inv; f.y = (float)b * inv; f.z = (float)c * inv; f.w = (float)d * inv;
        stw(f, y, e);
    }
}

// k_i16_wire_finish_vec's layout and one-writer ballot flags (V/4 = 1 << shift lanes per slot).  A
// wave whose 64 chunks are all whole -- every wave but the bucket's last -- takes one wave-uniform
// branch and no per-lane test against n; the last wave tests per lane and finishes the values past
// the last whole chunk one by one.
template <typename Y>
__global__ __launch_bounds__(kBlk) void k_i16_wire_finish_blk_vec(const int32_t* __restrict__ wsum, size_t n,
                                                                  const int8_t* __restrict__ kblk, int shift,
                                                                  int16_t* __restrict__ out16,
                                                                  Y* __restrict__ y,
                                                                  uint8_t* __restrict__ ovf) {
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlk;
    const int lane = threadIdx.x & 63, lps = 1 << shift;
    const size_t n4 = n / 4, nch = (n + 3) / 4;
    const u32x4* w4 = reinterpret_cast<const u32x4*>(wsum);
    for (size_t base = tid & ~(size_t)63; base < nch; base += stride) {
        const size_t i = base + lane;
        const size_t e = 4 * i;
        bool sat = false;
        if (base + 64 <= n4) {                                   // wave-uniform
            const float inv = pow2f(-rd_k(kblk, i >> shift));
            finish4(__builtin_nontemporal_load(w4 + i), inv, e, out16, y, sat);
        } else if (e < n) {
            const float inv = pow2f(-rd_k(kblk, i >> shift));
            if (i < n4) {
                finish4(__builtin_nontemporal_load(w4 + i), inv, e, out16, y, sat);
            } else {
                for (size_t j = e; j < n; ++j) {
                    const int32_t r = finish1((uint32_t)wsum[j], sat);
                    if (out16) out16[j] = (int16_t)r;
                    if (y) st1((float)r * inv, y, j);
                }
            }
        }
        const unsigned long long m = __ballot(sat);
        if (ovf && e < n && (lane & (lps - 1)) == 0) {
            const int g0 = lane & ~(lps - 1);
            const unsigned long long gm = (lps == 64) ? ~0ull : (((1ull << lps) - 1ull) << g0);
            ovf[i >> shift] = (m & gm) ? 1 : 0;
        }
    }
}

// any alignment / any V: flags pre-zeroed by the caller, saturating elements store 1
template <typename Y>
__global__ __launch_bounds__(kBlk) void k_i16_wire_finish_blk_scalar(const int32_t* __restrict__ wsum, size_t n,
                                                                     const int8_t* __restrict__ kblk, int V,
                                                                     int16_t* __restrict__ out16,
                                                                     Y* __restrict__ y,
                                                                     uint8_t* __restrict__ ovf) {
    const size_t stride = (size_t)gridDim.x * kBlk;
    for (size_t i = (size_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += stride) {
        const size_t s = i / (size_t)V;
        bool sat = false;
        const int32_t r = finish1((uint32_t)wsum[i], sat);
        if (out16) out16[i] = (int16_t)r;
        if (y) st1((float)r * pow2f(-rd_k(kblk, s)), y, i);
        if (sat && ovf) ovf[s] = 1;
    }
}

inline bool al(const void* p, unsigned a) { return ((uintptr_t)p % a) == 0; }

// (vec_v, the vector path's block sizes, is in ina_internal.h)

// The launches, one copy for every element type; the entry points below check their arguments first.
// A lane's access to a bucket of X is 4 * sizeof(X) bytes, and so is the alignment its vector path
// needs.  cap: ew_grid_cap() for the fp32 calls; the 16-bit calls also keep under default_grid_cap().
template <typename X>
int launch_quantize_wire(const X* x, int32_t* wire, size_t n, int k, int cap, ina_stream_t stream) {
    const int vec = al(x, 4 * sizeof(X)) && al(wire, 16);
    hipLaunchKernelGGL(k_quantize_i16_wire<X>, dim3(grid_of(vec ? n / 4 + 1 : n, cap)), dim3(kBlk), 0, hs(stream), x,
                       wire, n, ldexpf(1.0f, k), vec);
    return check_launch("quantize_i16_wire");
}

template <typename Y>
int launch_wire_finish(const int32_t* wire_sum, size_t n, int k, int V, int16_t* out16, Y* y,
                       uint8_t* overflow_per_slot, int cap, ina_stream_t stream) {
    hipStream_t s = hs(stream);
    const float inv = ldexpf(1.0f, -k);
    const int l = V / 4;
    const bool ballot = V % 4 == 0 && l >= 1 && l <= 64 && (l & (l - 1)) == 0;
    const bool vec = al(wire_sum, 16) && (!out16 || al(out16, 8)) && (!y || al(y, 4 * sizeof(Y)));
    if (vec && (ballot || !overflow_per_slot)) {
        hipLaunchKernelGGL(k_i16_wire_finish_vec<Y>, dim3(grid_of((n + 3) / 4, cap)), dim3(kBlk), 0, s, wire_sum, n,
                           inv, ballot ? l : 1, V, out16, y, overflow_per_slot);
    } else {
        if (overflow_per_slot &&
            hipMemsetAsync(overflow_per_slot, 0, (n + (size_t)V - 1) / (size_t)V, s) != hipSuccess)
            return set_error(INA_EHIP, "memset overflow flags%s", "");
        hipLaunchKernelGGL(k_i16_wire_finish_scalar<Y>, dim3(grid_of(n, cap)), dim3(kBlk), 0, s, wire_sum, n, inv, V,
                           out16, y, overflow_per_slot);
    }
    return check_launch("i16_wire_finish");
}

template <typename X>
int launch_quantize_wire_blk(const X* x, const int8_t* kblk, int V, int32_t* wire, size_t n, int cap,
                             ina_stream_t stream) {
    int shift;
    if (vec_v(V, shift) && al(x, 4 * sizeof(X)) && al(wire, 16)) {
        hipLaunchKernelGGL(k_quantize_i16_wire_blk<X>, dim3(grid_of(n / 4 + 1, cap)), dim3(kBlk), 0, hs(stream), x,
                           kblk, wire, n, shift);
    } else {
        hipLaunchKernelGGL(k_quantize_i16_wire_blk_scalar<X>, dim3(grid_of(n, cap)), dim3(kBlk), 0, hs(stream), x,
                           kblk, wire, n, V);
    }
    return check_launch("quantize_blk_i16_wire");
}

template <typename Y>
int launch_wire_finish_blk(const int32_t* wire_sum, size_t n, const int8_t* kblk, int V, int16_t* out16, Y* y,
                           uint8_t* overflow_per_slot, int cap, ina_stream_t stream) {
    hipStream_t s = hs(stream);
    int shift;
    if (vec_v(V, shift) && al(wire_sum, 16) && (!out16 || al(out16, 8)) && (!y || al(y, 4 * sizeof(Y)))) {
        hipLaunchKernelGGL(k_i16_wire_finish_blk_vec<Y>, dim3(grid_of((n + 3) / 4, cap)), dim3(kBlk), 0, s, wire_sum,
                           n, kblk, shift, out16, y, overflow_per_slot);
    } else {
        if (overflow_per_slot &&
            hipMemsetAsync(overflow_per_slot, 0, (n + (size_t)V - 1) / (size_t)V, s) != hipSuccess)
            return set_error(INA_EHIP, "memset overflow flags%s", "");
        hipLaunchKernelGGL(k_i16_wire_finish_blk_scalar<Y>, dim3(grid_of(n, cap)), dim3(kBlk), 0, s, wire_sum, n,
                           kblk, V, out16, y, overflow_per_slot);
    }
    return check_launch("i16_wire_finish_blk");
}

// the 16-bit calls' grid cap: the elementwise one, held under tuning key 0 as well
inline int x16_grid_cap() {
    const int a = ew_grid_cap(), b = default_grid_cap();
    return a < b ? a : b;
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

int ina_quantize_f32_i16_wire(const float* x, int32_t* wire, size_t n, int k, ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !wire) return set_error(INA_EINVAL, "null pointer%s", "");
    return launch_quantize_wire(x, wire, n, k, ew_grid_cap(), stream);
}

int ina_i16_wire_finish(const int32_t* wire_sum, size_t n, int k, int V, int16_t* out16, float* y,
                        uint8_t* overflow_per_slot, ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    if (!wire_sum) return set_error(INA_EINVAL, "null pointer%s", "");
    return launch_wire_finish(wire_sum, n, k, V, out16, y, overflow_per_slot, ew_grid_cap(), stream);
}

int ina_quantize_blk_f32_i16_wire(const float* x, const int8_t* kblk, int V, int32_t* wire, size_t n,
                                  ina_stream_t stream) {
    if (V < 1) return set_error(INA_EINVAL, "V must be >= 1%s", "");
    if (n == 0) return INA_OK;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    if (!x || !wire) return set_error(INA_EINVAL, "null pointer%s", "");
    return launch_quantize_wire_blk(x, kblk, V, wire, n, ew_grid_cap(), stream);
}

int ina_i16_wire_finish_blk(const int32_t* wire_sum, size_t n, const int8_t* kblk, int V, int16_t* out16,
                            float* y, uint8_t* overflow_per_slot, ina_stream_t stream) {
    if (V < 1) return set_error(INA_EINVAL, "V must be >= 1%s", "");
    if (n == 0) return INA_OK;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    if (!wire_sum) return set_error(INA_EINVAL, "null pointer%s", "");
    return launch_wire_finish_blk(wire_sum, n, kblk, V, out16, y, overflow_per_slot, ew_grid_cap(), stream);
}

// ---- include/ina_shard_x16.h: the four above with a 16-bit x / y ----

int ina_quantize_x16_i16_wire(const void* x, int xtype, int32_t* wire, size_t n, int k, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !wire) return set_error(INA_EINVAL, "null pointer%s", "");
    if (int rc = check_al2(x)) return rc;
    if (xtype == INA_X16_BF16)
        return launch_quantize_wire(static_cast<const bf16*>(x), wire, n, k, x16_grid_cap(), stream);
    return launch_quantize_wire(static_cast<const f16*>(x), wire, n, k, x16_grid_cap(), stream);
}

int ina_i16_wire_finish_x16(const int32_t* wire_sum, size_t n, int k, int V, int16_t* out16, void* y, int ytype,
                            uint8_t* overflow_per_slot, ina_stream_t stream) {
    if (int rc = check_x16_type(ytype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    if (!wire_sum) return set_error(INA_EINVAL, "null pointer%s", "");
    if (int rc = check_al2(y)) return rc;
    if (ytype == INA_X16_BF16)
        return launch_wire_finish(wire_sum, n, k, V, out16, static_cast<bf16*>(y), overflow_per_slot, x16_grid_cap(),
                                  stream);
    return launch_wire_finish(wire_sum, n, k, V, out16, static_cast<f16*>(y), overflow_per_slot, x16_grid_cap(),
                              stream);
}

int ina_quantize_blk_x16_i16_wire(const void* x, int xtype, const int8_t* kblk, int V, int32_t* wire, size_t n,
                                  ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (V < 1) return set_error(INA_EINVAL, "V must be >= 1%s", "");
    if (n == 0) return INA_OK;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    if (!x || !wire) return set_error(INA_EINVAL, "null pointer%s", "");
    if (int rc = check_al2(x)) return rc;
    if (xtype == INA_X16_BF16)
        return launch_quantize_wire_blk(static_cast<const bf16*>(x), kblk, V, wire, n, x16_grid_cap(), stream);
    return launch_quantize_wire_blk(static_cast<const f16*>(x), kblk, V, wire, n, x16_grid_cap(), stream);
}

int ina_i16_wire_finish_blk_x16(const int32_t* wire_sum, size_t n, const int8_t* kblk, int V, int16_t* out16,
                                void* y, int ytype, uint8_t* overflow_per_slot, ina_stream_t stream) {
    if (int rc = check_x16_type(ytype)) return rc;
    if (V < 1) return set_error(INA_EINVAL, "V must be >= 1%s", "");
    if (n == 0) return INA_OK;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    if (!wire_sum) return set_error(INA_EINVAL, "null pointer%s", "");
    if (int rc = check_al2(y)) return rc;
    if (ytype == INA_X16_BF16)
        return launch_wire_finish_blk(wire_sum, n, kblk, V, out16, static_cast<bf16*>(y), overflow_per_slot,
                                      x16_grid_cap(), stream);
    return launch_wire_finish_blk(wire_sum, n, kblk, V, out16, static_cast<f16*>(y), overflow_per_slot,
                                  x16_grid_cap(), stream);
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_shard() { return take_store_violations(); }
#endif
