// ina_i4.hip -- the 4-bit wire of the sharded step (include/ina_i4.h states the contract): the nibble quantiser
// with its scales, and the two sums of up to 64 ranks' nibble slices -- exact into int16, and rounded to bytes
// under a per-block shift.
//
// Scales and quantiser run in the rotation's lanes (ina_rot.hip), as the byte wire's do (ina_i8.hip): a lane
// owns the 4 values 4l..4l+3 of its wave's 256, a block is V/4 adjacent lanes, the butterfly and the scalar-unit
// signs are ina_rot_device.h's as they are; the scales are k_i8_scales under the limit 6.5 (no kernel of their
// own).  A lane's 4 results are clamped by one v_med3_f32 each at +-7, converted and packed into 16 bits, and
// leave as one 2-byte sc1 store a lane, 128 contiguous bytes a wave.  (Bringing the odd lane's halfword to its
// even neighbour by quad-perm DPP and storing a dword from the even lanes measured 3.7 % slower, DESIGN 4.1t -- as
// the four-lane gather did for bytes)  n is a multiple of V >= 8, so no chunk crosses n; every loop
// has a wave-uniform trip count, and a lane past n carries zeros through every exchange and writes nothing.
//
// The slice sums never unpack a nibble to a 32-bit lane; they are SWAR on two levels.  A lane owns 32 values,
// one 16-byte load a slice.  w ^ 0x88888888 makes every nibble unsigned (v + 8 in [0, 15]); w & 0x0F0F0F0F and
// (w >> 4) & 0x0F0F0F0F are a word's even and odd nibbles as four byte fields each, and plain 32-bit adds
// accumulate them: 6 VALU for 8 values, 0.75 a value and slice where the byte wire spends 1.5.  A byte field
// holds 17 summands at most (17 * 15 = 255), so slices are taken in batches of at most 16, the loads issued up
// to 8 at a time; after a batch & 0x00FF00FF and >> 8 widen the byte fields into 16-bit fields of 16 words,
// which add up the batches (64 * 15 = 960).  G <= 16 is one batch and no second-level add.  The bias 8 G comes
// off once at the end, by a packed 16-bit subtract per word.  Word j of the load then sits in four words of two
// sums each -- values 8j + (0, 4), (2, 6), (1, 5) and (3, 7) -- which is the byte wire's (even, odd) layout
// once more:
//   exact sum    one v_perm_b32 per output word back into element order, four 16-byte stores of int16 a lane.
//   requantiser  packed 16-bit arithmetic on those words, as k_sum_rq_i8 does (ina_i8_gather.hip; its few lines
//                of shift and rounding are copied here, so that kernel's code is untouched): |S| per field and
//                the maximum per load word -- V = 8 is four blocks inside a lane, V = 16 two, V = 32 the lane,
//                V >= 64 is 2 to 8 adjacent lanes by the row-level DPP max of ina_i8_sum_device.h, nothing
//                crosses a row --, the shift from one v_ffbh_u32 plus the bump test, the tie-to-even rounding,
//                four v_perm_b32 per load word into element order, two 16-byte stores of bytes a lane; the
//                block's first lane writes the shift byte.
// G = 2, 4, 8, 16 are compile-time; any other G is a run-time loop over batches.  n mod 32 is 0, 8, 16 or 24:
// the lane after the last whole chunk loads only its 1, 2 or 3 dwords of each slice and stores only their sums.
#include <hip/hip_runtime.h>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"
#include "ina_rot_device.h"
#include "ina_i8_device.h"
#include "ina_i8_sum_device.h"

namespace ina {
namespace {

constexpr int kBlk = 256;
constexpr double kLimI4 = 6.5;   // ina_scale_for_i4: absmax * 2^k + 1/2 <= 7

// ---------------------------------------------------------------------------
// the quantiser
// ---------------------------------------------------------------------------
// clamp(y, -7, 7) as an int; NaN -> 0; sat |= clamped or NaN
__device__ __forceinline__ uint32_t q4_of(float y, bool& sat) {
    const float c = __builtin_amdgcn_fmed3f(y, -7.0f, 7.0f);           // one v_med3_f32
    sat |= !(c == y);
    return (uint32_t)((y != y) ? 0 : (int)c);
}
// clamp(rne(v * s), -7, 7) of 4 values as 4 nibbles, the first the lowest; NaN -> 0; sat |= clamped or NaN
__device__ __forceinline__ uint32_t q4x4(f32x4 v, float s, bool& sat) {
    const uint32_t a = q4_of(q8_round(v.x, s), sat), b = q4_of(q8_round(v.y, s), sat);
    const uint32_t c = q4_of(q8_round(v.z, s), sat), d = q4_of(q8_round(v.w, s), sat);
    return (a & 15u) | ((b & 15u) << 4) | ((c & 15u) << 8) | ((d & 15u) << 12);
}

// ina_device.h's stream_store for a lane's two bytes: the sc1 buffer store of 16 bits at the lane's distance from
// the wave's first active lane's address, under the same contract (a lane's address is not below that lane's) and
// counted the same way in a checked build
__device__ __forceinline__ void stream_store16(uint32_t h, uint8_t* p) {
    const uint64_t a = (uint64_t)(uintptr_t)p, a0 = wave_uniform(a);
#if INA_STORE_CHECK
    if (a < a0 || a - a0 > 0x7FFFFFFFull - 2ull) atomicAdd(&g_store_violations, 1ull);
#endif
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)a0, 0, 0x7FFFFFFF, kRawBufferWord3);
    __builtin_amdgcn_raw_buffer_store_b16((short)h, r, (int)(uint32_t)(a - a0), 0, kAuxSC1);
}

template <typename X, bool ROT>
__global__ __launch_bounds__(kBlk) void k_q4(const X* __restrict__ x, const int8_t* __restrict__ kblk,
                                             uint8_t* __restrict__ q4, size_t n, int shift, int V,
                                             uint8_t* __restrict__ ovf, SrKey key) {
    const size_t nq = n / 4;                                           // even: n is a multiple of 8
    const int lane = threadIdx.x & 63;
    INA_I8_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        f32x4 r = ld4(x, e, n);
        if constexpr (ROT) r = rot_fwd(r, rot_signs(key, 4 * base_, lane), shift, lane);
        const int k = e < n ? rd_k(kblk, i >> shift) : 0;
        bool sat = false;
        const uint32_t h = q4x4(r, pow2f(k), sat);
        if (e < n) stream_store16(h, q4 + 2 * i);
        const unsigned long long m = __ballot(sat);                    // wave-convergent
        if (ovf) write_slot_flags8(m, e < n, e, V, 1 << shift, ovf);
    }
}

// ---------------------------------------------------------------------------
// the slice sums
// ---------------------------------------------------------------------------
constexpr uint32_t kLow4 = 0x0F0F0F0Fu;
constexpr int kBatch = 16;   // slices a byte field takes: 16 * 15 <= 255

// the lane's chunk i (32 values, 16 bytes) of B slices: whole chunks are one 16-byte load; the lane after them
// loads the `rag` (1..3) dwords the slices still hold; any other lane holds zeros
template <int B>
__device__ __forceinline__ void ld_nibbles(const PtrPack<int8_t>& in, int g0, size_t i, size_t nfull, int rag,
                                           u32x4* w) {
    if (i < nfull) {
#pragma unroll
        for (int j = 0; j < B; ++j) w[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in.p[g0 + j]) + i);
    } else {
#pragma unroll
        for (int j = 0; j < B; ++j) w[j] = u32x4{0u, 0u, 0u, 0u};
        if (i == nfull && rag > 0) {
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(in.p[g0 + j]) + 4 * i;
                w[j].x = __builtin_nontemporal_load(p);
                if (rag > 1) w[j].y = __builtin_nontemporal_load(p + 1);
                if (rag > 2) w[j].z = __builtin_nontemporal_load(p + 2);
            }
        }
    }
}
// first level: the even and the odd nibbles of every word into four byte fields each
__device__ __forceinline__ void add_nibbles(u32x4 w, u32x4& ev, u32x4& od) {
    w ^= 0x88888888u;
    ev += w & kLow4;
    od += (w >> 4) & kLow4;
}
template <int B>
__device__ __forceinline__ void add_slices(const PtrPack<int8_t>& in, int g0, size_t i, size_t nfull, int rag,
                                           u32x4& ev, u32x4& od) {
    u32x4 w[B];
    ld_nibbles<B>(in, g0, i, nfull, rag, w);
#pragma unroll
    for (int j = 0; j < B; ++j) add_nibbles(w[j], ev, od);
}

// The sums of a lane's 32 values: 16-bit fields, the low field first.  With j the load word:
//   a[j] values 8j + (0, 4)   b[j] values 8j + (2, 6)   c[j] values 8j + (1, 5)   d[j] values 8j + (3, 7)
struct Sums {
    u32x4 a, b, c, d;
};
// second level: a batch's byte fields widened into the 16-bit fields
template <bool FIRST>
__device__ __forceinline__ void widen(u32x4 ev, u32x4 od, Sums& s) {
    const u32x4 a = ev & kLow8, b = (ev >> 8) & kLow8, c = od & kLow8, d = (od >> 8) & kLow8;
    if constexpr (FIRST) s = Sums{a, b, c, d};
    else s.a += a, s.b += b, s.c += c, s.d += d;
}
__device__ __forceinline__ u32x4 unbias(u32x4 v, int16_t bias) {
    const s16x2 b = {bias, bias};
    return u32x4{word(fields(v.x) - b), word(fields(v.y) - b), word(fields(v.z) - b), word(fields(v.w) - b)};
}
// the signed sums of chunk i over the ng slices; G > 0: ng = G at compile time
template <int G>
__device__ __forceinline__ Sums slice_sums(const PtrPack<int8_t>& in, int ng, size_t i, size_t nfull, int rag) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
    Sums s;
    if constexpr (G > 0) {
        static_assert(G <= kBatch, "one batch");
        constexpr int B = G < 8 ? G : 8;
        u32x4 ev = zero, od = zero;
#pragma unroll
        for (int g0 = 0; g0 < G; g0 += B) add_slices<B>(in, g0, i, nfull, rag, ev, od);
        widen<true>(ev, od, s);
    } else {
        s = Sums{zero, zero, zero, zero};
        for (int g0 = 0; g0 < ng; g0 += kBatch) {                      // wave-uniform: ng is a kernel argument
            const int g1 = min(g0 + kBatch, ng);
            u32x4 ev = zero, od = zero;
            int g = g0;
            for (; g + 8 <= g1; g += 8) add_slices<8>(in, g, i, nfull, rag, ev, od);
            for (; g + 2 <= g1; g += 2) add_slices<2>(in, g, i, nfull, rag, ev, od);
            if (g < g1) add_slices<1>(in, g, i, nfull, rag, ev, od);
            widen<false>(ev, od, s);
        }
    }
    const int16_t bias = (int16_t)(8 * ng);
    return Sums{unbias(s.a, bias), unbias(s.b, bias), unbias(s.c, bias), unbias(s.d, bias)};
}

// (a vector's element by a run of the unrolled loop's index)
__device__ __forceinline__ uint32_t el(u32x4 v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// G > 0: compile-time slice count; G = 0: Gd slices
template <int G>
__global__ __launch_bounds__(kBlk) void k_sum_i4(PtrPack<int8_t> in, int Gd, int16_t* __restrict__ out, size_t n) {
    const int ng = G > 0 ? G : Gd;
    const size_t nfull = n / 32, nq = (n + 31) / 32;
    const int rag = (int)(n & 31) / 8;                                 // the dwords of the chunk after the whole ones
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x, stride = (size_t)gridDim.x * kBlk;
    for (size_t i = tid; i < nq; i += stride) {
        const Sums s = slice_sums<G>(in, ng, i, nfull, rag);
        auto lo = [](uint32_t o, uint32_t e) { return __builtin_amdgcn_perm(o, e, 0x05040100u); };
        auto hi = [](uint32_t o, uint32_t e) { return __builtin_amdgcn_perm(o, e, 0x07060302u); };
        u32x4* o = reinterpret_cast<u32x4*>(out + 32 * i);
        const int nw = i < nfull ? 4 : rag;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                  // load word j: values 8j .. 8j + 7
            const uint32_t a = el(s.a, j), b = el(s.b, j), c = el(s.c, j), d = el(s.d, j);
            if (j < nw) stream_store(u32x4{lo(c, a), lo(d, b), hi(c, a), hi(d, b)}, o + j);
        }
    }
}

// ina_i8_gather.hip's rule, copied: the smallest sh with rne(a / 2^sh) <= 127 (here a <= 512, so sh <= 3)
__device__ __forceinline__ int shift_of(int a) {
    const int s0 = max(0, 25 - (int)__builtin_clz((uint32_t)a | 1u));          // bitlen(a) - 7
    const int r = s0 ? (a + (1 << (s0 - 1)) - 1 + ((a >> s0) & 1)) >> s0 : a;   // rne(a / 2^s0)
    return s0 + (r == 128 ? 1 : 0);
}
// rne(S / 2^sh) in both fields of a word, as there
struct Requant {
    s16x2 sh, bias, tie0;   // sh; 2^(sh-1) - 1 (sh = 0: -1); sh = 0: 1, else 0
};
__device__ __forceinline__ Requant requant_of(int sh) {
    const int16_t s = (int16_t)sh, b = (int16_t)(((1 << sh) >> 1) - 1), t = (int16_t)(sh == 0 ? 1 : 0);
    return Requant{s16x2{s, s}, s16x2{b, b}, s16x2{t, t}};
}
__device__ __forceinline__ uint32_t requant(uint32_t w, const Requant& r) {
    const s16x2 s = fields(w), one = {1, 1};
    return word((s + r.bias + (((s >> r.sh) & one) | r.tie0)) >> r.sh);
}
// the 8 bytes of load word j in element order from its four words of sums
__device__ __forceinline__ u32x2 bytes_of(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const Requant& r) {
    const uint32_t t0 = __builtin_amdgcn_perm(requant(c, r), requant(a, r), 0x06020400u);   // values 0, 1, 4, 5
    const uint32_t t1 = __builtin_amdgcn_perm(requant(d, r), requant(b, r), 0x06020400u);   // values 2, 3, 6, 7
    return u32x2{__builtin_amdgcn_perm(t1, t0, 0x05040100u), __builtin_amdgcn_perm(t1, t0, 0x07060302u)};
}

// G > 0: compile-time slice count; G = 0: Gd slices.  lv = log2 V
template <int G>
__global__ __launch_bounds__(kBlk) void k_sum_rq_i4(PtrPack<int8_t> in, int Gd, int8_t* __restrict__ q8,
                                                    uint8_t* __restrict__ shift, size_t n, int lv) {
    const int ng = G > 0 ? G : Gd;
    const size_t nfull = n / 32, nq = (n + 31) / 32;
    const int rag = (int)(n & 31) / 8;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x, stride = (size_t)gridDim.x * kBlk;
    const int lane = threadIdx.x & 63;
    for (size_t base = tid & ~(size_t)63; base < nq; base += stride) {   // wave-uniform
        const size_t i = base + lane;
        const Sums s = slice_sums<G>(in, ng, i, nfull, rag);             // a lane past n holds zeros
        int m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = absmax4(el(s.a, j), el(s.b, j), el(s.c, j), el(s.d, j));
        if (lv == 4) {
            m[0] = m[1] = max(m[0], m[1]);
            m[2] = m[3] = max(m[2], m[3]);
        } else if (lv > 4) {
            m[0] = m[1] = m[2] = m[3] = row_group_max(max(max(m[0], m[1]), max(m[2], m[3])), lv - 5);
        }
        const int nw = i < nfull ? 4 : i == nfull ? rag : 0;             // the load words this lane holds
        int sh[4];
        u32x2 o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sh[j] = shift_of(m[j]);
            o[j] = bytes_of(el(s.a, j), el(s.b, j), el(s.c, j), el(s.d, j), requant_of(sh[j]));
        }
        int8_t* q = q8 + 32 * i;
        if (nw == 4) {
            stream_store(u32x4{o[0].x, o[0].y, o[1].x, o[1].y}, reinterpret_cast<u32x4*>(q));
            stream_store(u32x4{o[2].x, o[2].y, o[3].x, o[3].y}, reinterpret_cast<u32x4*>(q) + 1);
        } else if (nw > 0) {                                             // V = 8 or 16: the one ragged lane
            if (nw >= 2) stream_store(u32x4{o[0].x, o[0].y, o[1].x, o[1].y}, reinterpret_cast<u32x4*>(q));
            if (nw == 1) stream_store(o[0], reinterpret_cast<u32x2*>(q));
            if (nw == 3) stream_store(o[2], reinterpret_cast<u32x2*>(q) + 2);
        }
        if (lv == 3) {                                                   // blocks 4i .. 4i + 3
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nw) shift[4 * i + j] = (uint8_t)sh[j];
        } else if (lv == 4) {                                            // blocks 2i and 2i + 1
            if (nw >= 2) shift[2 * i] = (uint8_t)sh[0];
            if (nw == 4) shift[2 * i + 1] = (uint8_t)sh[2];
        } else if (nw == 4 && (lane & ((1 << (lv - 5)) - 1)) == 0) {
            shift[(32 * i) >> lv] = (uint8_t)sh[0];
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int launched() { return check_launch("int4 wire kernel launch"); }

template <typename X>
int quantize(const void* x, const int8_t* kblk, int V, uint8_t* q4, size_t n, uint8_t* ovf, const ina_sr_t* sr,
             ina_stream_t stream) {
    int shift;
    if (int rc = check_blocks(V, kblk, n, shift)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q4) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!aligned16(x) || !aligned16(q4)) return misaligned();
    SrKey key{};
    if (sr)
        if (int rc = rot_key(sr, V, key)) return rc;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    const X* xp = static_cast<const X*>(x);
    if (sr) hipLaunchKernelGGL((k_q4<X, true>), g, b, 0, hs(stream), xp, kblk, q4, n, shift, V, ovf, key);
    else hipLaunchKernelGGL((k_q4<X, false>), g, b, 0, hs(stream), xp, kblk, q4, n, shift, V, ovf, key);
    return launched();
}

// the slices as the sums' kernels take them (they only ever load whole words)
const int8_t* const* as_bytes(const uint8_t* const* slices) { return reinterpret_cast<const int8_t* const*>(slices); }

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

int ina_scale_for_i4(float absmax, int* k_out) {
    return scale_for_lim(absmax, k_out, kLimI4);
}

int ina_block_scales_i4(const void* const* xs, int xtype, int W, size_t n, int V, int8_t* kblk, const ina_sr_t* sr,
                        ina_stream_t stream) {
    return block_scales_i8(xs, xtype, W, n, V, kblk, sr, kLimI4, stream);
}

int ina_quantize_i4_wire(const void* x, int xtype, const int8_t* kblk, int V, uint8_t* q4, size_t n,
                         uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_I8_X_CALL(xtype, quantize, x, kblk, V, q4, n, overflow_per_slot, sr, stream);
}

int ina_sum_i4_slices(const uint8_t* const* slices, int G, int16_t* out16, size_t n, ina_stream_t stream) {
    if (!slices || G < 1 || G > INA_MAX_WORKERS) return set_error(INA_EINVAL, "G must be in [1, %s]", "64");
    if (n % 8) return set_error(INA_EINVAL, "n must be a multiple of 8%s", "");
    if (n == 0) return INA_OK;
    PtrPack<int8_t> pk;
    bool al;
    if (int rc = fill_pack(pk, as_bytes(slices), G, al)) return rc;
    if (!out16) return set_error(INA_EINVAL, "null out16%s", "");
    if (!al || !aligned16(out16)) return misaligned();
    const dim3 g(grid_of((n + 31) / 32, default_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
#define L(GG) hipLaunchKernelGGL(k_sum_i4<GG>, g, b, 0, s, pk, G, out16, n)
    switch (G) {
        case 2: L(2); break;
        case 4: L(4); break;
        case 8: L(8); break;
        case 16: L(16); break;
        default: L(0);
    }
#undef L
    return launched();
}

int ina_sum_i4_slices_requant(const uint8_t* const* slices, int G, int V, int8_t* q8, uint8_t* shift, size_t n,
                              ina_stream_t stream) {
    PtrPack<int8_t> pk;
    int lv;
    if (int rc = check_sum_rq(as_bytes(slices), G, V, q8, shift, n, pk, lv)) return rc;
    if (n == 0) return INA_OK;
    const dim3 g(grid_of((n + 31) / 32, default_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
#define L(GG) hipLaunchKernelGGL(k_sum_rq_i4<GG>, g, b, 0, s, pk, G, q8, shift, n, lv)
    switch (G) {
        case 2: L(2); break;
        case 4: L(4); break;
        case 8: L(8); break;
        case 16: L(16); break;
        default: L(0);
    }
#undef L
    return launched();
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_i4() { return take_store_violations(); }
#endif
