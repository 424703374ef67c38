// ina_i8.hip -- the 8-bit wire of the sharded step (include/ina_i8.h states the contract): the byte
// quantiser with its scales, and the exact int16 sum of up to 64 ranks' byte slices.
//
// Scales and quantiser run in the rotation's lanes (ina_rot.hip): a lane owns the 16-byte chunk of 4 values
// 4l..4l+3 of its wave's 256, a block is V/4 adjacent lanes, the butterfly and the scalar-unit signs are
// ina_rot_device.h's as they are.  ROT = false (sr == NULL) is an arm of its own with no butterfly and no
// signs.  A lane's 4 results are clamped by one v_med3_f32 each, converted, packed two by two
// (v_cvt_pk_i16_i32) and their low bytes gathered by one v_perm_b32: one dword a lane, 256 contiguous bytes a
// wave (collecting four lanes' dwords by quad-perm DPP into one 16-byte store per fourth lane measured 3-7 %
// slower).  n is a multiple of V >= 8, so no chunk crosses n; every loop has a wave-uniform trip
// count, and a lane past n carries zeros through every exchange and writes nothing.
//
// The slice sum never unpacks a byte to a 32-bit lane.  A lane loads 16 bytes of each slice; w ^ 0x80808080
// makes every byte unsigned, w & 0x00FF00FF and (w >> 8) & 0x00FF00FF are its even and odd bytes as two 16-bit
// fields each, and plain 32-bit adds accumulate them: a field starts at 0x8000 - 128 G and gains at most
// 255 G, so it ends below 0x8000 + 127 * 64 and never carries into its neighbour.  Flipping each field's
// top bit afterwards leaves sum - 128 G + 128 G = the signed sum as an int16 (|sum| <= 8192), and one
// v_perm_b32 per output word puts even and odd fields back in element order: about 1.5 VALU a value and
// slice.  G = 2, 4, 8, 16 are compile-time (loads issued up to 8 at a time, then the adds); any other G runs
// a loop with two slices' loads in flight.  The n mod 16 values of a ragged tail are summed value by value by
// the grid's last lanes.
#include <hip/hip_runtime.h>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"
#include "ina_rot_device.h"
#include "ina_i8_device.h"

namespace ina {
namespace {

constexpr int kBlk = 256;

// r of the contract for the lane's chunk
template <bool ROT>
__device__ __forceinline__ f32x4 rotated(f32x4 x, const SrKey& key, size_t e256, int shift, int lane) {
    if constexpr (ROT) return rot_fwd(x, rot_signs(key, e256, lane), shift, lane);
    else return x;
}

template <typename X, bool ROT>
__global__ __launch_bounds__(kBlk) void k_i8_scales(PtrPack<X> xs, int W, size_t n, int shift, double lim, SrKey key,
                                                    int8_t* __restrict__ kblk) {
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_I8_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        [[maybe_unused]] u32x4 sg = {0u, 0u, 0u, 0u};
        if constexpr (ROT) sg = rot_signs(key, 4 * base_, lane);
        auto r = [&](f32x4 x) {
            if constexpr (ROT) return rot_fwd(x, sg, shift, lane);
            else return x;
        };
        uint32_t m = 0u;
        int w = 0;
        for (; w + 2 <= W; w += 2) {                                   // two buckets' loads in flight
            const f32x4 a = ld4(xs.p[w], e, n), b = ld4(xs.p[w + 1], e, n);
            m = fold4(fold4(m, r(a)), r(b));
        }
        if (w < W) m = fold4(m, r(ld4(xs.p[w], e, n)));
        m = group_max(m, 1 << shift);
        if (e < n && (lane & ((1 << shift) - 1)) == 0) kblk[i >> shift] = (int8_t)scale_of(m, lim);
    }
}

template <typename X, bool ROT>
__global__ __launch_bounds__(kBlk) void k_q8(const X* __restrict__ x, const int8_t* __restrict__ kblk,
                                             int8_t* __restrict__ q8, size_t n, int shift, int V,
                                             uint8_t* __restrict__ ovf, SrKey key) {
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_I8_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        const f32x4 r = rotated<ROT>(ld4(x, e, n), key, 4 * base_, shift, lane);
        const int k = e < n ? rd_k(kblk, i >> shift) : 0;
        bool sat = false;
        const uint32_t d = q8x4(r, pow2f(k), sat);
        if (e < n) stream_store(d, reinterpret_cast<uint32_t*>(q8 + e));
        const unsigned long long m = __ballot(sat);                    // wave-convergent
        if (ovf) write_slot_flags8(m, e < n, e, V, 1 << shift, ovf);
    }
}

// ---------------------------------------------------------------------------
// the slice sum
// ---------------------------------------------------------------------------
constexpr uint32_t kTop16 = 0x80008000u, kLow8 = 0x00FF00FFu;

__device__ __forceinline__ u32x4 ld16b(const int8_t* p, size_t i) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + i);
}
__device__ __forceinline__ void add_bytes(u32x4 w, u32x4& ev, u32x4& od) {
    w ^= 0x80808080u;
    ev += w & kLow8;
    od += (w >> 8) & kLow8;
}

// G > 0: compile-time slice count; G = 0: Gd slices
template <int G>
__global__ __launch_bounds__(kBlk) void k_sum_i8(PtrPack<int8_t> in, int Gd, int16_t* __restrict__ out, size_t n) {
    const int ng = G > 0 ? G : Gd;
    const size_t nq = n / 16;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x, stride = (size_t)gridDim.x * kBlk;
    const uint32_t init = kTop16 - (uint32_t)ng * 128u * 0x00010001u;
    for (size_t i = tid; i < nq; i += stride) {
        u32x4 ev = {init, init, init, init}, od = ev;
        if constexpr (G > 0) {
            constexpr int B = G < 8 ? G : 8;
#pragma unroll
            for (int g0 = 0; g0 < G; g0 += B) {
                u32x4 w[B];
#pragma unroll
                for (int j = 0; j < B; ++j) w[j] = ld16b(in.p[g0 + j], i);
#pragma unroll
                for (int j = 0; j < B; ++j) add_bytes(w[j], ev, od);
            }
        } else {
            int g = 0;
            for (; g + 2 <= ng; g += 2) {                              // two slices' loads in flight
                const u32x4 a = ld16b(in.p[g], i), b = ld16b(in.p[g + 1], i);
                add_bytes(a, ev, od);
                add_bytes(b, ev, od);
            }
            if (g < ng) add_bytes(ld16b(in.p[g], i), ev, od);
        }
        ev ^= kTop16;
        od ^= kTop16;
        // word j of ev holds values 4j and 4j+2, of od 4j+1 and 4j+3
        auto lo = [](uint32_t o, uint32_t e) { return __builtin_amdgcn_perm(o, e, 0x05040100u); };
        auto hi = [](uint32_t o, uint32_t e) { return __builtin_amdgcn_perm(o, e, 0x07060302u); };
        u32x4* o = reinterpret_cast<u32x4*>(out + 16 * i);
        stream_store(u32x4{lo(od.x, ev.x), hi(od.x, ev.x), lo(od.y, ev.y), hi(od.y, ev.y)}, o);
        stream_store(u32x4{lo(od.z, ev.z), hi(od.z, ev.z), lo(od.w, ev.w), hi(od.w, ev.w)}, o + 1);
    }
    const size_t j = stride - 1 - tid;                                 // the ragged tail: the grid's last lanes
    if (j < (n & 15)) {
        const size_t e = 16 * nq + j;
        int s = 0;
        for (int g = 0; g < ng; ++g) s += (int)in.p[g][e];
        out[e] = (int16_t)s;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int launched() { return check_launch("int8 wire kernel launch"); }

template <typename X>
int block_scales(const void* const* xs, int W, size_t n, int V, int8_t* kblk, const ina_sr_t* sr, double lim,
                 ina_stream_t stream) {
    int shift;
    if (int rc = check_blocks(V, kblk, n, shift)) return rc;
    if (n == 0) return INA_OK;
    PtrPack<X> pk;
    bool al;
    if (int rc = fill_pack(pk, xs, W, al)) return rc;
    if (!al) return misaligned();
    SrKey key{};
    if (sr)
        if (int rc = rot_key(sr, V, key)) return rc;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    if (sr) hipLaunchKernelGGL((k_i8_scales<X, true>), g, b, 0, hs(stream), pk, W, n, shift, lim, key, kblk);
    else hipLaunchKernelGGL((k_i8_scales<X, false>), g, b, 0, hs(stream), pk, W, n, shift, lim, key, kblk);
    return launched();
}

template <typename X>
int quantize(const void* x, const int8_t* kblk, int V, int8_t* q8, size_t n, uint8_t* ovf, const ina_sr_t* sr,
             ina_stream_t stream) {
    int shift;
    if (int rc = check_blocks(V, kblk, n, shift)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q8) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!aligned16(x) || !aligned16(q8)) return misaligned();
    SrKey key{};
    if (sr)
        if (int rc = rot_key(sr, V, key)) return rc;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    const X* xp = static_cast<const X*>(x);
    if (sr) hipLaunchKernelGGL((k_q8<X, true>), g, b, 0, hs(stream), xp, kblk, q8, n, shift, V, ovf, key);
    else hipLaunchKernelGGL((k_q8<X, false>), g, b, 0, hs(stream), xp, kblk, q8, n, shift, V, ovf, key);
    return launched();
}

}  // namespace

int block_scales_i8(const void* const* xs, int xtype, int W, size_t n, int V, int8_t* kblk, const ina_sr_t* sr,
                    double lim, ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_I8_X_CALL(xtype, block_scales, xs, W, n, V, kblk, sr, lim, stream);
}

}  // namespace ina

using namespace ina;

extern "C" {

int ina_scale_for_i8(float absmax, int* k_out) {
    return scale_for_lim(absmax, k_out, kLimI8);
}

int ina_block_scales_i8(const void* const* xs, int xtype, int W, size_t n, int V, int8_t* kblk, const ina_sr_t* sr,
                        ina_stream_t stream) {
    return block_scales_i8(xs, xtype, W, n, V, kblk, sr, kLimI8, stream);
}

int ina_quantize_i8_wire(const void* x, int xtype, const int8_t* kblk, int V, int8_t* q8, size_t n,
                         uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_I8_X_CALL(xtype, quantize, x, kblk, V, q8, n, overflow_per_slot, sr, stream);
}

int ina_sum_i8_slices(const int8_t* const* slices, int G, int16_t* out16, size_t n, ina_stream_t stream) {
    if (!slices || G < 1 || G > INA_MAX_WORKERS) return set_error(INA_EINVAL, "G must be in [1, %s]", "64");
    if (n == 0) return INA_OK;
    PtrPack<int8_t> pk;
    bool al;
    if (int rc = fill_pack(pk, slices, G, al)) return rc;
    if (!out16) return set_error(INA_EINVAL, "null out16%s", "");
    if (!al || !aligned16(out16)) return misaligned();
    const dim3 g(grid_of(n / 16 + 1, default_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
#define L(GG) hipLaunchKernelGGL(k_sum_i8<GG>, g, b, 0, s, pk, G, out16, n)
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
unsigned long long ina::store_violations_i8() { return take_store_violations(); }
#endif
