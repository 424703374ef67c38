// ina_i8_sr.hip -- unbiased stochastic rounding on both halves of the 8-bit wire (include/ina_i8_sr.h states the
// contract): the byte quantiser that rounds the rotated values up or down by chance, the requantising slice sum
// that does the same to the owner's sums in integers, and the scale rule with a whole quantum of headroom.
//
// Quantiser (k_q8_sr<X, ROT>).  The rotation's lanes (ina_rot.hip, ina_i8.hip): a lane owns the chunk of 4 values
// 4l..4l+3 of its wave's 256, a block is V/4 adjacent lanes of one wave.  The lane
//   words  issues its one Philox call first: the counter e0/4 + i depends on nothing the lane loads, the rounding
//          key sits in scalar registers, and the ten rounds' multiplies fill the loads' latency and interleave with
//          the butterfly's cross-lane moves;
//   fwd    loads its chunk (16 bytes, 8 for bf16 / fp16, widened), takes the wave's signs from the scalar unit under
//          the rotation's key and runs the butterfly: rot_signs and rot_fwd of ina_rot_device.h as they are;
//   round  y = floor(t) + (u < t - floor(t)) of t = r * 2^k: sr_y4 of ina_sr_device.h, word j of the call for value j;
//   bytes  one v_med3_f32 a value, v_cvt_pk_i16_i32, v_perm_b32 (q8_of, q8_pack of ina_i8_device.h), one dword
//          store, and the one-writer ballot for the block's flag.
// ROT = false (rot == NULL) is an arm of its own with no butterfly and no signs.  n is a multiple of V >= 8, so no
// chunk crosses n; the trip count is wave-uniform and a lane past n carries zeros and writes nothing.
//
// Slice sum (k_sum_rq_i8_sr<G>).  The front, the block maximum and the stores are k_sum_rq_i8's
// (ina_i8_sum_device.h): a lane owns 16 values, their sums sit as 16-bit fields in 8 words, even bytes' sums in ev,
// odd bytes' in od.  One Philox call a lane at counter e0/16 + i gives 16 random bytes, byte j for value j; its
// four words split into even and odd bytes with the masks that split the data, so the random fields already sit
// under the sums they belong to.  Then per word: v_and with 2^sh - 1 in both fields, v_pk_add_i16, v_pk_ashrrev_i16,
// and the sibling's v_perm_b32 into element order.  (S + u) >> sh rounds up with probability (S mod 2^sh) / 2^sh
// exactly; |S + u| <= 8192 + 127 stays inside a field; sh = 0 masks u to zero and writes S.  No 32-bit lanes, no
// LDS, builtins only.
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

constexpr int kBlk = kI8Blk;

// ---------------------------------------------------------------------------
// the byte quantiser
// ---------------------------------------------------------------------------
template <typename X, bool ROT>
__global__ __launch_bounds__(kBlk) void k_q8_sr(const X* __restrict__ x, const int8_t* __restrict__ kblk,
                                                int8_t* __restrict__ q8, size_t n, int shift, int V,
                                                uint8_t* __restrict__ ovf, SrKey rot, SrKey rnd) {
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_I8_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        const u32x4 w = philox(rnd, rnd.i0 + i);                       // ahead of the loads and the butterfly
        f32x4 r = ld4(x, e, n);
        if constexpr (ROT) r = rot_fwd(r, rot_signs(rot, 4 * base_, lane), shift, lane);
        const int k = e < n ? rd_k(kblk, i >> shift) : 0;
        const f32x4 y = sr_y4(r, pow2f(k), w);
        bool sat = false;
        const int a = q8_of(y.x, sat), b = q8_of(y.y, sat), c = q8_of(y.z, sat), d = q8_of(y.w, sat);
        if (e < n) stream_store(q8_pack(a, b, c, d), reinterpret_cast<uint32_t*>(q8 + e));
        const unsigned long long m = __ballot(sat);                    // wave-convergent
        if (ovf) write_slot_flags8(m, e < n, e, V, 1 << shift, ovf);
    }
}

// ---------------------------------------------------------------------------
// sum + stochastic requantise
// ---------------------------------------------------------------------------
// a field's start: 0x8000 - 128 G, so that bytes made unsigned add up to the signed sum with its top bit flipped
__device__ __forceinline__ uint32_t sum_init(int ng) { return kTop16 - (uint32_t)ng * 128u * 0x00010001u; }
// the signed sums of the lane's chunk i over the slices: word j of ev holds the sums of values 4j and 4j+2, of
// od 4j+1 and 4j+3; init is sum_init(ng).  G > 0: compile-time slice count, up to 8 loads in flight; G = 0: ng
// slices, two in flight.  k_sum_rq_i8 keeps the same steps written out in its loop: folding them into these
// helpers there changed its instances' scalar register counts, and the existing instances stay as they are
template <int G>
__device__ __forceinline__ void sum_chunks(const PtrPack<int8_t>& in, int ng, uint32_t init, size_t i, size_t nfull,
                                           bool half, u32x4& ev, u32x4& od) {
    ev = u32x4{init, init, init, init};
    od = ev;
    if constexpr (G > 0) {
        constexpr int B = G < 8 ? G : 8;
#pragma unroll
        for (int g0 = 0; g0 < G; g0 += B) {
            u32x4 w[B];
            ld_chunks<B>(in, g0, i, nfull, half, w);
#pragma unroll
            for (int j = 0; j < B; ++j) add_bytes(w[j], ev, od);
        }
    } else {
        int g = 0;
        for (; g + 2 <= ng; g += 2) {                                // two slices' loads in flight
            u32x4 w[2];
            ld_chunks<2>(in, g, i, nfull, half, w);
            add_bytes(w[0], ev, od);
            add_bytes(w[1], ev, od);
        }
        if (g < ng) {
            u32x4 w[1];
            ld_chunks<1>(in, g, i, nfull, half, w);
            add_bytes(w[0], ev, od);
        }
    }
    ev ^= kTop16;
    od ^= kTop16;
}

// A of the lane's two half chunks (values 0-7, values 8-15): V = 8 (lv = 3) leaves them apart, a larger V folds
// them and the block's V/16 adjacent lanes into one number
__device__ __forceinline__ void block_absmax(const u32x4& ev, const u32x4& od, int lv, int& a, int& b) {
    a = absmax4(ev.x, od.x, ev.y, od.y);
    b = absmax4(ev.z, od.z, ev.w, od.w);
    if (lv > 3) a = b = row_group_max(max(a, b), lv - 4);
}
// the lane's 16 bytes and its blocks' shift bytes: blocks 2i and 2i + 1 at V = 8, else the block's first lane
__device__ __forceinline__ void store_rq(u32x4 o, int sa, int sb, int8_t* q8, uint8_t* shift, size_t i, size_t nfull,
                                         size_t nq, bool half, int lv, int lane) {
    if (i < nfull) stream_store(o, reinterpret_cast<u32x4*>(q8) + i);
    else if (half) stream_store(u32x2{o.x, o.y}, reinterpret_cast<u32x2*>(q8 + 16 * i));
    if (lv == 3) {
        if (i < nq) shift[2 * i] = (uint8_t)sa;
        if (i < nfull) shift[2 * i + 1] = (uint8_t)sb;
    } else if (i < nq && (lane & ((1 << (lv - 4)) - 1)) == 0) {
        shift[(16 * i) >> lv] = (uint8_t)sa;
    }
}

// the smallest sh with a <= 127 << sh, for 0 <= a <= 8192
__device__ __forceinline__ int shift_sr_of(int a) {
    const int s0 = max(0, 25 - (int)__builtin_clz((uint32_t)a | 1u));          // bitlen(a) - 7
    return s0 + (a > (127 << s0) ? 1 : 0);
}
// (S + (u & (2^sh - 1))) >> sh in both fields of a word
__device__ __forceinline__ uint32_t requant_sr(uint32_t s, uint32_t u, uint32_t mask, s16x2 sh) {
    return word((fields(s) + fields(u & mask)) >> sh);
}
// 4 bytes in element order from the words of values (0, 2) and (1, 3) and the random word of the same 4 values
__device__ __forceinline__ uint32_t bytes_sr_of(uint32_t e, uint32_t o, uint32_t rw, uint32_t mask, s16x2 sh) {
    return __builtin_amdgcn_perm(requant_sr(o, (rw >> 8) & kLow8, mask, sh), requant_sr(e, rw & kLow8, mask, sh),
                                 0x06020400u);
}

// G > 0: compile-time slice count; G = 0: Gd slices.  lv = log2 V
template <int G>
__global__ __launch_bounds__(kBlk) void k_sum_rq_i8_sr(PtrPack<int8_t> in, int Gd, int8_t* __restrict__ q8,
                                                       uint8_t* __restrict__ shift, size_t n, int lv, SrKey rnd) {
    const int ng = G > 0 ? G : Gd;
    const size_t nfull = n / 16, nq = (n + 15) / 16;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x, stride = (size_t)gridDim.x * kBlk;
    const int lane = threadIdx.x & 63;
    const uint32_t init = sum_init(ng);
    for (size_t base = tid & ~(size_t)63; base < nq; base += stride) {   // wave-uniform
        const size_t i = base + lane;
        const bool half = i == nfull && i < nq;
        const u32x4 rw = philox(rnd, rnd.i0 + i);                        // byte j for value j; ahead of the loads
        u32x4 ev, od;
        sum_chunks<G>(in, ng, init, i, nfull, half, ev, od);
        int a, b;
        block_absmax(ev, od, lv, a, b);
        const int sa = shift_sr_of(a), sb = shift_sr_of(b);
        const uint32_t ma = ((1u << sa) - 1u) * 0x00010001u, mb = ((1u << sb) - 1u) * 0x00010001u;
        const s16x2 va = {(int16_t)sa, (int16_t)sa}, vb = {(int16_t)sb, (int16_t)sb};
        const u32x4 o = {bytes_sr_of(ev.x, od.x, rw.x, ma, va), bytes_sr_of(ev.y, od.y, rw.y, ma, va),
                         bytes_sr_of(ev.z, od.z, rw.z, mb, vb), bytes_sr_of(ev.w, od.w, rw.w, mb, vb)};
        store_rq(o, sa, sb, q8, shift, i, nfull, nq, half, lv, lane);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int launched() { return check_launch("int8 stochastic-rounding kernel launch"); }

// *rnd as the kernels take it, the stream counted in calls of `per` values; the last two refusals
int rnd_key(const ina_sr_t* rnd, unsigned per, SrKey& a) {
    if (!rnd) return set_error(INA_EINVAL, "null rnd%s", "");
    if (rnd->e0 % per) return set_error(INA_EINVAL, "rnd->e0 must be a multiple of %s", per == 4 ? "4" : "16");
    a = SrKey{(uint32_t)rnd->seed, (uint32_t)(rnd->seed >> 32), rnd->step, rnd->sub, rnd->e0 / per};
    return INA_OK;
}

template <typename X>
int quantize_sr(const void* x, const int8_t* kblk, int V, int8_t* q8, size_t n, uint8_t* ovf, const ina_sr_t* rot,
                const ina_sr_t* rnd, ina_stream_t stream) {
    int shift;
    if (int rc = check_blocks(V, kblk, n, shift)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q8) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!aligned16(x) || !aligned16(q8)) return misaligned();
    SrKey rk{}, key{};
    if (rot)
        if (int rc = rot_key(rot, V, rk)) return rc;
    if (int rc = rnd_key(rnd, 4, key)) return rc;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    const X* xp = static_cast<const X*>(x);
    if (rot) hipLaunchKernelGGL((k_q8_sr<X, true>), g, b, 0, hs(stream), xp, kblk, q8, n, shift, V, ovf, rk, key);
    else hipLaunchKernelGGL((k_q8_sr<X, false>), g, b, 0, hs(stream), xp, kblk, q8, n, shift, V, ovf, rk, key);
    return launched();
}

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

int ina_scale_for_i8_sr(float absmax, int* k_out) { return scale_for_lim(absmax, k_out, kLimI8Sr); }

int ina_block_scales_i8_sr(const void* const* xs, int xtype, int W, size_t n, int V, int8_t* kblk, const ina_sr_t* rot,
                           ina_stream_t stream) {
    return block_scales_i8(xs, xtype, W, n, V, kblk, rot, kLimI8Sr, stream);
}

int ina_quantize_sr_i8_wire(const void* x, int xtype, const int8_t* kblk, int V, int8_t* q8, size_t n,
                            uint8_t* overflow_per_slot, const ina_sr_t* rot, const ina_sr_t* rnd, ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_I8_X_CALL(xtype, quantize_sr, x, kblk, V, q8, n, overflow_per_slot, rot, rnd, stream);
}

int ina_sum_i8_slices_requant_sr(const int8_t* const* slices, int G, int V, int8_t* q8, uint8_t* shift, size_t n,
                                 const ina_sr_t* rnd, ina_stream_t stream) {
    PtrPack<int8_t> pk;
    int lv;
    if (int rc = check_sum_rq(slices, G, V, q8, shift, n, pk, lv)) return rc;
    if (n == 0) return INA_OK;
    SrKey key{};
    if (int rc = rnd_key(rnd, 16, key)) return rc;
    const dim3 g(grid_of((n + 15) / 16, default_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
#define L(GG) hipLaunchKernelGGL(k_sum_rq_i8_sr<GG>, g, b, 0, s, pk, G, q8, shift, n, lv, key)
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
unsigned long long ina::store_violations_i8sr() { return take_store_violations(); }
#endif
