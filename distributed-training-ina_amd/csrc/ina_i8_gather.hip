// ina_i8_gather.hip -- the requantised 8-bit gather of the byte wire (include/ina_i8_gather.h states the
// contract): the sum of up to 64 ranks' byte slices rounded back to bytes under a per-block shift in one pass,
// and the decode that reads those bytes.
//
// Sum + requantise.  The front is k_sum_i8's (ina_i8.hip; its loads, byte adds and block maximum are in
// ina_i8_sum_device.h, which ina_i8_sr.hip's stochastic requantiser shares): a lane owns 16 values, loads 16
// bytes of each slice and adds their even and odd bytes as 16-bit fields of 32-bit words (bytes made unsigned by w ^ 0x80808080, a
// field starting at 0x8000 - 128 G, its top bit flipped at the end); G = 2, 4, 8, 16 are compile-time with up
// to 8 loads in flight, any other G runs a loop with two.  The 8 words of signed sums then stay in registers
// and everything up to the bytes is packed 16-bit arithmetic on them (v_pk_*_i16, written as vector
// expressions; |S| <= 8192 and every intermediate of the rounding <= 8256):
//   max    |S| per field, the max of the words of values 0-7 and of values 8-15, each folded to one number.
//          V = 8: those are two blocks and that is all.  V >= 16: their max, then the max over the block's V/16
//          adjacent lanes by row-level DPP folded into v_max_i32 -- quad_perm [1,0,3,2] and [2,3,0,1], then
//          row_half_mirror and row_mirror (after the two quad steps a quad's lanes agree, so a mirror is as
//          good as lane ^ 4 and lane ^ 8).  V = 256 is one row of 16 lanes; nothing crosses a row, no LDS, no
//          bpermute.
//   shift  s0 = max(0, bitlen(A) - 7) from one v_ffbh, plus one where rne(A / 2^s0) is 128.
//   round  (S + 2^(sh-1) - 1 + ((S >> sh) & 1)) >> sh per field.  sh = 0 takes the same instructions: the bias
//          is then -1 and the tie bit is forced to 1, which adds 0.
//   bytes  each field now holds an int8 in its low byte; one v_perm_b32 per (even, odd) pair of words puts 4
//          of them in element order, one 16-byte sc1 store a lane.  The block's first lane writes its shift
//          byte (V = 8: every lane writes its two).
// n is a multiple of V >= 8, so the one ragged case is n mod 16 = 8 at V = 8: the lane after the last whole
// chunk loads and stores 8 bytes and writes one shift.  The loop's trip count is wave-uniform (all 64 lanes
// reach the DPP steps); a lane past n holds zeros, which add nothing to a maximum, and writes nothing.
//
// Decode.  The rotation's lanes (ina_rot.hip): a lane owns 4 values, here one dword of bytes, 256 contiguous
// bytes a wave; the block's scale and shift are one byte load each.  The bytes are sign-extended and shifted
// left, which is the int16 the contract speaks of, and from there the sequence is k_dq_rot<int16_t>'s (deq4,
// rot_inv with ina_rot_device.h's signs and butterfly) or k_dq_blk's (deq4): one instance per arm for every V.
#include <hip/hip_runtime.h>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"
#include "ina_rot_device.h"
#include "ina_i8_sum_device.h"

namespace ina {
namespace {

constexpr int kBlk = 256;

// ---------------------------------------------------------------------------
// sum + requantise
// ---------------------------------------------------------------------------
// the smallest sh with rne(a / 2^sh) <= 127, for 0 <= a <= 8192
__device__ __forceinline__ int shift_of(int a) {
    const int s0 = max(0, 25 - (int)__builtin_clz((uint32_t)a | 1u));          // bitlen(a) - 7
    const int r = s0 ? (a + (1 << (s0 - 1)) - 1 + ((a >> s0) & 1)) >> s0 : a;   // rne(a / 2^s0)
    return s0 + (r == 128 ? 1 : 0);
}
// rne(S / 2^sh) in both fields of a word
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
// 4 bytes in element order from the words of values (0, 2) and (1, 3)
__device__ __forceinline__ uint32_t bytes_of(uint32_t e, uint32_t o, const Requant& r) {
    return __builtin_amdgcn_perm(requant(o, r), requant(e, r), 0x06020400u);
}

// G > 0: compile-time slice count; G = 0: Gd slices.  lv = log2 V
template <int G>
__global__ __launch_bounds__(kBlk) void k_sum_rq_i8(PtrPack<int8_t> in, int Gd, int8_t* __restrict__ q8,
                                                    uint8_t* __restrict__ shift, size_t n, int lv) {
    const int ng = G > 0 ? G : Gd;
    const size_t nfull = n / 16, nq = (n + 15) / 16;
    const size_t tid = (size_t)blockIdx.x * kBlk + threadIdx.x, stride = (size_t)gridDim.x * kBlk;
    const int lane = threadIdx.x & 63;
    const uint32_t init = kTop16 - (uint32_t)ng * 128u * 0x00010001u;
    for (size_t base = tid & ~(size_t)63; base < nq; base += stride) {   // wave-uniform
        const size_t i = base + lane;
        const bool half = i == nfull && i < nq;
        u32x4 ev = {init, init, init, init}, od = ev;
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
        // word j of ev holds the sums of values 4j and 4j+2, of od 4j+1 and 4j+3
        int a = absmax4(ev.x, od.x, ev.y, od.y), b = absmax4(ev.z, od.z, ev.w, od.w);
        if (lv > 3) a = b = row_group_max(max(a, b), lv - 4);
        const int sa = shift_of(a), sb = shift_of(b);
        const Requant ra = requant_of(sa), rb = requant_of(sb);
        const u32x4 o = {bytes_of(ev.x, od.x, ra), bytes_of(ev.y, od.y, ra), bytes_of(ev.z, od.z, rb),
                         bytes_of(ev.w, od.w, rb)};
        if (i < nfull) stream_store(o, reinterpret_cast<u32x4*>(q8) + i);
        else if (half) stream_store(u32x2{o.x, o.y}, reinterpret_cast<u32x2*>(q8 + 16 * i));
        if (lv == 3) {                                                   // blocks 2i and 2i + 1
            if (i < nq) shift[2 * i] = (uint8_t)sa;
            if (i < nfull) shift[2 * i + 1] = (uint8_t)sb;
        } else if (i < nq && (lane & ((1 << (lv - 4)) - 1)) == 0) {
            shift[(16 * i) >> lv] = (uint8_t)sa;
        }
    }
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
// chunk i = values 4i..4i+3; base_ is the wave's first chunk (a multiple of 64)
#define INA_I8G_QUAD_LOOP(nq)                                    \
    const size_t tid_ = (size_t)blockIdx.x * kBlk + threadIdx.x; \
    const size_t stride_ = (size_t)gridDim.x * kBlk;             \
    for (size_t base_ = tid_ & ~(size_t)63; base_ < (nq); base_ += stride_)

// ROT: the inverse rotation after the scale (sr != NULL)
template <bool ROT>
__global__ __launch_bounds__(kBlk) void k_dq_i8g(const int8_t* __restrict__ q8, const uint8_t* __restrict__ shb,
                                                 const int8_t* __restrict__ kblk, float* __restrict__ y, size_t n,
                                                 int shift, SrKey key) {
    const size_t nq = n / 4;                                             // n is a multiple of V >= 8
    const int lane = threadIdx.x & 63;
    INA_I8G_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        uint32_t w = 0u;
        int k = 0, sh = 0;
        if (i < nq) {
            w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(q8) + i);
            k = rd_k(kblk, i >> shift);
            sh = min((int)shb[i >> shift], 7);
        }
        // (int16)q8 << sh of the contract, held widened
        const u32x4 q = {(uint32_t)((int32_t)(int8_t)w << sh), (uint32_t)((int32_t)(int8_t)(w >> 8) << sh),
                         (uint32_t)((int32_t)(int8_t)(w >> 16) << sh), (uint32_t)(((int32_t)w >> 24) << sh)};
        f32x4 x = deq4(q, pow2f(-k));
        if constexpr (ROT) x = rot_inv(x, rot_signs(key, 4 * base_, lane), shift, lane);
        if (i < nq) st4(x, y, e, n);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int launched() { return check_launch("int8 gather kernel launch"); }
int misaligned() { return set_error(INA_EINVAL, "buffers must be 16-byte aligned%s", ""); }
int bad_v() { return set_error(INA_EINVAL, "V must be a power of two in [8, 256]%s", ""); }
int bad_n() { return set_error(INA_EINVAL, "n must be a multiple of V%s", ""); }

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

int ina_sum_i8_slices_requant(const int8_t* const* slices, int G, int V, int8_t* q8, uint8_t* shift, size_t n,
                              ina_stream_t stream) {
    PtrPack<int8_t> pk;
    int lv;
    if (int rc = check_sum_rq(slices, G, V, q8, shift, n, pk, lv)) return rc;
    if (n == 0) return INA_OK;
    const dim3 g(grid_of((n + 15) / 16, default_grid_cap())), b(kBlk);
    hipStream_t s = hs(stream);
#define L(GG) hipLaunchKernelGGL(k_sum_rq_i8<GG>, g, b, 0, s, pk, G, q8, shift, n, lv)
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

int ina_dequantize_i8_gather(const int8_t* q8, const uint8_t* shift, const int8_t* kblk, int V, float* y, size_t n,
                             const ina_sr_t* sr, ina_stream_t stream) {
    int qs;
    if (!vec_v(V, qs)) return bad_v();
    if (n % (size_t)V) return bad_n();
    if (n == 0) return INA_OK;
    if (!q8 || !y || !kblk) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!shift) return set_error(INA_EINVAL, "null shift%s", "");
    if (!aligned16(q8) || !aligned16(y)) return misaligned();
    SrKey key{};
    if (sr)
        if (int rc = rot_key(sr, V, key)) return rc;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    if (sr) hipLaunchKernelGGL(k_dq_i8g<true>, g, b, 0, hs(stream), q8, shift, kblk, y, n, qs, key);
    else hipLaunchKernelGGL(k_dq_i8g<false>, g, b, 0, hs(stream), q8, shift, kblk, y, n, qs, key);
    return launched();
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_i8g() { return take_store_violations(); }
#endif
