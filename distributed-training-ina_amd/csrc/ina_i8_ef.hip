// ina_i8_ef.hip -- error feedback on the 8-bit wire (include/ina_i8_ef.h states the contract): the byte
// quantiser that adds the rank's residual in front of the rotation and carries the rounding error back through
// the inverse rotation into the residual, in one launch, and the scales of what that launch will quantise.
//
// Both kernels run in the rotation's lanes (ina_rot.hip, ina_i8.hip): a lane owns the 16-byte chunk of 4 values
// 4l..4l+3 of its wave's 256, a block is V/4 adjacent lanes of one wave.  The quantiser lane
//   loads  its chunk of x (16 bytes, 8 for bf16 / fp16, widened) and of resid (16 bytes) and adds them: v;
//   signs  takes the wave's 256 sign bits once from the scalar unit (rot_signs) and keeps its 4 masks;
//   fwd    r = rot_fwd(v): the butterfly across the block's lanes by DPP and v_permlane*_swap;
//   bytes  clamps rne(r * 2^k) by one v_med3_f32 a value, converts, packs (v_cvt_pk_i16_i32, v_perm_b32) and
//          stores one dword: ina_i8_device.h's steps, k_q8's bytes.  The error d = r - float(q8) * 2^-k (+0
//          where r is NaN or inf) is ina_chunk.h's error-feedback step on the 4 ints before they are packed;
//   inv    u = rot_inv(d) with the kept masks: the same stages in the same lanes, so d never leaves its
//          registers -- no LDS, no memory between the two butterflies;
//   store  resid' = u where u is finite, else +0: one 16-byte store over the chunk it loaded.
// ROT = false (sr == NULL) is an arm of its own with no butterfly and no signs: r = v, u = d.  n is a multiple
// of V >= 8, so no chunk crosses n; the loop's trip count is wave-uniform (all 64 lanes reach every exchange of
// both butterflies), and a lane past n carries zeros -- v = 0, d = 0 -- and writes nothing.
//
// The scales kernel is k_i8_scales (ina_i8.hip) with the residuals as a second pointer pack and the add in
// front of the rotation; two pairs' loads (4 loads) are in flight.
#include <hip/hip_runtime.h>

#include "ina.h"
#include "ina_internal.h"
#include "ina_device.h"
#include "ina_chunk.h"
#include "ina_rot_device.h"
#include "ina_i8_device.h"

namespace ina {
namespace {

constexpr int kBlk = kI8Blk;

template <typename X, bool ROT>
__global__ __launch_bounds__(kBlk) void k_i8_scales_ef(PtrPack<X> xs, PtrPack<float> rs, int W, size_t n, int shift,
                                                       double lim, SrKey key, int8_t* __restrict__ kblk) {
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_I8_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        [[maybe_unused]] u32x4 sg = {0u, 0u, 0u, 0u};
        if constexpr (ROT) sg = rot_signs(key, 4 * base_, lane);
        auto r = [&](f32x4 x, f32x4 res) {
            const f32x4 v = ef_v4(x, res);
            if constexpr (ROT) return rot_fwd(v, sg, shift, lane);
            else return v;
        };
        uint32_t m = 0u;
        int w = 0;
        for (; w + 2 <= W; w += 2) {                                   // two pairs' loads in flight
            const f32x4 a = ld4(xs.p[w], e, n), ra = ld4(rs.p[w], e, n);
            const f32x4 b = ld4(xs.p[w + 1], e, n), rb = ld4(rs.p[w + 1], e, n);
            m = fold4(fold4(m, r(a, ra)), r(b, rb));
        }
        if (w < W) m = fold4(m, r(ld4(xs.p[w], e, n), ld4(rs.p[w], e, n)));
        m = group_max(m, 1 << shift);
        if (e < n && (lane & ((1 << shift) - 1)) == 0) kblk[i >> shift] = (int8_t)scale_of(m, lim);
    }
}

// resid' of one value: u where it is finite, else +0
__device__ __forceinline__ float guard(float u) {
    return (__float_as_uint(u) & 0x7F800000u) != 0x7F800000u ? u : 0.0f;
}

template <typename X, bool ROT>
__global__ __launch_bounds__(kBlk) void k_q8_ef(const X* __restrict__ x, float* __restrict__ resid,
                                                const int8_t* __restrict__ kblk, int8_t* __restrict__ q8, size_t n,
                                                int shift, int V, uint8_t* __restrict__ ovf, SrKey key) {
    const size_t nq = n / 4;
    const int lane = threadIdx.x & 63;
    INA_I8_QUAD_LOOP(nq) {
        const size_t i = base_ + lane, e = 4 * i;
        const f32x4 v = ef_v4(ld4(x, e, n), ld4(resid, e, n));
        [[maybe_unused]] u32x4 sg = {0u, 0u, 0u, 0u};
        f32x4 r = v;
        if constexpr (ROT) {
            sg = rot_signs(key, 4 * base_, lane);
            r = rot_fwd(v, sg, shift, lane);
        }
        const int k = e < n ? rd_k(kblk, i >> shift) : 0;
        const float s = pow2f(k), inv = pow2f(-k);
        bool sat = false;
        const int qa = q8_of(q8_round(r.x, s), sat), qb = q8_of(q8_round(r.y, s), sat);
        const int qc = q8_of(q8_round(r.z, s), sat), qd = q8_of(q8_round(r.w, s), sat);
        if (e < n) stream_store(q8_pack(qa, qb, qc, qd), reinterpret_cast<uint32_t*>(q8 + e));
        // d = r - float(q8) * 2^-k, +0 where r is NaN or inf: ina_ef.h's step on the rotated value
        f32x4 d = ef_r4(r, u32x4{(uint32_t)qa, (uint32_t)qb, (uint32_t)qc, (uint32_t)qd}, inv);
        const unsigned long long m = __ballot(sat);                    // wave-convergent
        if (ovf) write_slot_flags8(m, e < n, e, V, 1 << shift, ovf);
        if constexpr (ROT) d = rot_inv(d, sg, shift, lane);
        if (e < n) stream_store(f32x4{guard(d.x), guard(d.y), guard(d.z), guard(d.w)}, reinterpret_cast<f32x4*>(resid + e));
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int launched() { return check_launch("int8 error-feedback kernel launch"); }
int null_resid() { return set_error(INA_EINVAL, "null resid%s", ""); }

template <typename X>
int block_scales_ef(const void* const* xs, const float* const* resids, int W, size_t n, int V, int8_t* kblk,
                    const ina_sr_t* sr, ina_stream_t stream) {
    int shift;
    if (int rc = check_blocks(V, kblk, n, shift)) return rc;
    if (n == 0) return INA_OK;
    PtrPack<X> pk;
    PtrPack<float> rk;
    bool al, ral;
    if (int rc = fill_pack(pk, xs, W, al)) return rc;
    if (!resids) return null_resid();
    for (int w = 0; w < W; ++w)
        if (!resids[w]) return null_resid();
    if (int rc = fill_pack(rk, resids, W, ral)) return rc;
    if (!al || !ral) return misaligned();
    SrKey key{};
    if (sr)
        if (int rc = rot_key(sr, V, key)) return rc;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    if (sr) hipLaunchKernelGGL((k_i8_scales_ef<X, true>), g, b, 0, hs(stream), pk, rk, W, n, shift, kLimI8, key, kblk);
    else hipLaunchKernelGGL((k_i8_scales_ef<X, false>), g, b, 0, hs(stream), pk, rk, W, n, shift, kLimI8, key, kblk);
    return launched();
}

template <typename X>
int quantize_ef(const void* x, float* resid, const int8_t* kblk, int V, int8_t* q8, size_t n, uint8_t* ovf,
                const ina_sr_t* sr, ina_stream_t stream) {
    int shift;
    if (int rc = check_blocks(V, kblk, n, shift)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q8) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!resid) return null_resid();
    if (!aligned16(x) || !aligned16(q8) || !aligned16(resid)) return misaligned();
    SrKey key{};
    if (sr)
        if (int rc = rot_key(sr, V, key)) return rc;
    const dim3 g(grid_of(n / 4, default_grid_cap())), b(kBlk);
    const X* xp = static_cast<const X*>(x);
    if (sr) hipLaunchKernelGGL((k_q8_ef<X, true>), g, b, 0, hs(stream), xp, resid, kblk, q8, n, shift, V, ovf, key);
    else hipLaunchKernelGGL((k_q8_ef<X, false>), g, b, 0, hs(stream), xp, resid, kblk, q8, n, shift, V, ovf, key);
    return launched();
}

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

int ina_block_scales_i8_ef(const void* const* xs, const float* const* resids, int xtype, int W, size_t n, int V,
                           int8_t* kblk, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_I8_X_CALL(xtype, block_scales_ef, xs, resids, W, n, V, kblk, sr, stream);
}

int ina_quantize_ef_i8_wire(const void* x, int xtype, float* resid, const int8_t* kblk, int V, int8_t* q8, size_t n,
                            uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream) {
    if (int rc = check_xtype(xtype)) return rc;
    return INA_I8_X_CALL(xtype, quantize_ef, x, resid, kblk, V, q8, n, overflow_per_slot, sr, stream);
}

}  // extern "C"

#if INA_STORE_CHECK
unsigned long long ina::store_violations_i8ef() { return take_store_violations(); }
#endif
