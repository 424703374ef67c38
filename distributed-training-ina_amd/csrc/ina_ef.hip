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
// This file is the entry points and their argument checks.  There is no kernel here: the step
// (ef_v, ef_r) is in ina_chunk.h, and the launches run instances of the block-scale kernels of
// ina_blk.hip at W = 1 -- k_qr_blk_i32, k_qr_blk_i16, k_blk_scalar and k_blk_scales with the SrcEf
// value source in place of the plain one, which reads v for x and stores r' once v is quantised.
// The lane layouts, the scalar path and the in-place rule are described there.  The scale is the
// call's one k (K_GLOBAL, these calls only), the given block scales or the scales of the launch.
//
// The EF worker packs are instances of the split multi pack kernels of ina_kernels.hip (their EF
// template parameter); their entry points are there.
//
// The sharded int16 wire (include/ina_shard_ef.h): the two quantisers whose q is the int32 wire
// word q16 + (sat << 22) of ina_shard.hip.  They run the int32 instances above with the SrcEfWire
// source, which quantises with q16w and carries the word's q16: 16 bytes a value (x 4, r 4, word 4,
// r' 4) where the composition from existing ops moves about 40.
#include "ina.h"
#include "ina_internal.h"

namespace ina {
namespace {

// the global-k calls; xtype 0: fp32.  V = 0: int32 out (no slots; the scalar path's blocks are 256)
int quantize_ef(const void* x, int xtype, const float* base, float* resid, void* q, size_t n, int k, int V,
                uint8_t* ovf, ina_stream_t stream) {
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!resid) return set_error(INA_EINVAL, "null resid%s", "");
    if (xtype && ((uintptr_t)x & 1u)) return set_error(INA_EINVAL, "16-bit buffers must be 2-byte aligned%s", "");
    return ef_quantize(EfQuant{x, xtype, base, resid, q, V ? 16 : 32, n, K_GLOBAL, k, nullptr, 1.0, V ? V : 256, ovf},
                       stream);
}

int quantize_ef_blk(const float* x, const float* base, float* resid, int8_t* kblk, int mode, int degree, int V, void* q,
                    int bits, size_t n, uint8_t* ovf, ina_stream_t stream) {
    double lim;
    if (int rc = check_v(V)) return rc;
    if (int rc = check_mode(mode, kblk, degree, bits, lim)) return rc;
    if (n == 0) return INA_OK;
    if (!x || !q) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!resid) return set_error(INA_EINVAL, "null resid%s", "");
    return ef_quantize(EfQuant{x, 0, base, resid, q, bits, n, mode == INA_BLK_AUTO ? K_AUTO : K_GIVEN, 0, kblk, lim, V, ovf},
                       stream);
}

// n fp32 / int32 values at a and at b share a byte
bool overlap4(const void* a, const void* b, size_t n) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, len = (uintptr_t)n * 4u;
    return pa < pb ? pb - pa < len : pa - pb < len;
}

// the checks the wire siblings (ina_shard.hip) leave to the EF calls, then the launch
int quantize_ef_wire(const float* x, float* resid, int32_t* wire, size_t n, int km, int k, const int8_t* kblk, int V,
                     ina_stream_t stream) {
    if (!x || !wire) return set_error(INA_EINVAL, "null pointer%s", "");
    if (!resid) return set_error(INA_EINVAL, "null resid%s", "");
    if (overlap4(resid, x, n) || overlap4(resid, wire, n)) return set_error(INA_EINVAL, "resid overlaps x or wire%s", "");
    return ef_quantize(EfQuant{x, 0, nullptr, resid, wire, 32, n, km, k, const_cast<int8_t*>(kblk), 1.0, V, nullptr, true},
                       stream);
}

}  // namespace
}  // namespace ina

using namespace ina;

extern "C" {

// ---- include/ina_shard_ef.h: checks in the order of ina_quantize_f32_i16_wire / ina_quantize_blk_f32_i16_wire ----
int ina_quantize_ef_f32_i16_wire(const float* x, float* resid, int32_t* wire, size_t n, int k, ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    return quantize_ef_wire(x, resid, wire, n, K_GLOBAL, k, nullptr, 256, stream);   // (256: the scalar path's blocks)
}

int ina_quantize_ef_blk_f32_i16_wire(const float* x, float* resid, const int8_t* kblk, int V, int32_t* wire, size_t n,
                                     ina_stream_t stream) {
    if (int rc = check_v(V)) return rc;
    if (n == 0) return INA_OK;
    if (!kblk) return set_error(INA_EINVAL, "null kblk%s", "");
    return quantize_ef_wire(x, resid, wire, n, K_GIVEN, 0, kblk, V, stream);
}

int ina_quantize_ef_f32_i32(const float* x, const float* base, float* resid, int32_t* q, size_t n, int k,
                            ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    return quantize_ef(x, 0, base, resid, q, n, k, 0, nullptr, stream);
}

int ina_quantize_ef_f32_i16_sat(const float* x, const float* base, float* resid, int16_t* q, size_t n, int k, int V,
                                uint8_t* ovf, ina_stream_t stream) {
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    return quantize_ef(x, 0, base, resid, q, n, k, V, ovf, stream);
}

int ina_quantize_ef_x16_i32(const void* x, int xtype, const float* base, float* resid, int32_t* q, size_t n, int k,
                            ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (n == 0) return INA_OK;
    return quantize_ef(x, xtype, base, resid, q, n, k, 0, nullptr, stream);
}

int ina_quantize_ef_x16_i16_sat(const void* x, int xtype, const float* base, float* resid, int16_t* q, size_t n,
                                int k, int V, uint8_t* ovf, ina_stream_t stream) {
    if (int rc = check_x16_type(xtype)) return rc;
    if (int rc = check_k(k)) return rc;
    if (V <= 0) return set_error(INA_EINVAL, "V must be > 0%s", "");
    if (n == 0) return INA_OK;
    return quantize_ef(x, xtype, base, resid, q, n, k, V, ovf, stream);
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
    return ef_block_scales(px, pr, W, alx && alr, base, n, V, lim, kblk, stream);
}

int ina_quantize_ef_blk_f32_i32(const float* x, const float* base, float* resid, int8_t* kblk, int mode, int degree,
                                int V, int32_t* q, size_t n, ina_stream_t stream) {
    return quantize_ef_blk(x, base, resid, kblk, mode, degree, V, q, 32, n, nullptr, stream);
}

int ina_quantize_ef_blk_f32_i16_sat(const float* x, const float* base, float* resid, int8_t* kblk, int mode,
                                    int degree, int V, int16_t* q, size_t n, uint8_t* ovf, ina_stream_t stream) {
    return quantize_ef_blk(x, base, resid, kblk, mode, degree, V, q, 16, n, ovf, stream);
}

}  // extern "C"
