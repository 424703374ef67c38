/*
 * ina_blk.h -- block floating point: one exponent per block of V values for the quantiser,
 * the fused reduces and the PS update.  Included by ina.h; do not include it on its own.
 *
 * Every other quantising entry point takes one exponent k for the whole bucket, so all the
 * bits of the integer wire are spent on the bucket's largest value.  Here a bucket carries one
 * exponent per block, agreed by every worker (MIN across nodes), and the aggregator still adds
 * plain integers.  The block is the slot: one packet's payload, the unit of the overflow flags.
 *
 * Contract
 *   Blocks.  A block is V consecutive values: block s covers [s*V, min(n, (s+1)*V)), nblk =
 *     ceil(n / V).  The last block may be short and its scale comes from its own values only.
 *     V is any integer >= 1.
 *   Scales.  One int8_t per block, kblk[s] in [-126, 127]; a scale array is device memory of
 *     nblk bytes.
 *   Computed scales.  kblk[s] is computed for `degree` summands and width `bits` (16 or 32) and
 *     is exactly what ina_scale_for(amax_s, degree, bits) returns, with
 *         amax_s = max over the given buffers w and i in block s of |xs[w][i] - base[i]|
 *     (the fp32 subtraction, when base is not NULL; NaN ignored, as in ina_absmax_multi_f32).
 *     An all-zero or all-NaN block gives 127.  A block holding +-inf gives -126
 *     (ina_scale_for refuses inf; here the block saturates and its flag says so).  The result
 *     equals the host function bit for bit for every fp32 amax_s, subnormals and 3e38 included.
 *     `degree` is the number of summands of the whole job, not the W of this call: a GPU holding
 *     4 of a job's 16 workers passes W = 4 buffers and degree = 16.  degree is refused under
 *     ina_scale_for's rule: (2^(bits-1) - 1) / degree - 1/2 <= 0 is INA_EINVAL.
 *   Block-scaled results.  A block-scaled call's result on block s is bit for bit the global-k
 *     sibling's result on that block alone with k = kblk[s]: values, saturation and the slot
 *     flag.  The overflow flags stay per block, on the same V, and every flag is written when the
 *     pointer is non-NULL.  The dequantise scale is ldexpf(1.0f, -k) exactly, k = 127 (a
 *     subnormal) included.
 *   Given scales.  A given kblk entry of -127 or -128 is read as -126.  The library never
 *     writes one.
 *
 * fp32 sources only.  Argument order, return codes, the n == 0 no-op and the null checks follow
 * the global-k sibling of each call.  bits, degree, V and mode are checked before any device
 * work.  V a power of two in [8, 256] with every buffer 16-byte aligned takes the vector path;
 * any other V or alignment takes a slower path with identical results.  out may alias bufs[0]
 * where the sibling allows it, and local in the PS calls.
 *
 * The packet path (the NGA packs and the PS apply of completed packets, where a block is one
 * packet's payload) takes the same scales under the same contract; its three entry points are
 * declared in ina_pkt_blk.h, which ina.h includes after this file.
 */
#ifndef INA_BLK_H
#define INA_BLK_H

#ifndef INA_H
#error "include ina.h, which includes ina_blk.h"
#endif

#define INA_BLK_GIVEN 0 /* kblk is read */
#define INA_BLK_AUTO 1  /* kblk is computed from this call's buffers and written */

/* scales alone (a worker GPU, or before an exchange between nodes) */
int ina_block_scales_f32(const float* const* xs, int W, const float* base, size_t n, int V,
                         int degree, int bits, int8_t* kblk, ina_stream_t stream);
/* worker side, scales given: ina_quantize_f32_i32 / ina_quantize_f32_i16_sat */
int ina_quantize_blk_f32_i32(const float* x, const int8_t* kblk, int V, int32_t* q, size_t n,
                             ina_stream_t stream);
int ina_quantize_blk_f32_i16_sat(const float* x, const int8_t* kblk, int V, int16_t* q, size_t n,
                                 uint8_t* overflow_per_slot, ina_stream_t stream);
/* aggregating GPU: fused quantise + reduce (ina_quantize_reduce_f32_i32 / _i16_sat).  mode
 * INA_BLK_GIVEN reads kblk; INA_BLK_AUTO computes it from these W buffers for `degree` summands
 * (bits = the width of out) and writes it.  degree is ignored when the scales are given. */
int ina_quantize_reduce_blk_f32_i32(const float* const* bufs, int W, int8_t* kblk, int mode, int degree,
                                    int V, int32_t* out, size_t n, ina_stream_t stream);
int ina_quantize_reduce_blk_f32_i16_sat(const float* const* bufs, int W, int8_t* kblk, int mode,
                                        int degree, int V, int16_t* out, size_t n,
                                        uint8_t* overflow_per_slot, ina_stream_t stream);
/* ina_dequantize_i32_f32 / ina_dequantize_i16_f32 */
int ina_dequantize_blk_i32_f32(const int32_t* s, const int8_t* kblk, int V, float* y, size_t n,
                               ina_stream_t stream);
int ina_dequantize_blk_i16_f32(const int16_t* s, const int8_t* kblk, int V, float* y, size_t n,
                               ina_stream_t stream);
/* PS: ina_ps_apply_i32 with per-block k */
int ina_ps_apply_blk_i32(const float* local, const int32_t* sum_int, const int8_t* kblk, int V,
                         double weight_step, float* out, size_t n, ina_stream_t stream);
/* PS, one pass, no host read: ina_ps_combine_ina_f32 with per-block k computed on the fly from the
 * W deltas paras[w] - local (degree = W, bits = 32); kblk_out (nblk bytes) may be NULL */
int ina_ps_combine_ina_blk_f32(const float* local, const float* const* paras, int W, int V,
                               double weight_step, float* out, size_t n, int8_t* kblk_out,
                               ina_stream_t stream);

#endif /* INA_BLK_H */
