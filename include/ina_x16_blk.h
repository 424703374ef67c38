/*
 * ina_x16_blk.h -- per-block scales for bf16 / fp16 buckets: the scales, the quantisers, the fused
 * reduces, the decode into a 16-bit buffer and the one-launch worker pack.  Included by ina.h last
 * (it needs ina_x16.h's type codes, ina_blk.h's modes and the packet types); do not include it on
 * its own.
 *
 * A 16-bit gradient bucket is read as it is and widened in registers; widening is exact, so
 *
 *   every result is bit for bit the fp32 block-scaled sibling's (ina_blk.h, ina_pkt_blk.h) on the
 *   widened bucket: scales, values, saturation, the per-block flags, packet rows and descriptors.
 *
 * What follows from it: base stays fp32 and a delta is the fp32 subtraction widen(x) - base; NaN
 * reads as 0 and is ignored by a block's max; a block holding +-inf gets -126 and saturates with
 * its flag; a given -127 / -128 reads as -126; no scale outside kblk[0 .. ceil(n / V)) is read or
 * written.  The decode is float(s) * 2^-kblk[block] in fp32, rounded once to nearest even into the
 * 16-bit type (ina_dequantize_i32_x16's conversion: fp16 overflows to +-inf, subnormals kept).
 *
 * xtype / ytype is INA_X16_BF16 or INA_X16_F16; all W buffers of a call share one type.  Buffers
 * are void*, 2-byte aligned.  Argument checks are the fp32 sibling's, in its order and with its
 * messages, after the type code; n == 0 is a no-op.  V a power of two in [8, 256] with the 16-bit
 * buffers 8-byte aligned and the 32-bit ones 16-byte aligned takes the vector path (a lane owns 4
 * values: one 8-byte access on the 16-bit side); any other V or alignment takes the slower path
 * with identical results.  An int16 out may alias bufs[0], which has its width.
 *
 * Not here: the block-scaled int16 wire (ina_shard_blk.h), the single-worker packed pack, the PS
 * calls (their vectors are the PS's fp32 parameters) and the switch, which only sees integers.
 */
#ifndef INA_X16_BLK_H
#define INA_X16_BLK_H

#ifndef INA_SHARD_BLK_H
#error "include ina.h, which includes ina_x16_blk.h"
#endif

/* ina_block_scales_f32 */
int ina_block_scales_x16(const void* const* xs, int xtype, int W, const float* base, size_t n, int V,
                         int degree, int bits, int8_t* kblk_out, ina_stream_t stream);
/* ina_quantize_blk_f32_i32 / ina_quantize_blk_f32_i16_sat */
int ina_quantize_blk_x16_i32(const void* x, int xtype, const int8_t* kblk, int V, int32_t* q, size_t n,
                             ina_stream_t stream);
int ina_quantize_blk_x16_i16_sat(const void* x, int xtype, const int8_t* kblk, int V, int16_t* q, size_t n,
                                 uint8_t* overflow_per_block, ina_stream_t stream);
/* ina_quantize_reduce_blk_f32_i32 / ina_quantize_reduce_blk_f32_i16_sat */
int ina_quantize_reduce_blk_x16_i32(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode,
                                    int degree, int V, int32_t* out, size_t n, ina_stream_t stream);
int ina_quantize_reduce_blk_x16_i16_sat(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode,
                                        int degree, int V, int16_t* out, size_t n,
                                        uint8_t* overflow_per_block, ina_stream_t stream);
/* ina_dequantize_blk_i32_f32 / ina_dequantize_blk_i16_f32 into a bf16 / fp16 buffer */
int ina_dequantize_blk_i32_x16(const int32_t* s, const int8_t* kblk, int V, void* y, int ytype, size_t n,
                               ina_stream_t stream);
int ina_dequantize_blk_i16_x16(const int16_t* s, const int8_t* kblk, int V, void* y, int ytype, size_t n,
                               ina_stream_t stream);
/* ina_quantize_pack_nga_multi_split_blk: AUTO in the pack's own launch for V a power of two in
 * [8, 256] and W <= 8, else ina_block_scales_x16 first and the GIVEN pack */
int ina_quantize_pack_nga_multi_split_blk_x16(const void* const* x, int xtype, int W, const float* base,
                                              size_t n, int8_t* kblk, int mode, int degree,
                                              const ina_nga_params_t* prm, uint8_t* const* hdr,
                                              uint8_t* const* pay, ina_nga_desc_t* const* desc,
                                              ina_stream_t stream);

#endif /* INA_X16_BLK_H */
