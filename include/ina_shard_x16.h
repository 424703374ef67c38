/*
 * ina_shard_x16.h -- bf16 / fp16 buckets on the int16 wire of a sharded bucket: the wire quantisers
 * and the decodes of ina.h and ina_shard_blk.h with a 16-bit source (x) or a 16-bit target (y).
 * Included by ina.h after ina_shard_blk.h and before ina_shard_ef.h; do not include it on its own.
 *
 * Each function is its fp32 sibling with a type code (INA_X16_BF16 / INA_X16_F16, ina_x16.h) after
 * the 16-bit pointer.  One rule, that of ina_x16_blk.h:
 *
 *   Widening is exact, so a wire word is bit for bit the fp32 sibling's on the widened bucket:
 *     NaN -> 0 with the saturation bit, +-inf and clamped values with it, a given -127 / -128 read
 *     as -126, and no byte outside kblk[0 .. ceil(n / V)) read.
 *   In the decodes out16 and the flags are the sibling's.  y is float(sum) * 2^-k (2^-kblk[e / V])
 *     in fp32, rounded once to nearest even to the 16-bit type with the converters of ina_x16.h
 *     (fp16: overflow to +-inf, subnormal results produced; never a packed round-toward-zero
 *     convert) -- bit for bit ina_dequantize_i16_x16 / ina_dequantize_blk_i16_x16 on out16.
 *
 * Checks: the type code first ("16-bit type must be ..."), then the sibling's in its order and with
 * its messages (k in [-126, 127] or V >= 1 / V > 0, the n == 0 no-op, a null kblk, null pointers),
 * then a 16-bit pointer that is not 2-byte aligned; each is INA_EINVAL before any device work.
 * out16, y and overflow_per_slot may each be NULL (ytype is checked all the same).
 *
 * Layout: a lane owns 4 values -- one 8-byte access on the 16-bit side, one 16-byte access on the
 * 32-bit side.  The vector path needs the 16-bit buffer 8-byte aligned, the 32-bit buffers 16-byte
 * aligned (out16: 8-byte) and, for the block forms, V a power of two in [8, 256]; any other
 * alignment or V takes a value-by-value path with identical results.
 */
#ifndef INA_SHARD_X16_H
#define INA_SHARD_X16_H

#ifndef INA_SHARD_BLK_H
#error "include ina.h, which includes ina_shard_blk.h and ina_shard_x16.h"
#endif

/* ina_quantize_f32_i16_wire from a 16-bit bucket */
int ina_quantize_x16_i16_wire(const void* x, int xtype, int32_t* wire, size_t n, int k, ina_stream_t stream);
/* ina_quantize_blk_f32_i16_wire from a 16-bit bucket */
int ina_quantize_blk_x16_i16_wire(const void* x, int xtype, const int8_t* kblk, int V, int32_t* wire,
                                  size_t n, ina_stream_t stream);
/* ina_i16_wire_finish with y a 16-bit buffer of type ytype */
int ina_i16_wire_finish_x16(const int32_t* wire_sum, size_t n, int k, int V, int16_t* out16, void* y,
                            int ytype, uint8_t* overflow_per_slot, ina_stream_t stream);
/* ina_i16_wire_finish_blk with y a 16-bit buffer of type ytype */
int ina_i16_wire_finish_blk_x16(const int32_t* wire_sum, size_t n, const int8_t* kblk, int V,
                                int16_t* out16, void* y, int ytype, uint8_t* overflow_per_slot,
                                ina_stream_t stream);

#endif /* INA_SHARD_X16_H */
