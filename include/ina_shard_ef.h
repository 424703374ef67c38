/*
 * ina_shard_ef.h -- error feedback on the int16 wire of a sharded bucket: the wire quantisers of
 * ina.h and ina_shard_blk.h with a residual carried on the device from step to step.  Included by
 * ina.h after ina_shard_blk.h and before ina_ef.h, whose contract holds here with no base; do not
 * include it on its own.
 *
 * A sharded int16 job sums up to 64 ranks, so ina_scale_for leaves each rank as little as 9 bits,
 * and every rank rounds its whole bucket to that wire on every step.  Here a rank owns one fp32
 * residual of n values per bucket; it starts at zero and each call updates it in place.  The
 * collective, the decode (ina_i16_wire_finish, ina_i16_wire_finish_blk) and the wire format are
 * untouched: the ranks still sum plain int32 words.
 *
 * Contract.  Per element, in fp32, unfused:
 *     v    = x + r
 *     q16  = sat16(rne(v * 2^k)), NaN -> 0;   sat = clamped, +-inf or NaN
 *     word = q16 + (sat << INA_I16_WIRE_SHIFT)          the wire sibling's word on v
 *     r'   = isfinite(v) ? v - float(q16) * 2^-k : +0.0f
 *   The residual uses q16, never the word with its count bits.  2^-k is built from its bits (k =
 *     127 gives the subnormal 2^-127).
 *   With block scales, k = kblk[e / V] under the contract of ina_blk.h: a given -127 / -128 reads as
 *     -126, the last block may be short, and no byte outside kblk[0 .. ceil(n / V)) is read.
 *   There is no AUTO mode: the ranks agree on the scales (MIN) before anyone quantises.  A rank's
 *     own scales of v are ina_block_scales_ef_f32 with bits = 16 and degree = the number of ranks.
 * Two consequences:
 *   Replay.  word is the wire sibling's on v, and (q16, r') is ina_quantize_ef_f32_i16_sat's /
 *     ina_quantize_ef_blk_f32_i16_sat's (q, r') on the same inputs, bit for bit.
 *   Zero residual.  With resid all zero the word equals the non-EF sibling's on x bit for bit.
 *
 * Checks, in each wire sibling's order and with its messages: k in [-126, 127] (V >= 1), then the
 * n == 0 no-op, then a null kblk, a null x or wire, a null resid ("null resid"), and a resid that
 * overlaps x or wire; each is INA_EINVAL before any device work.  16-byte aligned buffers (and V a
 * power of two in [8, 256] for the block form) take the vector path: 4 values per lane, x, r, word
 * and r' one 16-byte access each.  Any other alignment or V takes a value-by-value path with
 * identical results.  fp32 buckets only.
 */
#ifndef INA_SHARD_EF_H
#define INA_SHARD_EF_H

#ifndef INA_SHARD_BLK_H
#error "include ina.h, which includes ina_shard_blk.h and ina_shard_ef.h"
#endif

/* ina_quantize_f32_i16_wire on v = x + resid; resid updated in place */
int ina_quantize_ef_f32_i16_wire(const float* x, float* resid, int32_t* wire, size_t n, int k,
                                 ina_stream_t stream);
/* ina_quantize_blk_f32_i16_wire on v = x + resid, scales given (the ranks agreed on them first) */
int ina_quantize_ef_blk_f32_i16_wire(const float* x, float* resid, const int8_t* kblk, int V,
                                     int32_t* wire, size_t n, ina_stream_t stream);

#endif /* INA_SHARD_EF_H */
