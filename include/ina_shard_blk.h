/*
 * ina_shard_blk.h -- per-block scales on the int16 wire of a sharded bucket.
 * Included by ina.h after ina_switch_blk.h; ina_blk.h's contract holds here; do not include it on
 * its own.
 *
 * The block-scaled siblings of ina_quantize_f32_i16_wire and ina_i16_wire_finish (ina.h): element e
 * is scaled by 2^kblk[e / V] where the sibling takes 2^k, so on block s the result is bit for bit
 * the sibling's on that block alone with k = kblk[s] -- wire words, int16 sums, y, and the block's
 * flag (V is also the slot size of the flags: one flag per block).
 *
 *   kblk holds ceil(n / V) device bytes and no byte outside kblk[0 .. ceil(n / V)) is read.  A
 *     given -127 / -128 is read as -126.  wire_sum and kblk may start in the middle of a bucket (a
 *     rank's shard); the caller guarantees that the shard starts on a block boundary, and kblk[0]
 *     is the scale of wire_sum's first block.
 *   Ranks agree on a block's scale before they quantise (the MIN of their ina_block_scales_f32 for
 *     the job's number of summands and 16 bits); the summed wire decoded with the same scales then
 *     equals ina_quantize_reduce_blk_f32_i16_sat over the ranks' buckets, flags included.
 *   Checks: V >= 1; n == 0 is a no-op; a null kblk, x, wire or wire_sum is INA_EINVAL before any
 *     device work.  out16, y and overflow_per_slot may each be NULL; every flag of
 *     overflow_per_slot[0 .. ceil(n / V)) is written.
 *
 * fp32 buckets only.
 */
#ifndef INA_SHARD_BLK_H
#define INA_SHARD_BLK_H

#ifndef INA_SWITCH_BLK_H
#error "include ina.h, which includes ina_switch_blk.h and ina_shard_blk.h"
#endif

/* ina_quantize_f32_i16_wire with 2^kblk[e / V] for element e */
int ina_quantize_blk_f32_i16_wire(const float* x, const int8_t* kblk, int V, int32_t* wire, size_t n,
                                  ina_stream_t stream);
/* ina_i16_wire_finish; y (when asked for) is scaled by 2^-kblk[e / V] */
int ina_i16_wire_finish_blk(const int32_t* wire_sum, size_t n, const int8_t* kblk, int V, int16_t* out16,
                            float* y, uint8_t* overflow_per_slot, ina_stream_t stream);

#endif /* INA_SHARD_BLK_H */
