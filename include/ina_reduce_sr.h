/*
 * ina_reduce_sr.h -- stochastic rounding (ina_sr.h) in the fused quantise + reduce calls: the GPU that
 * holds W workers' buckets (configs 2 and 4, layout B of config 5) rounds each summand without bias
 * and sums it in the same launch.  Included by ina.h directly after ina_pkt_sr.h; do not include it on
 * its own.
 *
 * Error feedback cannot serve here -- the summing GPU does not own the workers' residuals (ina_ef.h)
 * -- and the unfused way, W ina_quantize_sr_* launches into W int32 temporaries and a sum reduce, moves
 * W * (4 + 4) + W * 4 + 4 bytes a value where these calls move W * 4 + 4 (half of that from 16-bit
 * buckets) and keep no temporary.
 *
 * Contract.  For element e of worker w's bucket, in fp32, unfused (a 16-bit value is widened exactly
 * first):
 *     y_w = ina_sr.h's y of t = bufs[w][e] * 2^k
 *   the random word from Philox4x32-10 under the key sr->seed at the counter
 *   ((sr->e0 + e) >> 2, sr->step, sr->sub + w mod 2^32), output word (sr->e0 + e) & 3: worker w draws
 *   from stream sub + w, the rule of the multi-worker packs (ina_pkt_sr.h).  There is no base, as in
 *   the round-to-nearest siblings.
 *     int32:  out[e] = sum_w q32_of(y_w) mod 2^32
 *     int16:  a = sum_w q16_of(y_w) in int32, each summand saturated at the wire's width;
 *             out[e] = sat16(a); the flag of slot e / V is 1 if any summand or the sum saturated or
 *             any y_w was NaN, else 0.  Every flag is written when overflow_per_slot is not NULL.
 *   q32_of / q16_of / sat16 are the siblings' clamps and NaN handling (NaN -> 0, +-inf saturates).
 * Consequences:
 *   Composition.  The int32 result equals ina_sum_reduce_i32 of the W ina_quantize_sr_{f32,x16}_i32
 *     results called with sub + w, bit for bit; the int16 result equals ina_sum_reduce_i16_sat of the
 *     W ina_quantize_sr_{f32,x16}_i16_sat results, the flags OR-ed -- whatever the grid, the
 *     alignment, the W specialisation or the path.
 *   Integers.  Where every t is an integer, the result is the nearest sibling's for every seed.
 *   Slices.  Reducing bufs[w][lo:hi) with e0 = lo (lo a multiple of V on the int16 calls) gives that
 *     slice of the whole-bucket result.
 *   Layouts.  With sub = 0, step = t and e0 = lo, the reduce over all ranks' slices of the range
 *     [lo, hi) equals that range of the integer aggregate of a sharded step at step t
 *     (ShardedAggregator(rounding="stochastic"), which rounds rank r on stream r), on the int32 and
 *     on the int16 wire: layouts A and B of config 5 give the same bits.
 *
 * Argument checks: each function is its round-to-nearest sibling's argument list (ina.h, ina_x16.h)
 * with `sr` before `stream`.  The sibling's checks come first, in its order and with its messages --
 * the type code on the x16 calls, k, V, the n == 0 no-op, W in [1, INA_MAX_WORKERS], a null worker
 * buffer, a 16-bit buffer that is not 2-byte aligned, a null out -- then a null sr ("null sr") and
 * sr->e0 % 4 != 0 ("e0 must be a multiple of 4").  Each is INA_EINVAL before any device work.  *sr is
 * copied into the kernel arguments during the call.
 *
 * Layout: the siblings' lanes with ina_sr.h's chunk of 4 values.  int32: lane i owns chunk i of every
 * worker -- one 16-byte (fp32) or 8-byte (bf16 / fp16) load per worker, W Philox calls, one 16-byte
 * store.  int16: a wave owns 512 values, lane l the 4 at 4l of each 256-value half, the slot flags
 * from two wave ballots.  The vector paths need fp32 / int32 buffers 16-byte aligned, 16-bit sources
 * and the int16 out 8-byte aligned and, for the slot flags, V with a ballot layout (V % 8 == 0, V / 8
 * a power of two <= 64); anything else takes a value-by-value path with identical results.
 *
 * Not here: a base, error feedback, and the PS combine.  Stochastic rounding with block scales
 * (ina_quantize_reduce_blk_sr_*) is in ina_blk_sr.h, which this header includes as its last line.
 */
#ifndef INA_REDUCE_SR_H
#define INA_REDUCE_SR_H

#ifndef INA_PKT_SR_H
#error "include ina.h, which includes ina_pkt_sr.h and ina_reduce_sr.h"
#endif

/* ina_quantize_reduce_f32_i32 / ina_quantize_reduce_f32_i16_sat, each summand rounded stochastically */
int ina_quantize_reduce_sr_f32_i32(const float* const* bufs, int W, int32_t* out, size_t n, int k,
                                   const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_reduce_sr_f32_i16_sat(const float* const* bufs, int W, int16_t* out, size_t n, int k, int V,
                                       uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream);
/* ina_quantize_reduce_x16_i32 / ina_quantize_reduce_x16_i16_sat: all W buffers of one xtype */
int ina_quantize_reduce_sr_x16_i32(const void* const* bufs, int xtype, int W, int32_t* out, size_t n, int k,
                                   const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_reduce_sr_x16_i16_sat(const void* const* bufs, int xtype, int W, int16_t* out, size_t n, int k,
                                       int V, uint8_t* overflow_per_slot, const ina_sr_t* sr,
                                       ina_stream_t stream);

#include "ina_blk_sr.h" /* the same with per-block scales; from here, since ina.h names no block-scale header
                         * with an infix */

#endif /* INA_REDUCE_SR_H */
