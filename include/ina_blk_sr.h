/*
 * ina_blk_sr.h -- stochastic rounding (ina_sr.h) with per-block scales (ina_blk.h): the bulk quantisers,
 * the fused quantise + reduce calls and the sharded wires.  Included by ina.h directly after
 * ina_reduce_sr.h's declarations (that header's last line includes this one); do not include it on its
 * own.
 *
 * Per-block scales keep the bits of a narrow wire on every layer; stochastic rounding keeps the
 * components below half a quantum without a residual.  An int16 job wants both (64 ranks leave 9 bits a
 * rank), and so does every place where error feedback cannot serve: bf16 / fp16 buckets on the wire
 * calls, and a GPU that sums other workers' values (layout B of config 5).  The packet path has the pair
 * in ina_pkt_sr.h; these are the calls off it.  The decode side needs nothing new: ina_dequantize_blk_*
 * and ina_i16_wire_finish_blk* do no rounding.
 *
 * Contract.  For element e of worker w's bucket, in block s = e / V, in fp32, unfused (a 16-bit value is
 * widened exactly first):
 *     t   = bufs[w][e] * 2^kblk[s]        a given scale of -127 or -128 is read as -126; the library
 *                                         never writes one
 *     y_w = ina_sr.h's y of t
 *   the random word from Philox4x32-10 under the key sr->seed at the counter
 *   ((sr->e0 + e) >> 2, sr->step, sr->sub + w mod 2^32), output word (sr->e0 + e) & 3; a single-bucket
 *   call has w = 0.  The scale has no part in the random stream.
 *     int32:       out[e]  = sum_w q32_of(y_w) mod 2^32
 *     int16 wire:  wire[e] = q16 + (sat << INA_I16_WIRE_SHIFT) of y_0
 *     int16:       a = sum_w q16_of(y_w) in int32, each summand saturated at the wire's width;
 *                  out[e] = sat16(a); the flag of block s is 1 if any summand or the sum saturated or
 *                  any y_w was NaN, else 0.  One flag per block, and every flag is written when
 *                  overflow_per_slot is not NULL.
 *   The clamps and the NaN handling are the siblings' (NaN -> 0, +-inf saturates).
 *   Computed scales (INA_BLK_AUTO, and ina_block_scales_sr_*) are exactly what
 *     ina_scale_for_sr(amax_s, degree, bits) returns for the block's max |value| over the call's
 *     buffers -- ina_block_scales_sr_f32's rule, lim = (2^(bits-1) - 1) / degree - 1, which leaves a
 *     whole quantum of headroom per summand; an all-zero or all-NaN block gives 127, a block holding
 *     +-inf gives -126, as in ina_blk.h.  A degree that ina_scale_for_sr refuses is INA_EINVAL before
 *     any device work.
 *   No call takes a base: the round-to-nearest siblings take none.
 * Consequences:
 *   Per block.  On block s the result is bit for bit the global-k stochastic sibling's
 *     (ina_quantize_sr_*, ina_quantize_reduce_sr_*) on that block alone, called with k = kblk[s] and
 *     e0 + s*V -- values, saturation and flag, on the vector and on the value-by-value path, for any
 *     grid and any W specialisation.  (For a V that is not a multiple of 4 the block's start is not a
 *     valid e0: the replay then takes the words of the whole bucket, not one call per block.)
 *   Composition.  The fused int32 result equals ina_sum_reduce_i32 of the W single-bucket results called
 *     with sub + w.  The fused int16 result equals the saturating sum of the W one-worker fused results
 *     called with sub + w, the flags OR-ed.
 *   Integers.  Where every t is an integer, the result is the round-to-nearest block sibling's
 *     (ina_blk.h, ina_x16_blk.h, ina_shard_blk.h, ina_shard_x16.h) for every seed.
 *   Slices.  Reducing x[lo:hi) with lo a multiple of V and of 4, e0 = lo and kblk + lo / V gives that
 *     slice of the whole-bucket result.
 *   Layouts.  With sub = 0, e0 = lo and degree = W = world, the AUTO reduce over all ranks' slices of
 *     [lo, hi) gives the same bits as the sharded step whose ranks round on stream r and agree on
 *     scales by MIN (ina_block_scales_sr_* of the rank's bucket for `world` summands, the element-wise
 *     MIN, ina_quantize_blk_sr_*_i32 or _i16_wire with sub = r, an integer SUM, the owner's decode) --
 *     the integers, the flags and the scales, on both wires.  ina_scale_for_sr is monotone in amax, so
 *     the MIN of the ranks' scales is the scale of their joint max.
 *
 * Argument checks: each function is its round-to-nearest sibling's argument list (ina_blk.h,
 * ina_x16_blk.h, ina_shard_blk.h, ina_shard_x16.h) with `sr` before `stream`; the scales call draws
 * nothing and keeps its sibling's list unchanged.  The sibling's checks come first, in its order and
 * with its messages -- the type code on the x16 calls, V, mode / degree / kblk, the n == 0 no-op, the
 * pointers -- then a null sr ("null sr") and sr->e0 % 4 != 0 ("e0 must be a multiple of 4").  Each is
 * INA_EINVAL before any device work.  *sr is copied into the kernel arguments during the call.
 *
 * Layout: the round-to-nearest block kernels' lanes (ina_blk.h) with one Philox call per worker's chunk
 * of 4 values.  V a power of two in [8, 256] with fp32 / int32 buffers 16-byte aligned and 16-bit
 * sources and the int16 out 8-byte aligned takes the vector path; any other V or alignment takes a
 * value-by-value path with identical results.  Every grid is under the default cap (ina_set_tuning
 * key 0).
 *
 * Not here: a standalone int16 quantiser (the W = 1 fused call, ina_quantize_reduce_blk_sr_*_i16_sat
 * with INA_BLK_GIVEN, is that operation), a base, error feedback combined with stochastic rounding, the
 * PS combine, and a pipelined sharded step (chunks > 1).
 */
#ifndef INA_BLK_SR_H
#define INA_BLK_SR_H

#ifndef INA_REDUCE_SR_H
#error "include ina.h, which includes ina_reduce_sr.h and ina_blk_sr.h"
#endif

/* ina_block_scales_x16 under ina_scale_for_sr's rule (fp32 buckets: ina_block_scales_sr_f32, ina_pkt_sr.h) */
int ina_block_scales_sr_x16(const void* const* xs, int xtype, int W, const float* base, size_t n, int V,
                            int degree, int bits, int8_t* kblk, ina_stream_t stream);
/* ina_quantize_blk_f32_i32 / ina_quantize_blk_x16_i32, rounded stochastically */
int ina_quantize_blk_sr_f32_i32(const float* x, const int8_t* kblk, int V, int32_t* q, size_t n,
                                const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_blk_sr_x16_i32(const void* x, int xtype, const int8_t* kblk, int V, int32_t* q, size_t n,
                                const ina_sr_t* sr, ina_stream_t stream);
/* ina_quantize_blk_f32_i16_wire / ina_quantize_blk_x16_i16_wire: the sharded int16 wire's words */
int ina_quantize_blk_sr_f32_i16_wire(const float* x, const int8_t* kblk, int V, int32_t* wire, size_t n,
                                     const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_blk_sr_x16_i16_wire(const void* x, int xtype, const int8_t* kblk, int V, int32_t* wire,
                                     size_t n, const ina_sr_t* sr, ina_stream_t stream);
/* ina_quantize_reduce_blk_{f32,x16}_i32 / _i16_sat, each summand rounded stochastically; INA_BLK_AUTO
 * computes the scales under ina_scale_for_sr's rule for `degree` summands */
int ina_quantize_reduce_blk_sr_f32_i32(const float* const* bufs, int W, int8_t* kblk, int mode, int degree,
                                       int V, int32_t* out, size_t n, const ina_sr_t* sr,
                                       ina_stream_t stream);
int ina_quantize_reduce_blk_sr_f32_i16_sat(const float* const* bufs, int W, int8_t* kblk, int mode,
                                           int degree, int V, int16_t* out, size_t n,
                                           uint8_t* overflow_per_slot, const ina_sr_t* sr,
                                           ina_stream_t stream);
int ina_quantize_reduce_blk_sr_x16_i32(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode,
                                       int degree, int V, int32_t* out, size_t n, const ina_sr_t* sr,
                                       ina_stream_t stream);
int ina_quantize_reduce_blk_sr_x16_i16_sat(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode,
                                           int degree, int V, int16_t* out, size_t n,
                                           uint8_t* overflow_per_slot, const ina_sr_t* sr,
                                           ina_stream_t stream);

#endif /* INA_BLK_SR_H */
