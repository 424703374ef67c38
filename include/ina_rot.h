/*
 * ina_rot.h -- a randomised Hadamard rotation in front of the block-scaled quantise and reduce (ina_blk.h).
 * Included by ina.h through ina_blk_sr.h, whose last line includes this header; do not include it on its
 * own.
 *
 * Inside one block the quantum is set by the block's largest value: a block with one large value and V - 1
 * values below half a quantum sends V - 1 zeros, whatever its exponent.  Rotating the block first -- a
 * diagonal of shared random signs, then a Walsh-Hadamard transform -- spreads its energy evenly, so its
 * largest value is a few times its RMS instead of up to sqrt(V) times, and the quantum shrinks by that
 * ratio.  The rotation is linear and the same on every worker, so the sum of rotated blocks is the rotated
 * sum: the wire, the switch and the scales are ina_blk.h's, and the receiver undoes the rotation once,
 * after the dequantise.
 *
 * Contract.  V = 2^m, m in [3, 8]; block s is elements [sV, (s+1)V); n is a multiple of V.  All arithmetic
 * is fp32, unfused, round to nearest; a bf16 / fp16 value is widened exactly first, so a 16-bit call equals
 * the fp32 call on the widened bucket.
 *   Signs.  g = sr->e0 + e.  sigma(e) = -1 where bit (g & 31) of output word (g >> 5) & 3 of
 *     Philox4x32-10 under the key sr->seed at the counter (g >> 7, sr->step, sr->sub) is set, else +1.
 *     Every worker of a call, and every rank of a job, uses this one stream (never sub + w).
 *   Forward.  t = sigma * x (a sign-bit flip).  For i = 0 .. m-1 in this order, h = 2^i: every pair
 *     (j, j + h) of the block with bit i of j clear becomes (t[j] + t[j+h], t[j] - t[j+h]).  Then
 *     r = t * 2^-ceil(m/2).  The stage order is part of the contract: every output is a fixed tree of
 *     fp32 adds, one bit pattern whatever the grid or the lanes (a NaN is a NaN: its sign and payload are
 *     not specified).
 *   Quantise.  ina_blk.h's quantisers on r * 2^kblk[s] (a given scale of -127 or -128 is read as -126):
 *     int32: out[e] = sum_w q32 mod 2^32.  int16: each summand and the sum saturated; the flag of block s
 *     is 1 if any summand or the sum saturated or any r was NaN, else 0; every flag is written when
 *     overflow_per_slot is not NULL.  NaN -> 0.  A NaN or an inf in a block spreads over that block only,
 *     as the adds dictate.
 *     INA_BLK_AUTO computes kblk[s] in the launch as ina_scale_for(max |r| over the call's W buffers,
 *     degree, bits) and writes it (all zero or all NaN: 127; a block holding +-inf: -126);
 *     ina_block_scales_rot computes the same scales alone, for the MIN agreement between ranks.
 *     Both rules are about the rotated values r, not the inputs.  The butterfly adds up to V values before
 *     the normalisation, so a block of finite inputs near the top of the fp32 range has r = +-inf (and NaN
 *     where inf - inf meets): it gets -126 and, on the int16 side, its flag.  An input +-inf whose r are
 *     all NaN (inf - inf in every output) counts as all NaN: it no longer decides the scale.
 *   Inverse.  y = float(sum) * 2^-kblk[s]; the same m stages in the same order give u;
 *     xhat = sigma * (u * 2^-floor(m/2)).
 *   PS combine.  ina_ps_combine_ina_rot_f32 is, bit for bit, ina_quantize_reduce_rot_i32 (INA_BLK_AUTO,
 *     degree = W) of the deltas paras[w] - local, ina_dequantize_rot_i32, then out = local + xhat *
 *     float(weight_step) in two fp32 operations -- in one launch.  kblk_out may be NULL.
 * Consequences: where every x is an integer and kblk[s] = ceil(m/2), every add is exact and the decode of
 * the int32 sum returns sum_w x_w bit for bit; slices [lo, hi) with lo a multiple of V and of 128 and
 * e0 = lo give that slice of the whole-bucket result.
 *
 * Arguments.  xtype: INA_ROT_F32 (0), INA_X16_BF16 or INA_X16_F16, the type of every bucket of the call.
 * Refused with INA_EINVAL, by name and before any device work, in this order: a bad xtype; V not a power
 * of two in [8, 256]; mode / degree / a null kblk as in ina_blk.h (a degree that ina_scale_for refuses);
 * n not a multiple of V; (n == 0 is a no-op;) null pointers; a bucket, `local` or an output that is not
 * 16-byte aligned; a null sr; sr->e0 not a multiple of 128 and of V.  There is no value-by-value path.
 * *sr is copied into the kernel arguments during the call.
 *
 * Layout: ina_blk.h's lanes (a lane owns 4 values, a block is V/4 adjacent lanes of one wave; int16 out:
 * the split halves).  Stages 0 and 1 run inside the lane, stage i >= 2 exchanges with lane ^ (1 << (i-2)).
 * The signs of a wave's 256 values are two Philox calls on the scalar unit.  Every grid is under the
 * default cap (ina_set_tuning key 0).
 *
 * Not here: the rotation combined with stochastic rounding, error feedback on the calls of this header, a
 * base, the sharded wires, the packet path, and V > 256.  A sharded wire that takes the rotation -- 8 bits a
 * value over an all-to-all -- is in ina_i8.h, which this header includes as its last line; the rotation
 * combined with error feedback, on that wire, is in ina_i8_ef.h further down the same chain, and the rotation
 * combined with stochastic rounding, on that wire, in ina_i8_sr.h at its end.
 */
#ifndef INA_ROT_H
#define INA_ROT_H

#ifndef INA_BLK_SR_H
#error "include ina.h, which includes ina_blk_sr.h and ina_rot.h"
#endif

#define INA_ROT_F32 0 /* xtype of fp32 buckets; 16-bit ones: INA_X16_BF16 / INA_X16_F16 */

/* the scales of the rotated values alone: kblk[s] = ina_scale_for(max |r| of block s over xs, degree, bits) */
int ina_block_scales_rot(const void* const* xs, int xtype, int W, size_t n, int V, int degree, int bits,
                         int8_t* kblk, const ina_sr_t* sr, ina_stream_t stream);
/* rotate + quantise + W-way sum (W = 1: the plain quantiser); mode INA_BLK_GIVEN reads kblk, INA_BLK_AUTO
 * writes it */
int ina_quantize_reduce_rot_i32(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode, int degree,
                                int V, int32_t* out, size_t n, const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_reduce_rot_i16_sat(const void* const* bufs, int xtype, int W, int8_t* kblk, int mode,
                                    int degree, int V, int16_t* out, size_t n, uint8_t* overflow_per_slot,
                                    const ina_sr_t* sr, ina_stream_t stream);
/* dequantise + inverse rotation into fp32 */
int ina_dequantize_rot_i32(const int32_t* sv, const int8_t* kblk, int V, float* y, size_t n, const ina_sr_t* sr,
                           ina_stream_t stream);
int ina_dequantize_rot_i16(const int16_t* sv, const int8_t* kblk, int V, float* y, size_t n, const ina_sr_t* sr,
                           ina_stream_t stream);
/* ina_ps_combine_ina_blk_f32 with the rotation on both sides of the integer sum */
int ina_ps_combine_ina_rot_f32(const float* local, const float* const* paras, int W, int V, double weight_step,
                               float* out, size_t n, int8_t* kblk_out, const ina_sr_t* sr, ina_stream_t stream);

#include "ina_i8.h" /* an 8-bit wire for sharded buckets: rotated blocks as bytes, byte slices summed to int16 */

#endif /* INA_ROT_H */
