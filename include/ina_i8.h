/*
 * ina_i8.h -- an 8-bit wire for sharded buckets: each rank's block-scaled (and, with sr, rotated) values as
 * int8 bytes, and the exact sum of up to INA_MAX_WORKERS ranks' byte slices into int16.  Included by ina.h
 * through ina_rot.h, whose last line includes this header; do not include it on its own.
 *
 * The integer wires of the sharded step put 4 bytes a value on the links of the reduce-scatter, because a
 * collective's SUM cannot saturate.  An all-to-all only moves bytes and the owner sums on its device, so a
 * wire word may be a byte: a rank quantises to [-127, 127] under per-block scales, sends slice j to rank j,
 * and rank j adds the G bytes of every value into an int16, which holds them exactly (64 * 128 = 8192).
 * There is no saturation on the owner, so no count bits and no flags travel; the all-gather moves the int16
 * sums, and ina_dequantize_rot_i16 (rotated) or ina_dequantize_blk_i16_f32 (plain) decodes them with the
 * agreed scales.  A step moves 1 + 2 bytes a value where the int16 wire moves 4 + 2 and the int32 wire 4 + 4.
 * Eight bits resolve a block only once it is flat, which is what ina_rot.h's rotation is for.
 *
 * Contract.  V = 2^m, m in [3, 8]; block s is elements [sV, (s+1)V); n is a multiple of V for the two block
 * calls.  All arithmetic is fp32, unfused, round to nearest even; a bf16 / fp16 value is widened exactly
 * first, so a 16-bit call equals the fp32 call on the widened bucket.
 *   Scale rule.  ina_scale_for_i8(absmax, &k) gives the largest k in [-126, 127] with
 *     absmax * 2^k + 1/2 <= 127 (-126 if there is none); absmax 0 gives 127.  The number of ranks does not
 *     enter: headroom for the sum comes from the int16 accumulator, not from the summand.  Refused as
 *     ina_scale_for refuses: a null k_out, then absmax negative, NaN or infinite.
 *   Rotation.  With sr != NULL, r is ina_rot.h's forward rotation of the block -- the same signs (g = sr->e0
 *     + e, one stream for every rank, never sub + rank), the same stage order, the same 2^-ceil(m/2).  With
 *     sr == NULL, r = x.
 *   ina_block_scales_i8.  kblk[s] = ina_scale_for_i8(max |r| of block s over the W buffers); an all-zero or
 *     all-NaN block gives 127, a block holding +-inf gives -126.  Ranks agree on the MIN of their scales
 *     before they quantise, as on the other block-scaled wires.  With sr != NULL these rules are about the
 *     rotated values r, as in ina_rot.h: finite inputs whose butterfly overflows give -126 (and clamp, so
 *     the quantiser raises the block's flag), and an input inf whose r are all NaN no longer decides the
 *     scale.
 *   ina_quantize_i8_wire.  q8[e] = clamp(rne(r[e] * 2^kblk[e/V]), -127, 127); NaN -> 0; -128 is never
 *     written.  The scales are given (a scale of -127 or -128 is read as -126).  overflow_per_slot may be
 *     NULL; otherwise every block's flag is written: 1 where a value of the block clamped or was NaN, else 0.
 *     The flag is rank-local and is not sent.
 *   ina_sum_i8_slices.  out16[e] = sum_g (int)slices[g][e], exact, for any int8 bytes (-128 included) and
 *     1 <= G <= INA_MAX_WORKERS: G * 128 <= 32767 holds by that limit.  n is any value >= 0; a ragged tail
 *     (n mod 16) is handled inside the kernel.
 *   Decode.  No entry point here: ina_dequantize_rot_i16 with the same *sr, or ina_dequantize_blk_i16_f32,
 *     on out16 with the agreed scales.
 * Consequences: the decode of the int16 sum of G ranks' q8 equals the sum of the ranks' q8 * 2^-k pushed
 * through the inverse rotation; on a block of integer inputs at kblk = ceil(m/2) (0 without the rotation) it
 * returns the integer sum bit for bit, provided every r * 2^kblk lies within [-127, 127] (a larger one
 * clamps and raises the flag).
 *
 * Arguments.  xtype: INA_ROT_F32 (0), INA_X16_BF16 or INA_X16_F16.  x, q8, every bucket, every slice and
 * out16 are 16-byte aligned; sr->e0 is a multiple of 128 and of V.  Refused with INA_EINVAL, by name and
 * before any device work, in this order.  The block calls: a bad xtype; V not a power of two in [8, 256]; a
 * null kblk; n not a multiple of V; (n == 0 is a no-op;) W outside [1, INA_MAX_WORKERS] or null pointers; a
 * buffer that is not 16-byte aligned; with sr != NULL, sr->e0 not a multiple of 128 and of V.  The sum: G
 * outside [1, INA_MAX_WORKERS] or a null slices; (n == 0 is a no-op;) a null slice or out16; a slice or out16
 * that is not 16-byte aligned.  *sr is copied into the kernel arguments during the call.
 *
 * Layout.  Scales and quantiser: ina_rot.h's lanes (a lane owns 4 values, a block is V/4 adjacent lanes of
 * one wave); a lane's 4 bytes leave as one dword, 256 contiguous bytes a wave.  Sum: a lane owns 16 values;
 * it adds the even and the odd bytes of each 32-bit word as two 16-bit fields of two words (the bytes made
 * unsigned by flipping their sign bits, the G * 128 taken off again per field), and writes 32 bytes of
 * int16.  Every grid is under the default cap (ina_set_tuning key 0).
 *
 * Not here: stochastic rounding on this wire, a base, layout B, the packet path, a pipelined step
 * (chunks > 1), a requantised 8-bit gather, error feedback, and bench.py.  The requantised gather -- the sums
 * rounded back to bytes under a per-block shift, and a decode that reads them -- is in ina_i8_gather.h, which
 * this header includes as its last line; error feedback on this wire -- the rounding error carried back
 * through the inverse rotation into a rank-local residual, in the quantiser's launch -- is in ina_i8_ef.h,
 * which that header includes as its last line; stochastic rounding on this wire -- the byte quantiser and the
 * requantised gather -- is in ina_i8_sr.h further down the same chain, and a 4-bit wire word in ina_i4.h at its end.
 */
#ifndef INA_I8_H
#define INA_I8_H

#ifndef INA_ROT_H
#error "include ina.h, which includes ina_rot.h and ina_i8.h"
#endif

int ina_scale_for_i8(float absmax, int* k_out);
/* the scales of the byte wire: kblk[s] = ina_scale_for_i8(max |r| of block s over xs); sr == NULL: r = x */
int ina_block_scales_i8(const void* const* xs, int xtype, int W, size_t n, int V, int8_t* kblk,
                        const ina_sr_t* sr, ina_stream_t stream);
/* (rotate +) quantise one bucket to bytes under given scales */
int ina_quantize_i8_wire(const void* x, int xtype, const int8_t* kblk, int V, int8_t* q8, size_t n,
                         uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream);
/* the exact sum of G byte slices into int16 */
int ina_sum_i8_slices(const int8_t* const* slices, int G, int16_t* out16, size_t n, ina_stream_t stream);

#include "ina_i8_gather.h" /* a requantised 8-bit gather: the slice sums as bytes under per-block shifts */

#endif /* INA_I8_H */
