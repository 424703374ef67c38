/*
 * ina_i4.h -- a 4-bit wire for sharded buckets: each rank's block-scaled (and, with sr, rotated) values as
 * signed nibbles, two to a byte, and the sum of up to INA_MAX_WORKERS ranks' nibble slices -- exact into int16,
 * or rounded to bytes under a per-block shift for ina_i8_gather.h's decode.  Included by ina.h through
 * ina_rot.h, ina_i8.h, ina_i8_gather.h, ina_i8_ef.h and ina_i8_sr.h, whose last line includes this header; do
 * not include it on its own.
 *
 * The byte wire of ina_i8.h sends one byte a value in the all-to-all.  A uniform 4-bit code under the same
 * shared per-block scale is still homomorphic: the owner adds the words as integers, exactly, and decodes the
 * sum once.  That is what THC-style in-network aggregation sends -- a Hadamard-rotated block, 4 bits a value,
 * summed without decoding -- and everything on both sides of the word is here already and stays as it is: the
 * rotation that makes a block flat (ina_rot.h), the MIN agreement of the scales, the all-to-all, and the decodes
 * of the sums (ina_dequantize_rot_i16 / ina_dequantize_blk_i16_f32, or ina_dequantize_i8_gather).  G summands in
 * [-7, 7] sum to |S| <= 7 G: for G <= 18 ranks the exact sum is already a byte (7 * 18 = 126), the requantising
 * sum picks shift 0 and loses nothing; for G <= 64, |S| <= 512 and the shift is at most 3.  A step moves
 * 0.5 + 1 (+ 2/V) bytes a value on the links against 1 + 1 with ina_i8_gather.h and 1 + 2 with ina_i8.h.  (This
 * is arithmetic on bytes, not a timing of any link.)  Four bits resolve a block only once it is flat; the word
 * is opt-in (dist.NibbleWireAggregator) and nothing of the byte wire changes.
 *
 * Contract.  V = 2^m, m in [3, 8]; block s is elements [sV, (s+1)V); n is a multiple of V for the block calls.
 * All float arithmetic is fp32, unfused, round to nearest even; a bf16 / fp16 value is widened exactly first.
 *   The word.  A signed 4-bit two's-complement value in [-7, 7]; the quantiser never writes -8.  Value e lives
 *     in byte e / 2: even e in the low nibble, odd e in the high nibble.  A buffer of n values is n / 2 bytes.
 *   Scale rule.  ina_scale_for_i4(absmax, &k) gives the largest k in [-126, 127] with absmax * 2^k + 1/2 <= 7
 *     (-126 if there is none); absmax 0 gives 127.  The number of ranks does not enter.  Refused as
 *     ina_scale_for_i8 refuses: a null k_out, then absmax negative, NaN or infinite.
 *   Rotation.  ina_i8.h's: with sr != NULL, r is ina_rot.h's forward rotation of the block; with sr == NULL,
 *     r = x.
 *   ina_block_scales_i4.  ina_block_scales_i8 under that rule: kblk[s] = ina_scale_for_i4(max |r| of block s
 *     over the W buffers), about the rotated values when sr != NULL; NaN is ignored (an all-zero or all-NaN
 *     block gives 127), a block holding +-inf gives -126.  Ranks agree on the MIN of their scales.
 *   ina_quantize_i4_wire.  nibble[e] = clamp(rne(r[e] * 2^kblk[e/V]), -7, 7); NaN -> 0.  The scales are given
 *     (a scale of -127 or -128 is read as -126).  overflow_per_slot may be NULL; otherwise every block's flag
 *     is written: 1 where a value of the block clamped or was NaN, else 0.  The flag is rank-local and is not
 *     sent.
 *   ina_sum_i4_slices.  out16[e] = sum_g nibble of slices[g] at e, exact, for any nibbles (-8 included) and
 *     1 <= G <= INA_MAX_WORKERS.  n is any multiple of 8.  The decode is ina_dequantize_rot_i16 with the same
 *     *sr, or ina_dequantize_blk_i16_f32, on out16 with the agreed scales.
 *   ina_sum_i4_slices_requant.  S is that exact sum; shift and q8 follow exactly the rule of
 *     ina_sum_i8_slices_requant: with A = max |S| over block s, shift[s] is the smallest sh in [0, 7] with
 *     rne(A / 2^sh) <= 127, ties to even, in integers, and q8[e] = rne(S[e] / 2^shift[e/V]).  |S| <= 512, so
 *     the rule only ever yields sh <= 3 here (A = 127 -> 0, 128 -> 1, 254 -> 1, 255 -> 2, 509 -> 2, 510 -> 3,
 *     512 -> 3), and ina_dequantize_i8_gather decodes the output unchanged.  The int16 sums never reach memory.
 * Consequences: the decode of the sum of G ranks' nibbles equals the sum of the ranks' nibble * 2^-k pushed
 * through the inverse rotation; on quantiser output at G <= 18 every shift is 0 and both sums decode alike; on
 * a block of integer inputs at kblk = ceil(m/2) (0 without the rotation) the step returns the integer sum bit
 * for bit, provided every r * 2^kblk lies within [-7, 7] (a larger one clamps and raises the flag).
 *
 * Arguments.  xtype: INA_ROT_F32 (0), INA_X16_BF16 or INA_X16_F16.  x, q4, every bucket, every slice, out16 and
 * q8 are 16-byte aligned; shift may sit at any byte address; sr->e0 is a multiple of 128 and of V.  Refused
 * with INA_EINVAL, by name and before any device work, in this order.  The block calls, as in ina_i8.h: a bad
 * xtype; V not a power of two in [8, 256]; a null kblk; n not a multiple of V; (n == 0 is a no-op;) W outside
 * [1, INA_MAX_WORKERS] or null pointers; a buffer that is not 16-byte aligned; with sr != NULL, sr->e0 not a
 * multiple of 128 and of V.  The exact sum: G outside [1, INA_MAX_WORKERS] or a null slices; n not a multiple
 * of 8; (n == 0 is a no-op;) a null slice or out16; a slice or out16 that is not 16-byte aligned.  The
 * requantising sum, as ina_sum_i8_slices_requant: G outside [1, INA_MAX_WORKERS] or a null slices; V not a
 * power of two in [8, 256]; a null shift; n not a multiple of V; (n == 0 is a no-op;) a null slice or q8; a
 * slice or q8 that is not 16-byte aligned.  *sr is copied into the kernel arguments during the call.
 *
 * Layout.  Scales and quantiser: ina_rot.h's lanes (a lane owns 4 values, a block is V/4 adjacent lanes of one
 * wave); a lane's 4 nibbles leave as one 2-byte store, 128 contiguous bytes a wave.  Sums: a lane owns 32 values, one 16-byte load a slice; w ^
 * 0x88888888 makes every nibble unsigned, the even and the odd nibbles of a word are four byte fields each and
 * plain 32-bit adds accumulate up to 16 slices in them; the byte fields are then widened into 16-bit fields,
 * which take the batches of a larger G, and the bias 8 G comes off once at the end.  No LDS.  Every grid is
 * under the default cap (ina_set_tuning key 0).
 *
 * Not here: error feedback and stochastic rounding on this word (the word and the scale rule are stated so that
 * they can follow), a 4-bit gather, a 16-bit output of the decode, a pipelined step (chunks > 1), layout B, the
 * packet path, and bench.py.
 */
#ifndef INA_I4_H
#define INA_I4_H

#ifndef INA_I8_SR_H
#error "include ina.h, which includes ina_rot.h, ina_i8.h, ina_i8_gather.h, ina_i8_ef.h, ina_i8_sr.h and ina_i4.h"
#endif

/* the largest k in [-126, 127] with absmax * 2^k + 1/2 <= 7 (-126 if none; 127 for absmax = 0) */
int ina_scale_for_i4(float absmax, int* k_out);
/* the scales of the nibble wire: kblk[s] = ina_scale_for_i4(max |r| of block s over xs); sr == NULL: r = x */
int ina_block_scales_i4(const void* const* xs, int xtype, int W, size_t n, int V, int8_t* kblk,
                        const ina_sr_t* sr, ina_stream_t stream);
/* (rotate +) quantise one bucket to packed nibbles under given scales: n / 2 bytes */
int ina_quantize_i4_wire(const void* x, int xtype, const int8_t* kblk, int V, uint8_t* q4, size_t n,
                         uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream);
/* the exact sum of G nibble slices into int16 */
int ina_sum_i4_slices(const uint8_t* const* slices, int G, int16_t* out16, size_t n, ina_stream_t stream);
/* the sum of G nibble slices, each block rounded to bytes under shift[block] (ina_sum_i8_slices_requant's rule) */
int ina_sum_i4_slices_requant(const uint8_t* const* slices, int G, int V, int8_t* q8, uint8_t* shift, size_t n,
                              ina_stream_t stream);

#endif /* INA_I4_H */
