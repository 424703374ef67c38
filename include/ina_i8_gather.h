/*
 * ina_i8_gather.h -- a requantised 8-bit gather for the byte wire of ina_i8.h: the owner of a shard sums the G
 * received byte slices and rounds each block of sums back to bytes under a small per-block shift, in one
 * launch; the all-gather then carries one byte a value plus one byte a block, and a decode reads those bytes
 * directly.  Included by ina.h through ina_rot.h and ina_i8.h, whose last line includes this header; do not
 * include it on its own.
 *
 * ina_i8.h's step moves 1 byte a value in the all-to-all and 2 in the all-gather (the exact int16 sums).  With
 * this header the gather moves 1 + 1/V: a step is 1 + 1 bytes a value (plus 2/V for the scales and the
 * shifts) against 3, against 6 on the int16 wire and 8 on the int32 wire.  It is not free: a sum of G bytes
 * carries more than 8 significant bits, and rounding it to 8 adds up to half of 2^shift summand quanta to the
 * G halves already there.  So it is opt-in (dist.ByteWireAggregator(gather="i8")), and nothing of ina_i8.h
 * changes.
 *
 * Contract.  V = 2^m, m in [3, 8]; block s is elements [sV, (s+1)V); n is a multiple of V.  Everything on the
 * owner's side is integer arithmetic.
 *   ina_sum_i8_slices_requant.  S[e] = sum_g (int)slices[g][e], exact, for any int8 bytes (-128 included) and
 *     1 <= G <= INA_MAX_WORKERS, so |S| <= 8192.  With A = max |S| over block s, shift[s] is the smallest sh
 *     in [0, 7] with rne(A / 2^sh) <= 127, rne being round half to even of the exact quotient (A = 127 -> 0,
 *     128 -> 1, 254 -> 1, 255 -> 2, 510 -> 3, 8129 -> 6, 8192 -> 7).  That is s0 = max(0, bitlen(A) - 7), plus
 *     one where rne(A / 2^s0) = 128.  q8[e] = rne(S[e] / 2^shift[e/V]); rounding is monotone, so nothing
 *     clamps and -128 is never written.  In integers, for sh >= 1, rne(S / 2^sh) = (S + 2^(sh-1) - 1 +
 *     ((S >> sh) & 1)) >> sh with an arithmetic shift, and S for sh = 0; every intermediate stays within
 *     +-8256, so the requantiser runs in 16-bit fields.  An all-zero block gives shift 0 and zeros.  The
 *     int16 sums are never written to memory.
 *   ina_dequantize_i8_gather.  Defined by its consequence: with sr != NULL, y is bit for bit what
 *     ina_dequantize_rot_i16 returns on the int16 array (int16)q8[e] << shift[e/V] with the same kblk, V and
 *     *sr; with sr == NULL, what ina_dequantize_blk_i16_f32 returns on that array.  float(q8) * 2^shift is an
 *     exact fp32 integer of at most 16256, so the decode rounds where those decodes round and nowhere else.
 *     A shift byte above 7 is read as 7; a scale of -127 or -128 is read as -126.
 * Consequences: on a block whose sums stay within [-127, 127] the shift is 0 and the step is ina_i8.h's, bit
 * for bit; otherwise a decoded block differs from ina_i8.h's by the inverse rotation of at most
 * 2^(shift-1) * 2^-kblk a value.
 *
 * Arguments.  Every slice, q8 and y are 16-byte aligned; shift may sit at any byte address; sr->e0 is a
 * multiple of 128 and of V.  Refused with INA_EINVAL, by name and before any device work, in this order.  The
 * sum: G outside [1, INA_MAX_WORKERS] or a null slices; V not a power of two in [8, 256]; a null shift; n not
 * a multiple of V; (n == 0 is a no-op;) a null slice or q8; a slice or q8 that is not 16-byte aligned.  The
 * decode: V not a power of two in [8, 256]; n not a multiple of V; (n == 0 is a no-op;) a null q8, y or kblk;
 * a null shift; q8 or y not 16-byte aligned; with sr != NULL, sr->e0 not a multiple of 128 and of V.  *sr is
 * copied into the kernel arguments during the call.
 *
 * Layout.  Sum: ina_sum_i8_slices' lanes -- a lane owns 16 values and adds the even and the odd bytes of each
 * 32-bit word as two 16-bit fields of two words.  The 8 words of sums stay in registers: |S| per field and
 * the lane's maximum in packed 16-bit arithmetic, the block's maximum over its V/16 adjacent lanes by
 * row-level DPP (V = 256 is one row of 16 lanes; V = 8 is two blocks inside a lane; nothing crosses a row),
 * the packed round-and-shift, one v_perm_b32 per pair of words into element order, one 16-byte store a lane
 * and one shift byte from the block's first lane.  Decode: ina_rot.h's lanes (a lane owns 4 values, one dword
 * of bytes; a block is V/4 adjacent lanes of one wave), the scale and the shift one byte load each.  Every
 * grid is under the default cap (ina_set_tuning key 0).
 *
 * Not here: stochastic rounding on either half of the wire, error feedback on the requantiser's rounding, a
 * 4-bit word, a 16-bit output of the decode, layout B, the packet path, a pipelined step (chunks > 1), and
 * bench.py.  Error feedback on the rank's own rounding -- the first half of the wire -- is in ina_i8_ef.h,
 * which this header includes as its last line; stochastic rounding on both halves has since come in ina_i8_sr.h.
 */
#ifndef INA_I8_GATHER_H
#define INA_I8_GATHER_H

#ifndef INA_I8_H
#error "include ina.h, which includes ina_rot.h, ina_i8.h and ina_i8_gather.h"
#endif

/* the sum of G byte slices, each block rounded to bytes under shift[block] */
int ina_sum_i8_slices_requant(const int8_t* const* slices, int G, int V, int8_t* q8, uint8_t* shift, size_t n,
                              ina_stream_t stream);
/* ina_dequantize_rot_i16 (sr != NULL) or ina_dequantize_blk_i16_f32 (sr == NULL) of (int16)q8 << shift[block] */
int ina_dequantize_i8_gather(const int8_t* q8, const uint8_t* shift, const int8_t* kblk, int V, float* y, size_t n,
                             const ina_sr_t* sr, ina_stream_t stream);

#include "ina_i8_ef.h" /* error feedback on the byte wire: the residual carried through the rotation */

#endif /* INA_I8_GATHER_H */
