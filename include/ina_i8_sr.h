/*
 * ina_i8_sr.h -- unbiased stochastic rounding on both halves of the 8-bit wire of ina_i8.h: the rank's byte
 * quantiser and the owner's requantised gather (ina_i8_gather.h) round up or down by chance, with the chance
 * set so that the expectation is the value itself.  It is the stateless alternative to ina_i8_ef.h's residual:
 * nothing is kept between steps, no extra byte moves, and it is the only answer to the second rounding, which
 * rounds sums of other ranks' values and which no rank-local residual can reach.  Included by ina.h through
 * ina_rot.h, ina_i8.h, ina_i8_gather.h and ina_i8_ef.h, whose last line includes this header; do not include it
 * on its own.
 *
 * Under round-to-nearest a rotated component below half a quantum is sent as zero on every step, and so is the
 * low part of a sum under a shift; with this header both are sent as one quantum now and then, as often as they
 * are large.  Nothing on the links changes: the bytes, the MIN of the scales, the shifts and both decodes are
 * ina_i8.h's and ina_i8_gather.h's.  The default of dist.ByteWireAggregator stays round-to-nearest.
 *
 * Contract.  V, the blocks, xtype, the alignment and the rotation are ina_i8.h's.  Two streams of ina_sr.h's
 * generator (Philox4x32-10 under the key `seed`) are separate arguments: *rot drives the rotation's signs and is
 * shared by every rank; *rnd drives the rounding and no two ranks may share it.
 *   ina_scale_for_i8_sr.  The largest k in [-126, 127] with absmax * 2^k + 1 <= 127, -126 if there is none, 127
 *     for absmax = 0: stochastic rounding can round up by almost a whole quantum, so it takes ina_scale_for_sr's
 *     whole quantum of headroom where ina_scale_for_i8 takes half.  Host only.  (The device limit is 126.0 where
 *     ina_scale_for_i8's is 126.5.)
 *   ina_block_scales_i8_sr.  ina_block_scales_i8 under that rule: kblk[s] = ina_scale_for_i8_sr(max |r| of block s
 *     over the W buckets); an inf in the block gives -126 and NaNs are ignored, as there.  rot may be NULL (no
 *     rotation).  The scale takes no part in any random stream.
 *   ina_quantize_sr_i8_wire.  r is ina_i8.h's: the forward rotation of the block of x under *rot, or x itself for
 *     rot == NULL.  Per element e, fp32, unfused:
 *         t = r * 2^kblk[e/V]          (-127 and -128 are read as -126)
 *         f = floor(t);  p = t - f;  u = float(word >> 8) * 2^-24;  y = f + (u < p ? 1 : 0)      (ina_sr.h's y)
 *         q8 = clamp(y, -127, 127), NaN -> 0                                    (-128 is never written)
 *     word is output word (rnd->e0 + e) & 3 of Philox4x32-10 under rnd->seed at the counter
 *     ((rnd->e0 + e) >> 2, rnd->step, rnd->sub), the high half of the index in counter word 1.  The flag of block
 *     s is ina_quantize_i8_wire's: 1 where a value of the block clamped or was NaN (overflow_per_slot may be
 *     NULL).  +-inf stays +-inf through y and clamps.
 *   ina_sum_i8_slices_requant_sr.  S[e] = sum_g (int)slices[g][e], exact, as in ina_i8_gather.h, and A = max |S|
 *     over block s.  shift[s] is the smallest sh in [0, 7] with ceil(A / 2^sh) <= 127, that is A <= 127 << sh
 *     (A = 127 -> 0, 128 -> 1, 254 -> 1, 255 -> 2, 508 -> 2, 509 -> 3, 8128 -> 6, 8129 -> 7, 8192 -> 7): s0 =
 *     max(0, bitlen(A) - 7), plus one where A > 127 << s0.  It differs from ina_sum_i8_slices_requant's rule only
 *     where that one relies on rounding down.  With g = rnd->e0 + e,
 *         q8[e] = (S[e] + u[e]) >> sh          (an arithmetic shift),   u[e] = byte & (2^sh - 1),
 *     byte being byte g & 3 (byte 0 the lowest) of output word (g >> 2) & 3 of Philox4x32-10 under rnd->seed at
 *     the counter (g >> 4, rnd->step, rnd->sub), the high half of g >> 4 in counter word 1: one call is 16 bytes,
 *     the 16 values a lane of the slice sum owns.  Integers only: q8 rounds up with probability
 *     (S mod 2^sh) / 2^sh exactly; |S + u| <= 8192 + 127, so it runs in the sum's 16-bit fields; neither -128 nor
 *     a clamp can occur; sh = 0 writes S.  The int16 sums never reach memory.  The decode is
 *     ina_dequantize_i8_gather, unchanged.
 * Consequences.
 *   Replay.  Every byte, flag, shift and scale is bit for bit the replay of the lines above, whatever the grid.
 *   Integers.  Where t is an integer, p = 0 and the quantiser equals ina_quantize_i8_wire for every seed.
 *   Shift 0.  A block whose A <= 127 has shift 0 and ina_sum_i8_slices_requant's bytes.
 *   Slices.  A call on the elements [lo, hi) of a bucket with rnd->e0 = lo (and rot->e0 = lo) gives that slice of
 *     the whole-bucket result.
 *   Bias.  E[y] = t up to the 2^-24 grain of u on the first half; E[q8] * 2^sh = S exactly on the second.
 *
 * Arguments.  As in ina_i8.h and ina_i8_gather.h; rnd is required; rnd->e0 is a multiple of 4 for the quantiser
 * (a lane's 4 values share one call) and of 16 for the sum.  Refused with INA_EINVAL, by name and before any
 * device work, in this order.  The scales: ina_block_scales_i8's.  The quantiser: ina_quantize_i8_wire's, in its
 * order and with its messages -- a bad xtype; V not a power of two in [8, 256]; a null kblk; n not a multiple of
 * V; (n == 0 is a no-op;) a null x or q8; a buffer that is not 16-byte aligned; with rot != NULL, rot->e0 not a
 * multiple of 128 and of V -- then a null rnd ("null rnd"), then rnd->e0 not a multiple of 4.  The sum:
 * ina_sum_i8_slices_requant's -- G outside [1, INA_MAX_WORKERS] or a null slices; V; a null shift; n not a
 * multiple of V; (n == 0 is a no-op;) a null slice or q8; a slice or q8 that is not 16-byte aligned -- then a
 * null rnd, then rnd->e0 not a multiple of 16.  ina_scale_for_i8_sr refuses what ina_scale_for_i8 refuses.  *rot
 * and *rnd are copied into the kernel arguments during the call.
 *
 * Layout.  Quantiser: ina_rot.h's lanes -- a lane owns 4 values, a block is V/4 adjacent lanes of one wave.  The
 * lane issues its one Philox call (the rounding key in scalar registers) ahead of its load and the butterfly,
 * which it does not depend on, rounds its 4 rotated values with the call's 4 words, clamps, packs and stores one
 * dword of bytes; the block's first lane writes the flag.  Sum: ina_sum_i8_slices_requant's lanes and front -- a
 * lane owns 16 values as 16-bit fields of 8 words, the block maximum by packed 16-bit arithmetic and row-level
 * DPP.  The lane's one Philox call is split into even and odd bytes by the masks that split the data, so the
 * random fields sit in the sums' layout; a packed mask with 2^sh - 1, a packed 16-bit add and a packed
 * arithmetic shift per word, then one v_perm_b32 per pair of words into element order.  No LDS.  Every grid is
 * under the default cap (ina_set_tuning key 0).
 *
 * Not here: stochastic rounding combined with error feedback, a 4-bit word, fewer Philox rounds or a shorter u
 * on the first half, scales computed in the quantiser's launch (an AUTO mode), layout B, the packet path, a
 * pipelined step (chunks > 1), and bench.py.  The 4-bit word -- round to nearest, packed nibbles and their slice
 * sums -- has since come in ina_i4.h, which this header includes as its last line.
 */
#ifndef INA_I8_SR_H
#define INA_I8_SR_H

#ifndef INA_I8_EF_H
#error "include ina.h, which includes ina_rot.h, ina_i8.h, ina_i8_gather.h, ina_i8_ef.h and ina_i8_sr.h"
#endif

/* the largest k in [-126, 127] with absmax * 2^k + 1 <= 127 (-126 if none; 127 for absmax = 0) */
int ina_scale_for_i8_sr(float absmax, int* k_out);
/* ina_block_scales_i8 under ina_scale_for_i8_sr's rule; rot: the rotation's stream, NULL for none */
int ina_block_scales_i8_sr(const void* const* xs, int xtype, int W, size_t n, int V, int8_t* kblk, const ina_sr_t* rot,
                           ina_stream_t stream);
/* (rotate under *rot +) quantise x to bytes under given scales, rounded stochastically under *rnd */
int ina_quantize_sr_i8_wire(const void* x, int xtype, const int8_t* kblk, int V, int8_t* q8, size_t n,
                            uint8_t* overflow_per_slot, const ina_sr_t* rot, const ina_sr_t* rnd, ina_stream_t stream);
/* the sum of G byte slices, each block rounded stochastically to bytes under shift[block] */
int ina_sum_i8_slices_requant_sr(const int8_t* const* slices, int G, int V, int8_t* q8, uint8_t* shift, size_t n,
                                 const ina_sr_t* rnd, ina_stream_t stream);

#include "ina_i4.h" /* a 4-bit wire word: packed nibbles, their exact and their requantising slice sums */

#endif /* INA_I8_SR_H */
