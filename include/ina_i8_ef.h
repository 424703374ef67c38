/*
 * ina_i8_ef.h -- error feedback on the 8-bit wire of ina_i8.h: a rank keeps what its byte quantiser dropped and
 * adds it to its next bucket.  The rounding error lives in the rotated domain, whose signs change every step,
 * so it goes back through the inverse rotation before it is kept: the residual is in the gradient's own domain,
 * fp32, rank-local, and never travels.  Included by ina.h through ina_rot.h, ina_i8.h and ina_i8_gather.h, whose
 * last line includes this header; do not include it on its own.
 *
 * Built from the existing calls the step is add -> ina_quantize_i8_wire -> widen the rank's own bytes ->
 * ina_dequantize_rot_i16 -> subtract: 38 bytes a value of memory traffic in five launches, and three bucket-sized
 * temporaries.  ina_quantize_ef_i8_wire runs the forward rotation, the quantiser and the inverse rotation of the
 * error in the same lanes of one launch: 4 + 4 + 1 + 4 = 13 bytes a value for an fp32 bucket (11 for bf16 /
 * fp16), no temporaries.  Nothing on the links changes: the bytes, the MIN of the scales, the slice sum and both
 * decodes are ina_i8.h's and ina_i8_gather.h's.
 *
 * Contract.  V, the blocks, xtype, sr, the alignment and the order of refusals are ina_i8.h's.  resid is fp32 for
 * every source type, n values, 16-byte aligned, updated in place, and must not overlap x or q8.  Per element,
 * fp32, unfused, round to nearest even:
 *     v      = widen(x) + resid
 *     r      = sr ? ina_rot.h's forward rotation of the block of v (same signs, stage order, 2^-ceil(m/2)) : v
 *     q8     = clamp(rne(r * 2^k), -127, 127), NaN -> 0      (ina_quantize_i8_wire on v; the same flag)
 *     d      = isfinite(r) ? r - float(q8) * 2^-k : +0.0f    (2^-k is exact; a clamped finite r carries the
 *                                                             clipped part)
 *     u      = sr ? ina_rot.h's inverse of the block of d (same stages, 2^-floor(m/2), then sigma) : d
 *     resid' = isfinite(u) ? u : +0.0f
 *   ina_block_scales_i8_ef.  kblk[s] = ina_scale_for_i8(max |r| of block s over the W pairs), r built from
 *     v = xs[w] + resids[w] as above.  It writes only kblk.  Ranks take the MIN of their scales before they
 *     quantise, as in ina_i8.h.
 *   ina_quantize_ef_i8_wire.  The scales are given (-127 and -128 are read as -126).  It writes q8, the flags
 *     (overflow_per_slot may be NULL) and resid' in one launch.
 * Consequences.
 *   Replay.  Every q8, flag, scale and resid' is bit for bit the fp32 replay of the lines above.
 *   Zero residual.  With resid all zero, the scales, bytes and flags equal ina_block_scales_i8's and
 *     ina_quantize_i8_wire's on the same input bit for bit (x + 0 = x; -0 becomes +0, which no byte, flag or
 *     scale can tell).
 *   A bad block heals.  With sr != NULL a NaN or +-inf in a block makes every r of the block NaN or inf, so the
 *     whole block's d, u and residual are zero; with sr == NULL only that element's residual is zero.  A finite
 *     block whose inverse butterfly overflows loses the residual of the values that came out NaN or inf, and
 *     nothing else.
 *   The sum is kept.  With xhat_t the decode of a rank's own bytes at step t, sum_t xhat_t + resid_T = T * x up
 *     to fp32 rounding for a constant bucket x: the mean of the decodes is off by resid_T / T.
 *
 * Arguments.  As in ina_i8.h, and resid / every resids[w] 16-byte aligned.  Refused with INA_EINVAL, by name and
 * before any device work, in this order: a bad xtype; V not a power of two in [8, 256]; a null kblk; n not a
 * multiple of V; (n == 0 is a no-op;) W outside [1, INA_MAX_WORKERS] or null pointers (x, q8, xs or one of its
 * buckets); a null resid (resids or one of its entries); a buffer that is not 16-byte aligned; with sr != NULL,
 * sr->e0 not a multiple of 128 and of V.  *sr is copied into the kernel arguments during the call.
 *
 * Layout.  ina_rot.h's lanes: a lane owns 4 values, a block is V/4 adjacent lanes of one wave.  The quantiser
 * lane loads its chunk of x and of resid, adds them, takes the wave's signs once from the scalar unit and keeps
 * its masks, runs the forward butterfly, quantises and packs as ina_quantize_i8_wire does and stores one dword
 * of bytes, forms d in registers, runs the same stages again as the inverse with the kept masks, and stores 16
 * bytes of resid'.  Nothing goes through LDS or memory between the two butterflies.  sr == NULL is an arm of
 * its own with no butterfly and no signs.  The scales kernel is ina_block_scales_i8's with a second pointer
 * pack and the add in front.  Every grid is under the default cap (ina_set_tuning key 0).
 *
 * Not here: stochastic rounding on this wire, scales computed in the quantiser's launch (an AUTO mode), a base,
 * error feedback on the requantised gather's second rounding, layout B, the packet path, and bench.py.
 * (Stochastic rounding on both halves of the wire, the second rounding included, has since come in
 * ina_i8_sr.h, which this header includes as its last line; combined with error feedback it is still not here.)
 */
#ifndef INA_I8_EF_H
#define INA_I8_EF_H

#ifndef INA_I8_GATHER_H
#error "include ina.h, which includes ina_rot.h, ina_i8.h, ina_i8_gather.h and ina_i8_ef.h"
#endif

/* the scales of the byte wire over xs[w] + resids[w]: kblk[s] = ina_scale_for_i8(max |r| of block s) */
int ina_block_scales_i8_ef(const void* const* xs, const float* const* resids, int xtype, int W, size_t n, int V,
                           int8_t* kblk, const ina_sr_t* sr, ina_stream_t stream);
/* (rotate +) quantise x + resid to bytes under given scales; resid becomes the (inverse-rotated) rounding error */
int ina_quantize_ef_i8_wire(const void* x, int xtype, float* resid, const int8_t* kblk, int V, int8_t* q8, size_t n,
                            uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream);

#include "ina_i8_sr.h" /* stochastic rounding on the byte wire: the quantiser and the requantised gather */

#endif /* INA_I8_EF_H */
