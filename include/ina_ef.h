/*
 * ina_ef.h -- error feedback for the quantiser: the worker keeps what rounding dropped and adds it
 * to the next step's gradient, in the quantiser's own launch.  Included by ina.h (it needs
 * ina_x16.h's type codes, ina_blk.h's modes and the packet types); do not include it on its own.
 *
 * Every other quantising entry point rounds a gradient to the integer wire and discards the
 * remainder, so a component that stays below half a quantum is sent as zero on every step.  Here a
 * worker owns one fp32 residual buffer `resid` of n values per bucket.  It starts at zero and every
 * call updates it in place, so the sum of what was sent tracks the sum of what was meant to be
 * sent.  The switch, the PS and the wire format are untouched: the aggregator adds plain integers.
 *
 * Contract.  Per element, in fp32, unfused:
 *     d  = base ? x - base : x          (x widened exactly first if it is bf16 / fp16)
 *     v  = d + r
 *     q  = Q(v, k)                      the sibling's quantiser, its saturation and its slot flag
 *     r' = isfinite(v) ? v - float(q) * 2^-k : +0.0f
 *   float(q) * 2^-k is the sibling dequantiser's arithmetic, 2^-k built exactly (k = 127 gives the
 *     subnormal 2^-127).
 *   A NaN or +-inf v quantises as the sibling does (0, or saturated with the flag) and leaves a
 *     zero residual, so one bad step does not poison the bucket.
 *   A finite v that saturates carries the clipped part forward.
 *   A lane reads its r before it writes r', so the update is in place.  resid is fp32 for every
 *     source type and must not overlap x, base or q.
 *   With block scales, k is kblk[block] under the contract of ina_blk.h (blocks, -127 / -128 read
 *     as -126, short last block).  Computed scales are ina_scale_for(amax_s, degree, bits) with
 *     amax_s taken over |v|, not |x|.
 * Two consequences:
 *   Replay.  q is the sibling's quantiser applied to v, and v and r' are the three fp32 operations
 *     above: every result (q, r', flags, scales, packet rows) is bit for bit that replay.
 *   Zero residual.  With resid all zero every q, flag, scale and packet row equals the non-EF
 *     sibling's on the same input bit for bit (d + 0 is d up to the sign of zero).
 *
 * Argument checks, their order and messages, the n == 0 no-op and the return codes follow each
 * sibling; a null resid is INA_EINVAL; every check happens before any device work.  16-byte aligned
 * fp32 / int32 buffers (8-byte aligned 16-bit sources and int16 outputs) take the vector path: 4
 * values per lane, r and r' always 16-byte accesses.  Any other alignment, or a V without a ballot
 * layout, takes a slower path with identical results.  The packs need their buffers 16-byte
 * aligned, as their siblings do.
 *
 * Not here: the fused quantise + reduce calls (their W residuals belong to workers that share the
 * GPU), the packed-row multi-worker pack, 16-bit sources on the block-scaled and pack calls, the
 * switch and the PS, which only see integers.  The sharded int16 wire's quantisers are in
 * ina_shard_ef.h.
 */
#ifndef INA_EF_H
#define INA_EF_H

#ifndef INA_SHARD_BLK_H
#error "include ina.h, which includes ina_ef.h"
#endif

/* ina_quantize_f32_i32 / ina_quantize_f32_i16_sat on v = (x - base) + resid; base may be NULL */
int ina_quantize_ef_f32_i32(const float* x, const float* base, float* resid, int32_t* q, size_t n, int k,
                            ina_stream_t stream);
int ina_quantize_ef_f32_i16_sat(const float* x, const float* base, float* resid, int16_t* q, size_t n, int k,
                                int V, uint8_t* overflow_per_slot, ina_stream_t stream);
/* ina_quantize_x16_i32 / ina_quantize_x16_i16_sat: x is bf16 / fp16, widened in registers */
int ina_quantize_ef_x16_i32(const void* x, int xtype, const float* base, float* resid, int32_t* q, size_t n,
                            int k, ina_stream_t stream);
int ina_quantize_ef_x16_i16_sat(const void* x, int xtype, const float* base, float* resid, int16_t* q,
                                size_t n, int k, int V, uint8_t* overflow_per_slot, ina_stream_t stream);
/* ina_block_scales_f32 over |(xs[w] - base) + resids[w]|: what workers agree on (MIN) before a
 * GIVEN call.  Nothing is written but kblk. */
int ina_block_scales_ef_f32(const float* const* xs, const float* const* resids, int W, const float* base,
                            size_t n, int V, int degree, int bits, int8_t* kblk, ina_stream_t stream);
/* ina_quantize_blk_f32_i32 / ina_quantize_blk_f32_i16_sat.  mode INA_BLK_GIVEN reads kblk;
 * INA_BLK_AUTO computes it from this call's v in the same launch (bits = the width of q) and
 * writes it.  degree is ignored when the scales are given. */
int ina_quantize_ef_blk_f32_i32(const float* x, const float* base, float* resid, int8_t* kblk, int mode,
                                int degree, int V, int32_t* q, size_t n, ina_stream_t stream);
int ina_quantize_ef_blk_f32_i16_sat(const float* x, const float* base, float* resid, int8_t* kblk, int mode,
                                    int degree, int V, int16_t* q, size_t n, uint8_t* overflow_per_slot,
                                    ina_stream_t stream);
/* ina_quantize_pack_nga_multi_split / ina_quantize_pack_nga_multi_split_blk with worker w's
 * residual resid[w] (a host array of W device pointers, each 16-byte aligned).  AUTO runs in the
 * pack's own launch for V a power of two in [8, 256] and W <= 8, else ina_block_scales_ef_f32 first
 * and the GIVEN pack. */
int ina_quantize_pack_nga_multi_split_ef(const float* const* x, float* const* resid, int W, const float* base,
                                         size_t n, int k, const ina_nga_params_t* prm, uint8_t* const* hdr,
                                         uint8_t* const* pay, ina_nga_desc_t* const* desc,
                                         ina_stream_t stream);
int ina_quantize_pack_nga_multi_split_ef_blk(const float* const* x, float* const* resid, int W,
                                             const float* base, size_t n, int8_t* kblk, int mode, int degree,
                                             const ina_nga_params_t* prm, uint8_t* const* hdr,
                                             uint8_t* const* pay, ina_nga_desc_t* const* desc,
                                             ina_stream_t stream);

#endif /* INA_EF_H */
