/*
 * ina_sr.h -- unbiased stochastic rounding for the quantisers and the int16 wire of a sharded bucket:
 * the stateless alternative to error feedback (ina_ef.h).  Included by ina.h (it needs ina_x16.h's type
 * codes); do not include it on its own.
 *
 * Every other quantiser rounds to nearest even, so a component that stays below half a quantum is
 * sent as zero on every step.  Error feedback answers that with an fp32 residual per bucket; it is
 * refused for 16-bit buckets on the wire calls and impossible where the rounding rank does not own
 * the values.  Here the quantiser rounds up with probability equal to the fraction it would drop:
 * no extra bytes move, no state is kept, bf16 / fp16 buckets are read as they are, and the random
 * word is a pure function of (seed, step, sub, element index), so every result can be replayed.
 *
 * Contract.  Per element e of a bucket, in fp32, unfused (a 16-bit x is widened exactly first; base,
 * where the call has one and it is not NULL, is subtracted with one rounding, as in ina_ef.h):
 *     t = d * 2^k                      d = x - base, or x
 *     f = floorf(t);  p = t - f        p == 0 once |t| >= 2^23
 *     u = float(word >> 8) * 2^-24     24 bits, in [0, 1)
 *     y = f + (u < p ? 1.0f : 0.0f)
 *     q = the sibling's clamp / NaN handling applied to y
 *   y stands where the round-to-nearest sibling has rintf(x * 2^k).  A NaN t gives y = NaN: q is 0,
 *     and on the int16 calls the slot flag / the wire word's saturation bit is set, as in the sibling.
 *     t = +-inf gives p = NaN, so y = +-inf and the value saturates as in the sibling.  Saturation, the
 *     slot flags (every slot written) and the wire word q16 + (sat << INA_I16_WIRE_SHIFT) are the
 *     siblings'.
 *   word comes from Philox4x32 with 10 rounds (Salmon et al., SC'11; the Random123 constants):
 *     multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85, the key bumped
 *     before rounds 2..10; one round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
 *     (hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0)).
 *     key     = (seed's low word, seed's high word)
 *     counter = (idx's low word, idx's high word, step, sub),  idx = (e0 + e) >> 2
 *     element e takes output word (e0 + e) & 3
 *   so one Philox call serves the 4 values a lane owns.  e0 is the bucket's offset in the stream of
 *   random words: a caller that quantises a slice x[lo:hi) of a bucket passes e0 = lo.
 * Consequences:
 *   Replay.  q, flags and wire words are bit for bit the replay of the lines above, whatever the
 *     grid, the alignment, or the vector or value-by-value path.
 *   Integers.  Where t is an integer, p is 0 and q equals the round-to-nearest sibling's for every
 *     seed.
 *   Slices.  Quantising x[lo:hi) with e0 = lo gives that slice of the whole-bucket result.
 *   Bias.  E[y] = t up to the 2^-24 grain of u.
 *
 * Argument checks: each function is its round-to-nearest sibling's argument list with `sr` before
 * `stream` (the first four also take `base` after x / xtype; it may be NULL).  The sibling's checks
 * come first, in its order and with its messages -- the type code on the x16 calls, k, V, the
 * n == 0 no-op, null pointers, a 16-bit pointer that is not 2-byte aligned -- then a null sr
 * ("null sr") and e0 % 4 != 0 ("e0 must be a multiple of 4": a lane's chunk never straddles two
 * Philox calls).  Each is INA_EINVAL before any device work.  *sr is copied into the kernel
 * arguments during the call, as ina_nga_params_t is.
 *
 * Layout: a lane owns 4 values -- one 16-byte access on the 32-bit side, one 8-byte access on the
 * 16-bit side.  The vector path needs fp32 / int32 buffers 16-byte aligned and 16-bit sources and
 * int16 outputs 8-byte aligned, and, for the slot flags, V with a ballot layout (V % 8 == 0, V / 8 a
 * power of two <= 64); any other alignment or V takes a value-by-value path with identical results.
 *
 * Not here: stochastic rounding combined with error feedback.  The worker packs of the packet path,
 * per-packet scales included, are in ina_pkt_sr.h; the fused quantise + reduce calls in ina_reduce_sr.h;
 * block scales on the bulk quantisers, the fused calls and the sharded wires in ina_blk_sr.h.
 */
#ifndef INA_SR_H
#define INA_SR_H

#ifndef INA_X16_H
#error "include ina.h, which includes ina_x16.h and ina_sr.h"
#endif

typedef struct ina_sr {
    uint64_t seed; /* the Philox key */
    uint64_t e0;   /* index of the bucket's first element in the random stream; a multiple of 4 */
    uint32_t step; /* counter word 2: the training step */
    uint32_t sub;  /* counter word 3: the stream within a step (the rank, the worker) */
} ina_sr_t;

/* ina_quantize_f32_i32 / ina_quantize_f32_i16_sat of x - base, rounded stochastically */
int ina_quantize_sr_f32_i32(const float* x, const float* base, int32_t* q, size_t n, int k, const ina_sr_t* sr,
                            ina_stream_t stream);
int ina_quantize_sr_f32_i16_sat(const float* x, const float* base, int16_t* q, size_t n, int k, int V,
                                uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream);
/* ina_quantize_x16_i32 / ina_quantize_x16_i16_sat: x is bf16 / fp16, widened in registers */
int ina_quantize_sr_x16_i32(const void* x, int xtype, const float* base, int32_t* q, size_t n, int k,
                            const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_sr_x16_i16_sat(const void* x, int xtype, const float* base, int16_t* q, size_t n, int k, int V,
                                uint8_t* overflow_per_slot, const ina_sr_t* sr, ina_stream_t stream);
/* ina_quantize_f32_i16_wire / ina_quantize_x16_i16_wire: the sharded int16 wire's words */
int ina_quantize_sr_f32_i16_wire(const float* x, int32_t* wire, size_t n, int k, const ina_sr_t* sr,
                                 ina_stream_t stream);
int ina_quantize_sr_x16_i16_wire(const void* x, int xtype, int32_t* wire, size_t n, int k, const ina_sr_t* sr,
                                 ina_stream_t stream);
/* ina_scale_for for stochastic rounding, which can round up by almost a whole quantum where nearest
 * rounds by half: the largest k in [-126, 127] with W * (absmax * 2^k + 1) <= 2^(bits-1) - 1, so
 * neither a value nor a W-way sum saturates.  Host only; ina_scale_for's refusals. */
int ina_scale_for_sr(float absmax, int W, int bits, int* k_out);

#endif /* INA_SR_H */
