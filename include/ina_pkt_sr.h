/*
 * ina_pkt_sr.h -- stochastic rounding (ina_sr.h) on the packet path: the fused worker packs, one
 * launch from the bucket to its NGA rows.  Included by ina.h directly after ina_sr.h; do not include
 * it on its own.
 *
 * Contract.  An SR pack writes, for element e of worker w's bucket, the payload word of
 *     q = q32_of(y)
 *   with y ina_sr.h's, computed in fp32, unfused, on
 *     t = (x[e] - base[e]) * 2^k         base may be NULL: t = x[e] * 2^k
 *   A 16-bit x is widened exactly first.  With per-packet scales k = kblk[e / V] under ina_blk.h's
 *   reading (-127 / -128 read as -126).  The random word is Philox4x32-10 under the key sr->seed at
 *   the counter ((sr->e0 + e) >> 2, sr->step, sr->sub + w), output word (sr->e0 + e) & 3: worker w of
 *   a multi-worker call takes stream sub + w (mod 2^32), a single-worker call is w = 0.
 *   Headers, descriptors, stride, the zero pad past n, the row layouts and the store policies are the
 *   round-to-nearest sibling's.  Pad words are 0 and draw nothing.
 * Consequences:
 *   Composition.  The rows equal the plain pack (ina_pack_nga_desc / ina_pack_nga_split) of
 *     ina_quantize_sr_{f32,x16}_i32 called with sub + w, bit for bit, whatever the grid, the pack
 *     kernel taken (flat, wave-per-packet at V = 256, byte path) or the number of pack groups.
 *   Workers.  One W-worker call equals W single-worker calls with sub + w, rows and descriptors.
 *   Integers.  Where every t is an integer, the rows are the nearest sibling's for every seed.
 *   Slices.  Packing x[lo:hi) with lo a multiple of V, e0 = lo and seq0 advanced by lo / V gives
 *     those packets of the whole bucket's call.
 *   Scales.  ina_block_scales_sr_f32 gives exactly ina_scale_for_sr(amax_s, degree, bits) per block
 *     (amax_s the block's max |x_w - base| over the workers, NaN skipped): ina_block_scales_f32's
 *     comparison with lim = (2^(bits-1) - 1) / degree - 1, so a degree-way sum of values that each
 *     may gain a whole quantum still fits.  INA_BLK_AUTO in the split pack computes the same scales
 *     in its own launch and writes them to kblk.
 *
 * Argument checks: each function is its sibling's argument list with `sr` before `stream`
 * (ina_block_scales_sr_f32 is its sibling's: it draws nothing).  The sibling's checks come first, in
 * its order and with its messages, the n == 0 no-op where the sibling has it; then a null sr ("null
 * sr") and sr->e0 % 4 != 0 ("e0 must be a multiple of 4").  Each is INA_EINVAL before any device
 * work.  ina_block_scales_sr_f32 and INA_BLK_AUTO refuse what ina_scale_for_sr refuses (degree < 1, a
 * width other than 16 / 32, a degree that leaves no room).  AUTO outside V a power of two in [8, 256]
 * and W <= 8 runs ina_block_scales_sr_f32 first and then the GIVEN kernels, as the sibling does:
 * identical scales and rows.  *sr is copied into the kernel arguments during the call.
 *
 * Not here: 16-bit buckets with block scales, stochastic rounding combined with error feedback and the
 * packed-row multi-worker pack (ina_quantize_pack_nga_multi).  The fused quantise + reduce calls are in
 * ina_reduce_sr.h.
 */
#ifndef INA_PKT_SR_H
#define INA_PKT_SR_H

#ifndef INA_SR_H
#error "include ina.h, which includes ina_sr.h and ina_pkt_sr.h"
#endif

/* one worker, packed rows: ina_quantize_pack_nga_desc / _x16_desc / _blk_desc (scales given) */
int ina_quantize_pack_nga_sr_desc(const float* x, const float* base, size_t n, int k,
                                  const ina_nga_params_t* prm, uint8_t* pkts, size_t stride,
                                  ina_nga_desc_t* desc, const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_pack_nga_x16_sr_desc(const void* x, int xtype, const float* base, size_t n, int k,
                                      const ina_nga_params_t* prm, uint8_t* pkts, size_t stride,
                                      ina_nga_desc_t* desc, const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_pack_nga_blk_sr_desc(const float* x, const float* base, size_t n, const int8_t* kblk,
                                      const ina_nga_params_t* prm, uint8_t* pkts, size_t stride,
                                      ina_nga_desc_t* desc, const ina_sr_t* sr, ina_stream_t stream);
/* W workers in one launch into split rows: ina_quantize_pack_nga_multi_split / _x16 / _blk (mode
 * INA_BLK_GIVEN reads kblk, INA_BLK_AUTO writes it); worker w draws from stream sr->sub + w */
int ina_quantize_pack_nga_multi_split_sr(const float* const* x, int W, const float* base, size_t n, int k,
                                         const ina_nga_params_t* prm, uint8_t* const* hdr,
                                         uint8_t* const* pay, ina_nga_desc_t* const* desc,
                                         const ina_sr_t* sr, ina_stream_t stream);
int ina_quantize_pack_nga_multi_split_x16_sr(const void* const* x, int xtype, int W, const float* base,
                                             size_t n, int k, const ina_nga_params_t* prm,
                                             uint8_t* const* hdr, uint8_t* const* pay,
                                             ina_nga_desc_t* const* desc, const ina_sr_t* sr,
                                             ina_stream_t stream);
int ina_quantize_pack_nga_multi_split_blk_sr(const float* const* x, int W, const float* base, size_t n,
                                             int8_t* kblk, int mode, int degree, const ina_nga_params_t* prm,
                                             uint8_t* const* hdr, uint8_t* const* pay,
                                             ina_nga_desc_t* const* desc, const ina_sr_t* sr,
                                             ina_stream_t stream);
/* ina_block_scales_f32 under ina_scale_for_sr's rule */
int ina_block_scales_sr_f32(const float* const* xs, int W, const float* base, size_t n, int V,
                            int degree, int bits, int8_t* kblk, ina_stream_t stream);

#endif /* INA_PKT_SR_H */
