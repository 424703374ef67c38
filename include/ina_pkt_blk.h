/*
 * ina_pkt_blk.h -- per-block scales on the packet path: the worker packs and the PS apply.
 * Included by ina.h after ina_blk.h, whose contract holds here; do not include it on its own.
 *
 * On the packet path the block is the packet: one NGA-V payload is V consecutive values, one
 * slot, so kblk[p] is packet p's exponent and nblk = npkts = ceil(n / V).  ngaa_h has no exponent
 * field: the scales travel beside the packets, one int8 per packet (1/(4V) of the payload), and
 * workers agree on them before they pack (MIN across workers).  The switch adds integers and is
 * not involved.
 *
 *   Packs.  Packet p's payload is quantised with 2^kblk[p]; headers, descriptors, layouts and the
 *     zero tail of a short last packet are the global-k sibling's, so a packet's bytes are the
 *     sibling's on that packet alone with k = kblk[p].  A given -127 / -128 is read as -126.
 *   AUTO (the multi-worker split pack).  kblk[p] = ina_scale_for(amax_p, degree, 32) with amax_p the
 *     max over these W workers of |x[w][i] - base[i]| in packet p, as ina_block_scales_f32 computes
 *     it; it is written to kblk and the rows are the GIVEN rows for it.  V a power of two in
 *     [8, 256] with W <= 8 computes it in the pack's own launch from registers (each bucket read
 *     once); any other V or W runs ina_block_scales_f32 first, then the GIVEN pack.
 *   Apply.  ina_apply_completed_nga with 2^-kblk[slot] in place of 2^-k, slot = frag_id - seq0:
 *     out = local + (float(sum) * 2^-kblk[slot]) * float(weight_step), the sibling's unfused fp32
 *     sequence; ack rows as the sibling writes them.
 *
 * fp32 sources only.  Argument checks, return codes and the n == 0 no-op follow each sibling;
 * mode and degree are checked before any device work.
 */
#ifndef INA_PKT_BLK_H
#define INA_PKT_BLK_H

#ifndef INA_BLK_H
#error "include ina.h, which includes ina_blk.h and ina_pkt_blk.h"
#endif

/* one worker, packed rows, scales given: ina_quantize_pack_nga_desc with kblk[p] for k */
int ina_quantize_pack_nga_blk_desc(const float* x, const float* base, size_t n, const int8_t* kblk,
                                   const ina_nga_params_t* prm, uint8_t* pkts, size_t stride,
                                   ina_nga_desc_t* desc, ina_stream_t stream);
/* W workers in one launch into split rows: ina_quantize_pack_nga_multi_split.  mode INA_BLK_GIVEN
 * reads kblk; INA_BLK_AUTO computes it from these W deltas for `degree` summands at 32 bits and
 * writes it.  degree is ignored when the scales are given. */
int ina_quantize_pack_nga_multi_split_blk(const float* const* x, int W, const float* base, size_t n,
                                          int8_t* kblk, int mode, int degree, const ina_nga_params_t* prm,
                                          uint8_t* const* hdr, uint8_t* const* pay,
                                          ina_nga_desc_t* const* desc, ina_stream_t stream);
/* PS: ina_apply_completed_nga with kblk[slot] for k.  pay == NULL: rows are packed rows of `stride`
 * bytes.  Otherwise split rows (ina_switch_batch_t's convention): rows = 16-byte header rows
 * (stride 16), pay = 4V-byte payload rows. */
int ina_apply_completed_nga_blk(const uint8_t* rows, const uint8_t* pay, size_t npkts, int V, size_t stride,
                                const uint8_t* actions, uint32_t seq0, const float* local,
                                const int8_t* kblk, double weight_step, float* out, size_t n,
                                uint8_t* acks, size_t ack_stride, ina_stream_t stream);

#endif /* INA_PKT_BLK_H */
