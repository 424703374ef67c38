/*
 * ina_switch_blk.h -- per-block scales in the fused switch + PS step.
 * Included by ina.h after ina_pkt_blk.h (and after the switch's own types), whose contract holds
 * here; do not include it on its own.
 *
 * ina_switch with a PS step, with 2^-kblk[slot] in place of 2^-k: a completed slot's sum goes from
 * the switch's registers straight into
 *     out[slot*V + j] = local[slot*V + j] + (float(sum) * 2^-kblk[slot]) * float(weight_step),
 * slot = frag_id - seq0, slot < ceil(n / V), slot*V + j < n -- the sibling's unfused fp32 sequence.
 * The block is the packet (ina_pkt_blk.h): kblk[s] is the exponent the workers packed slot s with.
 *
 *   kblk holds ceil(ps->n / V) device bytes.  Byte s is read only for a consumed packet: one that
 *     completes its slot with frag_id - seq0 == s inside the bucket.  A given -127 / -128 is read as
 *     -126.  ps->k is ignored; ina_switch_ps_t is the sibling's struct, field for field.
 *   Results: ina_switch without a PS step followed by ina_apply_completed_nga_blk, bit for bit --
 *     actions, registers, the rows written (or left as they arrived, keep_forwarded = 0), the ack
 *     rows and their descriptors; the same equality ina_switch's PS step keeps with its own
 *     two-call form.  Ack rows and descriptors do not depend on the scales.
 *   Checks: ps == NULL or kblk == NULL is INA_EINVAL in every phase (this entry point is the PS
 *     step); everything ina_switch checks for a PS step is checked here, in its order and with its
 *     messages, before the switch touches its state; npkts == 0 is a no-op.
 *   Phases: ina_switch's.  The sort reads neither ps nor kblk, and the sort / run pairing record
 *     and its refusals are the sibling's: INA_SWITCH_SORT through either entry point followed by
 *     INA_SWITCH_RUN through this one is valid.
 *
 * fp32 local and out.  Every layout ina_switch's PS step takes: packed and split rows, with and
 * without descriptors, every batch size.
 */
#ifndef INA_SWITCH_BLK_H
#define INA_SWITCH_BLK_H

#ifndef INA_PKT_BLK_H
#error "include ina.h, which includes ina_pkt_blk.h and ina_switch_blk.h"
#endif

int ina_switch_blk(const ina_switch_state_t* st, const ina_switch_batch_t* batch,
                   const ina_switch_ps_t* ps, const int8_t* kblk, int phase, ina_stream_t stream);

#endif /* INA_SWITCH_BLK_H */
