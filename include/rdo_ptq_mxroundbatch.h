/*
 * rdo_ptq_mxroundbatch.h -- C ABI of librdoptq_hip.so, continued: the learned-rounding step of rdo_ptq_mxround.h for every weight tensor
 * of a unit in one launch, planes, counter hand-over and the next mini-batch included (csrc/mx_round_batch.hip).  Same conventions as
 * rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status codes; the entry records into a plan); a header of its
 * own because the export table of rdo_ptq_mxround.h is closed (its symbol set is pinned by the suite).
 *
 * What the integer grids have in the batched AdaRound step of rdo_ptq_hip.h (items of type rdo_ada_step_item), on the MX grids: per
 * tensor the arithmetic, the slab order and the rounding-loss contract of the single-tensor MX step of rdo_ptq_mxround.h, bit for bit,
 * and per tensor the plane outputs that the split entries of rdo_ptq_hip.h would make of the new weights, bit for bit and in their
 * fragment orders.  Two launches: the step, then the dgrad layouts.
 */
#ifndef RDO_PTQ_MXROUNDBATCH_H
#define RDO_PTQ_MXROUNDBATCH_H
#include "rdo_ptq_mxround.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One weight tensor of the unit: rdo_ada_step_item with lo, gap (rdo_ptq_mxround.h) in place of w, delta, zp, and no dalpha.
 * d->n_levels is ignored.  numel % 4 == 0; lo, gap, slabs, alpha, adam_m, adam_v and wq are read and written 16 bytes at a time. */
typedef struct rdo_mx_round_step_item {
    rdo_ada_desc d;
    const float *lo, *gap, *slabs /* [nsplit][numel] */;
    int32_t nsplit;
    float *alpha, *adam_m, *adam_v, *wq, *wd /* nullable: the dgrad layout from d.KH / KW / Cin (the transpose for a gamma) */;
    /* nullable: the planes of the new wq [rows][KH][KW][Cin] and of wd [Cin][KH][KW][rows] in the conv kernels' fragment order.  plane
     * scale 0: 3 x numel bf16, the exact three-way split; > 0 (a power of two): 2 x numel fp16, the two-way split of w * scale, and a
     * value beyond fp16's range raises the bound overflow word as the fp16 conv split entry does.  wd_planes needs wd. */
    void *wq_planes, *wd_planes;
    float wq_plane_scale, wd_plane_scale;
    /* nullable: fp16 two-way planes of wq [rows][inner] * lin_plane_scale in the fragment order of the split-fp16 Linear kernel, and of
     * its transpose; they raise no overflow word (the Linear split entry raises none).  A 1 x 1 layout (d.KH == d.KW == 1) with rows and
     * inner multiples of 32, lin_plane_scale > 0. */
    void *lin_fwd_planes, *lin_bwd_planes;
    float lin_plane_scale;
} rdo_mx_round_step_item;

/* The fused step of n <= 8 tensors in one launch, and their dgrad layouts (wd, wd_planes, lin_bwd_planes) in a second one.
 *   round_loss_out (nullable): weight * sum(1 - |2h - 1|^b) of the CURRENT alpha over the non-pinned elements of every tensor goes into
 *       round_loss_out[*iter_ptr][slot] (atomicAdd), while the schedule row has round_on != 0.
 *   Counter: the step launch only reads *iter_ptr.  advance_iter (nullable): incremented by the SECOND launch, which reads no counter.
 *       iter_shadow (nullable, the alternative; must not be iter_ptr): the first thread of the step launch stores *iter_ptr + 1 there.
 *       No thread reads a word that another thread of the same launch writes.
 *   next (nullable): extra workgroups behind the step's own assemble the mini-batch of iteration *iter_ptr + 1 (gather + QDrop, fp32
 *       and / or H2 planes, as the stand-alone gather entries of rdo_ptq_hip.h do bit for bit); skipped when row *iter_ptr + 1 of
 *       idx_table does not exist.
 * Pinned elements (gap == 0) keep alpha, adam_m and adam_v untouched, their weight is lo (through d.reparam).
 * RDO_EINVAL, before anything is launched, for: NULL items, sched or iter_ptr; n outside 1 .. 8; an item whose descriptor does not fit,
 * whose numel is no multiple of 4, with a NULL lo / gap / slabs / alpha / adam_m / adam_v / wq or nsplit < 1; a misaligned pointer (16
 * bytes for the seven fp32 streams, 8 for planes, 4 for the rest; wd 16 when rows % 4 == 0); a negative or non-finite plane scale;
 * wd_planes without wd; wd or lin planes on a descriptor without a conv layout (d.Cin == 0); lin planes with rows or inner not a
 * multiple of 32, KH * KW != 1 or lin_plane_scale <= 0; both advance_iter and iter_shadow; iter_shadow == iter_ptr; a gather
 * descriptor that the batched AdaRound gather entry of rdo_ptq_hip.h would refuse. */
int rdo_mx_round_step_batch(const rdo_mx_round_step_item* items, int32_t n, float grad_scale, float round_weight, const rdo_sched_row* sched,
                            const int32_t* iter_ptr, float* round_loss_out, int32_t* advance_iter, int32_t* iter_shadow,
                            const rdo_gather_desc* next, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXROUNDBATCH_H */
