/*
 * rdo_ptq_mxround.h -- C ABI of librdoptq_hip.so, continued: learned rounding (AdaRound) on the grids of the OCP microscaling (MX)
 * block formats of rdo_ptq_mx.h (csrc/mx_round.hip).  Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as
 * void*, integer status codes; every entry records into a plan); a header of its own because the export tables of rdo_ptq_hip.h and
 * rdo_ptq_mx.h are closed (their symbol sets are pinned by the suite).
 *
 * A weight is its row matrix [rows][inner] cut into blocks of RDO_MX_BLOCK elements exactly as in rdo_ptq_mx.h.  The block scale
 * X = 2^E is the one rdo_mx_fakequant derives from the block's amax of the ORIGINAL weight; learned rounding never moves a scale.
 * The grid of a block is {+-mag * X} over the format's representable magnitudes, ordered on the real line, -0 == 0.  Per element w:
 *   lo   the largest grid value <= w,  hi the smallest grid value > w,  gap = hi - lo > 0      (all exactly representable in fp32)
 *        an exact power-of-two magnitude on the negative side takes the spacing of the binade below it; w = 0 and every element of
 *        an all-zero block: lo = 0, gap = smallest subnormal * X
 *   pinned  w >= max * X or w < -max * X (where round to nearest saturates): lo = +-max * X, gap = 0.  A pinned element does not exist
 *        for the optimiser: its alpha, m and v are never written, it adds nothing to the rounding loss, its soft and hard weight is lo
 *   a block that holds a NaN or an infinity: lo = NaN, gap = 0 (inputs are meant to be finite)
 *   soft weight  w~ = lo + gap * h(alpha),  h = clamp(1.2 sigmoid(alpha) - 0.1, 0, 1); no level clamp: hi is always on the grid.
 *        A GDN gamma (reparam) then goes through max(w~, bound)^2 - pedestal, as in rdo_adaround_step
 *   hard weight  lo + gap * (alpha >= 0)
 *   init  rest = (w - lo) / gap in fp32,  alpha0 = -log(1.2 / (rest + 0.1) - 1): hard(alpha0) is rdo_mx_fakequant's wq on every
 *        element that is neither pinned nor an exact tie; exact ties go up (alpha0 = 0) where the format kernel goes to the even mantissa
 */
#ifndef RDO_PTQ_MXROUND_H
#define RDO_PTQ_MXROUND_H
#include "rdo_ptq_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lo, gap fp32 [rows][inner] of w fp32 [rows][inner] in `format`; scales (nullable) uint8 [rows][ceil(inner / 32)]: the bytes
 * rdo_mx_fakequant writes.  Integer arithmetic on the fp32 bit pattern.
 * RDO_EINVAL for a NULL w / lo / gap, rows <= 0, inner <= 0, more than 2^40 blocks, an unknown format, w / lo / gap not 4-byte aligned. */
int rdo_mx_neighbours(const float* w, int32_t rows, int64_t inner, int32_t format, float* lo, float* gap, uint8_t* scales, void* stream);

/* alpha0 of numel elements from w and their neighbours; a pinned element (gap == 0) gets alpha = 0.
 * RDO_EINVAL for a NULL or misaligned pointer, numel <= 0. */
int rdo_mx_round_init_alpha(const float* w, const float* lo, const float* gap, int64_t numel, float* alpha, void* stream);

/* Soft (soft != 0) or hard weight into the layouts of rdo_adaround_fwd: wq as the weight, wd (nullable) the dgrad layout from
 * d->KH / KW / Cin (the transpose for a gamma), d->reparam honoured; d->n_levels is ignored.
 * With soft == 0 and codes (uint8 [rows][inner]) given it also writes the element codes of the hard weight under the block scales
 * scales_in (uint8 [rows][ceil(inner / 32)], needed with codes): rdo_mx_dequant(codes, scales_in) is the hard weight before any reparam
 * bit for bit (codes describe the stored weight).  The codes of a block whose scale code is 255 are unspecified.
 * RDO_EINVAL for a NULL d / lo / gap / alpha / wq, a descriptor whose numel, rows or conv layout do not fit, an unknown format,
 * misaligned fp32 pointers, codes with soft != 0, codes without scales_in. */
int rdo_mx_round_fwd(const rdo_ada_desc* d, const float* lo, const float* gap, const float* alpha, int32_t soft, float* wq, float* wd,
                     uint8_t* codes, const uint8_t* scales_in, int32_t format, void* stream);

/* The fused step on an MX grid: reduce the nsplit gradient slabs [nsplit][numel] -> reparam LowerBound backward -> g * gap * h'
 * -> + the rounding regulariser's gradient -> Adam(beta1 .9, beta2 .999, eps 1e-8) on alpha -> the next soft wq (and wd, nullable, by a
 * second launch).  The arithmetic and the accumulation contract of rdo_adaround_step's flat form with per-element delta = gap and no
 * level clamp: weight * sum(1 - |2h - 1|^b) of the CURRENT alpha over the non-pinned elements goes into
 * round_loss_out[*iter_ptr][slot] (atomicAdd; nullable); the counter is read, never moved.  d->n_levels is ignored.  No plane outputs.
 * RDO_EINVAL for a NULL pointer (wd and round_loss_out may be NULL), a descriptor that does not fit, nsplit < 1, misaligned fp32
 * pointers. */
int rdo_mx_round_step(const rdo_ada_desc* d, const float* lo, const float* gap, const float* slabs, int32_t nsplit, float grad_scale,
                      float round_weight, const rdo_sched_row* sched, const int32_t* iter_ptr, float* alpha, float* adam_m, float* adam_v,
                      float* wq, float* wd, float* round_loss_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXROUND_H */
