/*
 * rdo_ptq_subpel.h -- C ABI of librdoptq_hip.so, continued: the r = 2 pixel shuffle of a sub-pixel conv (and its inverse in the backward
 * pass) folded into the stores of the kernels that produce the tensor, instead of a launch of its own per tensor.
 * Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status codes); a header of its own because
 * the export table of rdo_ptq_hip.h is closed (its symbol count is pinned by the suite).
 *
 * Rows in 4 groups.  pixel_shuffle(r = 2) sends conv output channel 4 c + g (g = 2 i + j) of pixel (h, w) to channel c of pixel
 * (2 h + i, 2 w + j).  The plane kernels hold 4 consecutive channels per lane and 16 per H2 record, so with the weight's own row order a
 * record of the shuffled tensor would have to be collected from 16 lanes.  A sub-pixel conv whose weight PLANES carry logical row
 * 4 c + g at row g * C + c (C = Cout / 4) has every tile of output channels inside one group g, and the shuffle becomes an address change
 * of whole records.  Only the planes and the weight-gradient slabs of such a conv are in group order; w, alpha, the Adam moments, delta,
 * zero point and the fp32 soft weights keep the logical order everywhere.
 */
#ifndef RDO_PTQ_SUBPEL_H
#define RDO_PTQ_SUBPEL_H
#include "rdo_ptq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rdo_conv2d_fwd_h2 with a store mode: 0 plain (the same launch), 1 shuffle, 2 unshuffle.  The loads of the epilogue -- bias, aux,
 * aux_planes, residual -- keep the conv's own [B][Ho][Wo][Cout] index; only out / out_planes are written elsewhere:
 *   1: wplanes (and bias) with the rows in 4 groups; output element (b, h, w, n), g = n / C, goes to [B][2Ho][2Wo][C] at
 *      (b, 2 h + (g >> 1), 2 w + (g & 1), n - g C)                       = pixel_shuffle of the logically ordered conv
 *   2: output element (b, y, x, n) goes to [B][Ho/2][Wo/2][4 Cout] at (b, y >> 1, x >> 1, n + (2 (y & 1) + (x & 1)) Cout)
 *                                                                         = pixel_unshuffle with its channels in group order
 * `pre` must be NULL with a store mode.  rdo_conv2d_fwd_h2_px_supported: the shape is on the plane path, r = 2 geometry holds (mode 1:
 * Cout % 4 == 0, (Cout / 4) % 16 == 0 and the output-channel tile of the launch the shape takes divides Cout / 4; mode 2: Ho and Wo
 * even) and that launch is one that knows the remap (the 32-channel-stage halo kernel, direct or split over K); 0 otherwise. */
int rdo_conv2d_fwd_h2_px_supported(const rdo_conv_desc* d, int32_t store_mode);
int rdo_conv2d_fwd_h2_px(const rdo_conv_desc* d, const void* x_planes, float x_scale, const void* wplanes, float w_scale, const float* bias,
                         const float* aux, const void* aux_planes, const float* residual, float* out, float* pre, void* out_planes,
                         float out_scale, float* workspace, int64_t workspace_floats, int32_t store_mode, void* stream);

/* rdo_split_h2_conv with row_groups 0 (the same launch) or 4: the planes of logical row r are written at row (r & 3) Cout / 4 + (r >> 2). */
int rdo_split_h2_conv_px(const float* w, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin, float scale, void* planes, int32_t row_groups,
                         void* stream);

/* rdo_gdn_fwd_bwd whose dL/dout leaves the launch as H2 planes in unshuffle order instead of as fp32: the tokens are the pixels of
 * [B][H][W] (per_image = H W C), dup_planes the planes of [B][H/2][W/2][4 C] times dup_scale (a power of two), token (b, y, x) channel n
 * at (b, y >> 1, x >> 1, n + (2 (y & 1) + (x & 1)) C) -- rdo_pixel_unshuffle2 of grad_out with its channels in group order.  Every other
 * output as rdo_gdn_fwd_bwd.  dup_overflow_flag: the overflow words dup_planes raise (NULL: the bound ones, rdo_h2_bind_flag; dx_planes
 * always raise the bound ones).  _supported: what rdo_gdn_fwd_bwd_supported asks, H and W even, M = B H W for a whole number of images. */
int rdo_gdn_fwd_bwd_px_supported(int64_t M, int32_t C, int32_t H, int32_t W);
int rdo_gdn_fwd_bwd_px(const float* c, const void* fwd_planes, const void* bwd_planes, float wscale, const float* beta, const float* residual,
                       const float* tgt_cache, const int32_t* idx_table, const int32_t* iter_ptr, int32_t B, int32_t H, int32_t W, int32_t C,
                       float coef, int32_t inverse, float* out, void* dup_planes, float dup_scale, void* dup_overflow_flag, float* t, float* dx,
                       void* dx_planes, float dx_scale, float* loss_out, void* stream);

/* rdo_adaround_step_batch_gather with a parallel array row_groups[n] (0 or 4 per item).  An item with 4 has its rows in 4 groups: its
 * gradient slabs are READ at row (r & 3) rows / 4 + (r >> 2) for logical row r and its forward planes (wq_planes, fp16 two-way) are WRITTEN
 * at that row; everything else of the item -- w, delta, zp, alpha, Adam moments, wq, wd and the dgrad planes -- stays in logical order.
 * Such an item needs a conv layout with rows % 4 == 0 and Cin % 4 == 0 (the tile form of the step) and mode 0 or 2.  All zeros (or a
 * NULL array): the launch of rdo_adaround_step_batch_gather.  `next` may be NULL: no gather rides on the launch. */
int rdo_adaround_step_batch_gather_px(const rdo_ada_step_item* items, int32_t n, int32_t mode, float grad_scale, float round_weight,
                                      const rdo_sched_row* sched, const int32_t* iter_ptr, float* round_loss_out, int32_t* iter_shadow,
                                      const rdo_gather_desc* next, const int32_t* row_groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_SUBPEL_H */
