/*
 * rdo_ptq_gdn.h -- C ABI of librdoptq_hip.so, continued: the GDN / IGDN block of a calibration unit as one launch.
 * Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status codes); a header of its own
 * because the export table of rdo_ptq_hip.h is closed (its symbol count is pinned by the suite).
 */
#ifndef RDO_PTQ_GDN_H
#define RDO_PTQ_GDN_H
#include "rdo_ptq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The GDN / IGDN block of a unit, forward and backward, in ONE launch (csrc/gdn_fused.hip; quant_layer.py:142-147 norm pool and
 * epilogue, layer_opt.py:133,150 loss and gradient):  norm = beta' + gamma' . c^2 ; out = c * norm^(-1/2 | +1/2) (+ residual) ;
 * loss, grad_out = dL/dout and t = dL/dnorm as rdo_loss_gdn_bwd ; acc = t . gamma' ; dx = grad_out * norm^(-1/2 | +1/2) + 2 c acc
 *   = rdo_linear_h2(square_input) + rdo_loss_gdn_bwd + rdo_linear_h2 (planes of gamma'^T) + rdo_gdn_bwd_dx_h2, whose outputs it
 * reproduces bit for bit (the loss partial sums are added in another order); `norm` and `acc` never exist in memory.
 * c [B * per_image / C][C] fp32 (NHWC); fwd_planes / bwd_planes: rdo_split_h2_linear of gamma' and of gamma'^T, both times wscale;
 * out, grad_out, dx, dx_planes nullable (dx_planes: H2 planes of dx * dx_scale, overflow reported as by rdo_gdn_bwd_dx_h2); t fp32.
 * rdo_gdn_fwd_bwd_supported: C = 192 and M % 64 == 0 (and what rdo_linear_h2_supported asks); everything else keeps the four launches.
 * A loss / tail launch in the sense of rdo_iter_bind_publish. */
int rdo_gdn_fwd_bwd_supported(int64_t M, int32_t C);
int rdo_gdn_fwd_bwd(const float* c, const void* fwd_planes, const void* bwd_planes, float wscale, const float* beta, const float* residual,
                    const float* tgt_cache, const int32_t* idx_table, const int32_t* iter_ptr, int32_t B, int64_t per_image, int32_t C,
                    float coef, int32_t inverse, float* out, float* grad_out, float* t, float* dx, void* dx_planes, float dx_scale,
                    float* loss_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_GDN_H */
