/*
 * rdo_ptq_mxresunit.h -- C ABI of librdoptq_hip.so, continued: the residual unit of the Cheng2020 attention block on the block-scaled
 * matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 in one launch (csrc/mx_resunit.hip): 1x1 conv N -> N/2, ReLU, 3x3 conv (stride
 * 1, zero padding 1), ReLU, 1x1 conv N/2 -> N, the identity add and the last ReLU.  Same conventions as rdo_ptq_hip.h (borrowed device
 * pointers, hipStream_t as void*, integer status codes; the entry records into a plan); a header of its own because the export tables
 * of the earlier headers are closed (their symbol sets are pinned by the suite).
 *
 * Geometry: x fp32 NHWC [B, H, W, N], one row of N channels per pixel; w1 [N/2][N], w2 [N/2][9 N/2] with its rows in (kh, kw, in)
 * order and w3 [N][N/2], packed MX operands of rdo_ptq_mxgemm.h in the one format w_format, with their scale bytes [rows][K / 32];
 * b1, b2 fp32 [N/2] and b3 fp32 [N] (nullable).  act_format is the MX format of the three activations: x, h1 and h2.
 *
 * rdo_mx_residual_unit: one launch, bit for bit the composition of the existing entries on the same operands:
 *   xp     = rdo_mx_quant_pack(x, act_format)                                                        [B H W][N]
 *   h1     = rdo_mx_gemm_packed(xp, w1, b1, act_format, RDO_MX_ACT_RELU)                             [B H W][N/2]
 *   h2     = rdo_mx_conv2d_packed(h1, w2, B, H, W, N/2, N/2, 3, 1, 1, b2, act_format, RDO_MX_ACT_RELU) [B H W][N/2]
 *   branch = rdo_mx_gemm(h2, w3, b3)                                                                 [B H W][N]
 *   out    = rdo_relu_fwd(rdo_add(x, branch))
 * out is required.  xp / h1 / h2 (each nullable, with its scale bytes) receive the packed operands of those names, branch (nullable)
 * the fp32 tensor.  A block of a quantisation step that holds a NaN or an infinity gets the scale byte 255 and zero codes, as in
 * rdo_mx_quant_pack and rdo_ptq_mxchain.h.
 *
 * RDO_MXRESUNIT_MAX_N: the most channels -- a multiple of 64 -- whose LDS images (the packed 10 x 10 halo of x and of h1 with their
 * scale bytes, FP8) and the 4 608 B of wave-private staging tiles stay within 64 KiB a workgroup: N = 320 takes 52 700 + 4 608 =
 * 57 308 B, N = 384 would take 67 208 B.  Within 64 KiB the launch never raises the kernel's dynamic-LDS attribute and two workgroups
 * fit a CU at the largest N.
 *
 * RDO_EINVAL, with a message that starts with the entry's name and before any launch, for: a NULL x, w1, w2, w3, one of their scale
 * pointers, or out; non-positive B, H, W or N; B H W above 2^31 - 1; N % 64 != 0; N > RDO_MXRESUNIT_MAX_N; an unknown act_format or
 * w_format; xp, h1 or h2 given without its scale pointer or the other way round; x, out or branch not 16-byte aligned; a bias or a
 * packed pointer not 4-byte aligned.
 */
#ifndef RDO_PTQ_MXRESUNIT_H
#define RDO_PTQ_MXRESUNIT_H
#include "rdo_ptq_mxgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDO_MXRESUNIT_MAX_N 320

int rdo_mx_residual_unit(const float* x, int32_t B, int32_t H, int32_t W, int32_t N, int32_t act_format, const void* w1,
                         const uint8_t* w1_scales, const float* b1, const void* w2, const uint8_t* w2_scales, const float* b2,
                         const void* w3, const uint8_t* w3_scales, const float* b3, int32_t w_format, float* out, void* xp,
                         uint8_t* xp_scales, void* h1, uint8_t* h1_scales, void* h2, uint8_t* h2_scales, float* branch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXRESUNIT_H */
