/*
 * rdo_ptq_mxconv.h -- C ABI of librdoptq_hip.so, continued: k x k convolutions on the block-scaled matrix instruction from the packed MX
 * operands of rdo_ptq_mxgemm.h (csrc/mx_conv.hip).  Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*,
 * integer status codes; every entry records into a plan); a header of its own because the export tables of the earlier headers are
 * closed (their symbol sets are pinned by the suite).
 *
 * The convolution is rdo_mx_gemm with the A-side block address computed per (output pixel, tap): the activation is NHWC with one packed
 * row of C / 32 blocks per pixel, the weight rows are in (kh, kw, in) order, so with C % 32 == 0 block kb of an im2col row lies inside
 * tap t = kb / (C / 32) = (kh, kw) = (t / k, t % k) and is channel block kb % (C / 32) of input pixel (b, oy stride - pad + kh,
 * ox stride - pad + kw); a tap outside the image is a block of zero codes under the scale byte 127.  No im2col matrix is written.
 * The K order is a contract: for every output the instructions and their operands are those rdo_mx_gemm issues on that im2col matrix,
 * and the result equals rdo_mx_gemm's on it bit for bit (tests/test_gpu_mx_conv.py).  Its accuracy statement carries over with
 * K = k k C: an fp32 sum of exact products within K 2^-23 (sum |a b| + |bias|) of the real sum for every format pair, a pair with an FP8
 * operand running the eight-pass form.  A scale code of 255 leaves every output that sums over that block unspecified.
 */
#ifndef RDO_PTQ_MXCONV_H
#define RDO_PTQ_MXCONV_H
#include "rdo_ptq_mxgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* output pixels B * Ho * Wo with Ho = (H + 2 pad - k) / stride + 1 (Wo likewise); 0 for a refused geometry: B, H, W, k or stride <= 0,
 * pad < 0, H + 2 pad < k or W + 2 pad < k, B * H * W or B * Ho * Wo above 2^31 - 1.  Host only. */
int64_t rdo_mx_conv2d_out_pixels(int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad);

/* y fp32 [B*Ho*Wo][N] (NHWC) = conv(x, w) (+ bias[n]).
 * x  packed [B*H*W][C] in x_format with x_scales uint8 [B*H*W][C/32]   -- an NHWC activation, one packed row per pixel
 *                                                                        (what rdo_mx_quant_pack writes from the NHWC rows)
 * w  packed [N][k*k*C] in w_format with w_scales uint8 [N][k*k*C/32]   -- rows in (kh, kw, in) order
 * square kernel k, one stride, one zero padding, dilation 1, groups 1; any of the 5 x 5 format pairs; bias fp32 [N], nullable.
 * RDO_EINVAL, with a message that starts with the entry's name and before any launch, for: a NULL required pointer; a packed, bias or y
 * pointer that is not 4-byte aligned; an unknown format; B, H, W, C, N, k or stride <= 0; pad < 0; C % 32 != 0; H + 2 pad < k or
 * W + 2 pad < k; B * H * W or B * Ho * Wo above 2^31 - 1; more than 2^40 blocks in either operand; more than 2^31 - 1 output tiles of
 * 64 x 64. */
int rdo_mx_conv2d(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales, int32_t w_format,
                  int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad,
                  const float* bias, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXCONV_H */
