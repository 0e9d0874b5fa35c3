/*
 * rdo_ptq_mxtconv.h -- C ABI of librdoptq_hip.so, continued: transposed k x k convolutions on the block-scaled matrix instruction from the
 * packed MX operands of rdo_ptq_mxgemm.h (csrc/mx_tconv.hip).  Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as
 * void*, integer status codes; every entry records into a plan); a header of its own because the export tables of the earlier headers are
 * closed (their symbol sets are pinned by the suite).
 *
 * y[b, oy, ox, n] = bias[n] + sum x[b, iy, ix, c] w[n, kh, kw, c] over the taps with (oy + pad - kh) % stride == 0,
 * iy = (oy + pad - kh) / stride in [0, H), and the same in x; Ho = (H - 1) stride - 2 pad + k + output_padding, Wo likewise.  The
 * activation is NHWC with one packed row of C / 32 blocks per pixel; the weight rows are those of to_rows(W, tconv=True): row n, tap
 * (kh, kw), channel c holds W[c, n, kh, kw], taps un-flipped; with C % 32 == 0 every block lies inside one tap.  No format is new and
 * nothing is re-packed.
 *
 * The phase of an output pixel is (ry, rx) = ((oy + pad) % stride, (ox + pad) % stride); all pixels of a phase use the taps
 * kh in {ry, ry + stride, ...} < k and kw in {rx, rx + stride, ...} < k.  The gathered row of an output pixel lists those taps in
 * ascending (kh, kw) order, C / 32 blocks each -- a tap whose input pixel lies outside the image is a block of zero codes under the
 * scale byte 127 --, the gathered weight row of the phase is blocks (kh k + kw) C / 32 + c of weight row n in the same order.  The K
 * order is a contract: K step j covers blocks 4 j .. 4 j + 3 of the gathered row; for every output the instructions and their operands
 * are those rdo_mx_gemm issues on (gathered activation matrix of the phase) x (gathered weight matrix of the phase), and the result
 * equals rdo_mx_gemm's on them bit for bit (tests/test_gpu_mx_tconv.py).  A phase without taps (k < stride, rows and columns that
 * output_padding adds past the last tap) is bias alone, or 0 without a bias.  The GEMM's accuracy statement carries over with K the
 * number of elements of the gathered row (at most ceil(k / stride)^2 C): an fp32 sum of exact products within K 2^-23 (sum |a b| + |bias|)
 * of the real sum for every format pair, a pair with an FP8 operand running the eight-pass form.  A scale code of 255 leaves every output
 * that sums over that block unspecified.  Any stride >= 1 is served; the launch has stride^2 phases of tiles, which the tile limit bounds.
 */
#ifndef RDO_PTQ_MXTCONV_H
#define RDO_PTQ_MXTCONV_H
#include "rdo_ptq_mxgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* output pixels B * Ho * Wo with Ho = (H - 1) stride - 2 pad + k + output_padding (Wo likewise); 0 for a refused geometry: B, H, W, k or
 * stride <= 0, pad < 0, output_padding < 0 or >= stride, Ho <= 0 or Wo <= 0, B * H * W or B * Ho * Wo above 2^31 - 1.  Host only. */
int64_t rdo_mx_conv_transpose2d_out_pixels(int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad, int32_t output_padding);

/* y fp32 [B*Ho*Wo][N] (NHWC) = conv_transpose(x, w) (+ bias[n]).
 * x  packed [B*H*W][C] in x_format with x_scales uint8 [B*H*W][C/32]   -- an NHWC activation, one packed row per pixel
 *                                                                        (what rdo_mx_quant_pack writes from the NHWC rows)
 * w  packed [N][k*k*C] in w_format with w_scales uint8 [N][k*k*C/32]   -- rows in (kh, kw, in) order, taps un-flipped
 * square kernel k, one stride, one padding, one output padding, dilation 1, groups 1; any of the 5 x 5 format pairs; bias fp32 [N],
 * nullable.
 * RDO_EINVAL, with a message that starts with the entry's name and before any launch, for: a NULL required pointer; a packed, bias or y
 * pointer that is not 4-byte aligned; an unknown format; B, H, W, C, N, k or stride <= 0; pad < 0; output_padding < 0 or >= stride;
 * C % 32 != 0; Ho <= 0 or Wo <= 0; B * H * W or B * Ho * Wo above 2^31 - 1; more than 2^40 blocks in either operand; more than 2^31 - 1
 * output tiles of 64 x 64 over the stride^2 phases (each phase is given the tiles of the largest). */
int rdo_mx_conv_transpose2d(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales, int32_t w_format,
                            int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad,
                            int32_t output_padding, const float* bias, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXTCONV_H */
