/*
 * rdo_ptq_mxchain.h -- C ABI of librdoptq_hip.so, continued: the block-scaled GEMM, convolution and transposed convolution of
 * rdo_ptq_mxgemm.h / rdo_ptq_mxconv.h / rdo_ptq_mxtconv.h with a PACKED MX OUTPUT (csrc/mx_chain.hip): the epilogue applies the bias and
 * an activation function, quantises each output row's N values to an MX format in blocks of 32 and stores the packed rows and E8M0 bytes
 * -- the next layer's operand -- in the same launch.  No fp32 output reaches memory.  Same conventions as rdo_ptq_hip.h (borrowed device
 * pointers, hipStream_t as void*, integer status codes; every entry records into a plan); a header of its own because the export tables
 * of the earlier headers are closed (their symbol sets are pinned by the suite).
 *
 * The contract is bit equality with the un-fused path: with v = act(y) applied to the fp32 result y of the fp32 entry on the same
 * arguments -- LeakyReLU as v > 0 ? v : 0.01f * v, ReLU as v > 0 ? v : 0, both in fp32 --, y_packed and y_scales hold exactly the bytes
 * rdo_mx_quant_pack(v, rows = output rows, K = N, out_format) writes (tests/test_gpu_mx_chain.py).  The K loop is the fp32 entry's, in
 * the same K order, so the accumulators are its; the bias is added and the activation applied as separate fp32 operations.  A block that
 * holds a NaN or an infinity gets the scale byte 255 and zero codes.  The output's blocks run along N -- the K of the layer that reads
 * it --, hence N % 32 == 0.  The output is [rows][N] with rows = M (GEMM) or B * Ho * Wo output pixels in NHWC order (convolutions):
 * y_packed has rdo_mx_packed_bytes(rows, N, out_format) bytes, y_scales rows * N / 32.
 */
#ifndef RDO_PTQ_MXCHAIN_H
#define RDO_PTQ_MXCHAIN_H
#include "rdo_ptq_mxtconv.h"
#include "rdo_ptq_mxconv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* activation ids of the packed entries */
#define RDO_MX_ACT_NONE 0
#define RDO_MX_ACT_LRELU 1 /* LeakyReLU with slope 0.01 */
#define RDO_MX_ACT_RELU 2

/* Every entry below returns RDO_EINVAL, with a message that starts with the entry's name and before any launch, for everything its fp32
 * twin refuses (the twin's y aside) and for: an out_format that is no RDO_MX_* format; an act that is none of the ids above; N % 32 != 0;
 * a NULL y_packed or y_scales; a y_packed that is not 4-byte aligned. */

/* rdo_mx_gemm with the output act(A B^T + bias) packed in out_format: [M][N] */
int rdo_mx_gemm_packed(const void* a, const uint8_t* a_scales, int32_t a_format, const void* b, const uint8_t* b_scales, int32_t b_format,
                       int32_t M, int32_t N, int64_t K, const float* bias, int32_t out_format, int32_t act, void* y_packed, uint8_t* y_scales,
                       void* stream);

/* rdo_mx_conv2d with the output act(conv(x, w) + bias) packed in out_format: [B*Ho*Wo][N], one packed row per output pixel */
int rdo_mx_conv2d_packed(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales, int32_t w_format,
                         int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad, const float* bias,
                         int32_t out_format, int32_t act, void* y_packed, uint8_t* y_scales, void* stream);

/* rdo_mx_conv_transpose2d with the output act(conv_transpose(x, w) + bias) packed in out_format: [B*Ho*Wo][N]; an output pixel of a phase
 * without taps holds the quantised act(bias) */
int rdo_mx_conv_transpose2d_packed(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales,
                                   int32_t w_format, int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride,
                                   int32_t pad, int32_t output_padding, const float* bias, int32_t out_format, int32_t act, void* y_packed,
                                   uint8_t* y_scales, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXCHAIN_H */
