/*
 * rdo_ptq_mxgdn.h -- C ABI of librdoptq_hip.so, continued: the GDN / IGDN forward with its norm pool on the block-scaled matrix
 * instruction v_mfma_scale_f32_16x16x128_f8f6f4, in one launch (csrc/mx_gdn.hip).  Same conventions as rdo_ptq_hip.h (borrowed device
 * pointers, hipStream_t as void*, integer status codes; every entry records into a plan); a header of its own because the export tables
 * of the earlier headers are closed (their symbol sets are pinned by the suite).
 *
 * With x fp32 [rows][C] (the NHWC pixels), g the packed MX operand of gamma' [C][C] (rdo_ptq_mxgemm.h: blocks along the input channel,
 * g_scales uint8 [C][C / 32]) and beta fp32 [C] (beta'), an entry computes
 *   a     = what rdo_mx_quant_pack(x o x, rows, C, x2_format) writes (one fp32 multiply per element); it stays in LDS
 *   norm  = rdo_mx_gemm(a, g, beta) [rows][C], bit for bit: the same K steps of 128 in ascending order, the same one-of-eight passes for
 *           an FP8 operand, blocks past C / 32 of the last step as zeros under the scale 127
 *   y     = x * __frsqrt_rn(norm) (inverse = 0, GDN) or x * __fsqrt_rn(norm) (inverse = 1, IGDN), separate fp32 operations
 * and writes y as fp32 (rdo_mx_gdn) or as the packed operand rdo_mx_quant_pack(y, rows, C, out_format) writes, bit for bit
 * (rdo_mx_gdn_packed: y_packed has rdo_mx_packed_bytes(rows, C, out_format) bytes, y_scales rows * C / 32; a block that holds a NaN
 * or an infinity gets the scale byte 255 and zero codes, as in rdo_ptq_mxchain.h).  norm (nullable) receives the norm pool.  A row
 * of x that holds a non-finite value leaves that row's outputs unspecified and every other row's unaffected.
 *
 * Both entries return RDO_EINVAL, with a message that starts with the entry's name and before any launch, for: a NULL required
 * pointer; rows <= 0; C <= 0; C % 32 != 0; C > RDO_MXGDN_MAX_C (the 64-row image of a in LDS: at most 33 KB + 1 KB of scales at C =
 * 512 in FP8, beside 18 KB of epilogue tiles); an unknown x2_format, g_format or out_format; g, beta or y_packed not 4-byte aligned;
 * x, y or norm not 16-byte aligned (the kernel moves them as float4); inverse outside {0, 1}.
 */
#ifndef RDO_PTQ_MXGDN_H
#define RDO_PTQ_MXGDN_H
#include "rdo_ptq_mxgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDO_MXGDN_MAX_C 512

int rdo_mx_gdn(const float* x, int32_t rows, int32_t C, int32_t x2_format, const void* g, const uint8_t* g_scales, int32_t g_format,
               const float* beta, int32_t inverse, float* y, float* norm, void* stream);

int rdo_mx_gdn_packed(const float* x, int32_t rows, int32_t C, int32_t x2_format, const void* g, const uint8_t* g_scales, int32_t g_format,
                      const float* beta, int32_t inverse, int32_t out_format, void* y_packed, uint8_t* y_scales, float* norm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXGDN_H */
