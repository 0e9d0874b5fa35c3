/*
 * rdo_ptq_mxswin.h -- C ABI of librdoptq_hip.so, continued: the LayerNorm producer and the MLP half of a Swin transformer block on the
 * block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 (csrc/mx_swin.hip).  Same conventions as rdo_ptq_hip.h (borrowed
 * device pointers, hipStream_t as void*, integer status codes; every entry records into a plan); a header of its own because the export
 * tables of the earlier headers are closed (their symbol sets are pinned by the suite).
 *
 * With a, b fp32 [rows][C] (b nullable), weight and bias fp32 [C] (nullable: ones / zeros):
 *   s  = a + b, what rdo_add writes (a itself without b)
 *   ln = rdo_add_layer_norm(a, b, weight, bias, eps), bit for bit
 *
 * rdo_mx_layer_norm_pack: one launch; out_packed (rdo_mx_packed_bytes(rows, C, format) bytes) and out_scales (rows * C / 32) receive what
 * rdo_mx_quant_pack(ln, rows, C, format) writes, bit for bit (a block that holds a NaN or an infinity gets the scale byte 255 and zero
 * codes, as in rdo_ptq_mxchain.h); sum_out (nullable; needs b) receives s, ln (nullable) the fp32 LayerNorm.
 *
 * rdo_mx_swin_mlp: one launch; with w1 [Hd][C] and w2 [C][Hd] packed MX operands of rdo_ptq_mxgemm.h in the one format w_format, their
 * scale bytes w1_scales [Hd][C / 32] and w2_scales [C][Hd / 32], b1 fp32 [Hd] and b2 fp32 [C] (nullable),
 *   pre    = rdo_mx_gemm(rdo_mx_quant_pack(ln, act_format), w1, b1)      [rows][Hd]
 *   hidden = rdo_mx_quant_pack(gelu(pre), act_format)                    exact-erf GELU, what rdo_gelu_fwd writes
 *   out    = s + rdo_mx_gemm(hidden, w2, b2)                             [rows][C], the sum a separate fp32 add
 * each bit for bit.  Neither packed activation reaches memory unless asked for: ln and pre (nullable) receive the fp32 tensors of those
 * names, hidden with hidden_scales (both or neither) the packed hidden operand (rdo_mx_packed_bytes(rows, Hd, act_format) bytes, rows *
 * Hd / 32 scale bytes).  A row that holds a non-finite value leaves that row's outputs unspecified and every other row's unaffected.
 *
 * Both entries return RDO_EINVAL, with a message that starts with the entry's name and before any launch, for: a NULL required pointer;
 * rows <= 0; C (or Hd) no positive multiple of 32; C > RDO_MXSWIN_MAX_C or Hd > RDO_MXSWIN_MAX_HIDDEN (the 64-row images of the two
 * packed activations in LDS); an unknown format; sum_out without b; one of hidden / hidden_scales without the other; an fp32 pointer
 * that is not 16-byte aligned; a packed pointer that is not 4-byte aligned.
 */
#ifndef RDO_PTQ_MXSWIN_H
#define RDO_PTQ_MXSWIN_H
#include "rdo_ptq_mxgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDO_MXSWIN_MAX_C 512
#define RDO_MXSWIN_MAX_HIDDEN 1024

int rdo_mx_layer_norm_pack(const float* a, const float* b, const float* weight, const float* bias, int32_t rows, int32_t C, float eps,
                           int32_t format, void* out_packed, uint8_t* out_scales, float* sum_out, float* ln, void* stream);

int rdo_mx_swin_mlp(const float* a, const float* b, const float* ln_weight, const float* ln_bias, float eps, int32_t rows, int32_t C,
                    int32_t Hd, int32_t act_format, const void* w1, const uint8_t* w1_scales, const float* b1, const void* w2,
                    const uint8_t* w2_scales, const float* b2, int32_t w_format, float* out, float* ln, float* pre, void* hidden,
                    uint8_t* hidden_scales, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXSWIN_H */
