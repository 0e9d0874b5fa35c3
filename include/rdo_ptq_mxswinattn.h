/*
 * rdo_ptq_mxswinattn.h -- C ABI of librdoptq_hip.so, continued: the attention half of a Swin transformer block on the block-scaled matrix
 * instruction v_mfma_scale_f32_16x16x128_f8f6f4 in one launch (csrc/mx_swin_attn.hip): LayerNorm, the qkv Linear, the window attention
 * core, the proj Linear and the residual add.  Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*,
 * integer status codes; every entry records into a plan); a header of its own because the export tables of the earlier headers are
 * closed (their symbol sets are pinned by the suite).
 *
 * Geometry: the descriptor of rdo_window_attention_fwd.  x fp32 [B, H, W, C] in natural pixel order; ln_weight, ln_bias fp32 [C]
 * (nullable: ones / zeros); wqkv [3C][C] and wproj [C][C] packed MX operands of rdo_ptq_mxgemm.h in the one format w_format with their
 * scale bytes wqkv_scales [3C][C / 32] and wproj_scales [C][C / 32]; bqkv fp32 [3C] and bproj fp32 [C] (nullable); bias fp32
 * [heads, N, N], the relative-position bias.  act_format is the MX format of every activation: the LayerNorm, Q, K, V, the
 * probabilities and the attention output.
 *
 * rdo_mx_swin_attn: one launch, bit for bit the composition of the existing entries on the same operands:
 *   ln     = rdo_add_layer_norm(x, NULL, ln_weight, ln_bias, eps)                                   [B, H, W, C]
 *   qkv    = rdo_mx_gemm(rdo_mx_quant_pack(ln, act_format), wqkv, bqkv)                             [B, H, W, 3C]
 *   attn   = rdo_mx_window_attention(desc, qkv, bias, act_format, act_format)                       [B, H, W, C]
 *   branch = rdo_mx_gemm(rdo_mx_quant_pack(attn, act_format), wproj, bproj)                         [B, H, W, C]
 *   out    = rdo_add(x, branch)
 * out is required; ln, qkv, attn and branch (each nullable) receive the fp32 tensors of those names.  Only p_format == act_format is
 * served; another format of the probabilities keeps the five launches.  A block of a quantisation step that holds a NaN or an infinity
 * gets the scale byte 255 and zero codes, as in rdo_ptq_mxchain.h and rdo_ptq_mxattn.h; the outputs of a window that holds a
 * non-finite value are unspecified, every other window's unaffected.
 *
 * RDO_EINVAL, with a message that starts with the entry's name and before any launch, for: everything rdo_mx_window_attention refuses
 * of a descriptor (a head dim that is no multiple of 4 included); C no multiple of 32; C > RDO_MXSWINATTN_MAX_C (the kernel's LDS: the
 * header comment of csrc/mx_swin_attn.hip states the sum); an unknown act_format or w_format; a NULL x, wqkv, wqkv_scales, wproj,
 * wproj_scales, bias or out; an fp32 pointer other than `bias` that is not 16-byte aligned; bias or a packed pointer that is not 4-byte
 * aligned.
 */
#ifndef RDO_PTQ_MXSWINATTN_H
#define RDO_PTQ_MXSWINATTN_H
#include "rdo_ptq_mxgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDO_MXSWINATTN_MAX_C 320

int rdo_mx_swin_attn(const rdo_attn_desc* desc, const float* x, const float* ln_weight, const float* ln_bias, float eps,
                     int32_t act_format, const void* wqkv, const uint8_t* wqkv_scales, const float* bqkv, const void* wproj,
                     const uint8_t* wproj_scales, const float* bproj, int32_t w_format, const float* bias, float* out, float* ln,
                     float* qkv, float* attn, float* branch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXSWINATTN_H */
