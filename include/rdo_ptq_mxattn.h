/*
 * rdo_ptq_mxattn.h -- C ABI of librdoptq_hip.so, continued: the window attention core with both of its products, Q K^T and P V, on the
 * block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 (csrc/mx_attn.hip).  Same conventions as rdo_ptq_hip.h (borrowed
 * device pointers, hipStream_t as void*, integer status codes; every entry records into a plan); a header of its own because the export
 * tables of the earlier headers are closed (their symbol sets are pinned by the suite).
 *
 * Geometry and operands are those of rdo_window_attention_fwd: qkv fp32 [B, H, W, 3C] in natural pixel order, channel c = which * C +
 * head * hd + d; bias fp32 [heads, N, N]; the descriptor's window / shift addressing; the mask -100 between tokens of different regions.
 * Hp = hd rounded up to 32, Np = N rounded up to 32.  `format` is the MX format of Q, K and V, `p_format` that of the probabilities; any of
 * the 5 x 5 pairs.  For one (window, head):
 *   Qp, Kp  the [N, hd] tiles of q and k as qkv holds them (the softmax scale is no power of two and is NOT folded into q), zero-padded
 *           along hd to Hp and quantised to `format` in blocks of 32 along hd: what rdo_mx_quant_pack writes for the padded rows
 *   raw     rdo_mx_gemm(Qp, Kp): one K step from zero accumulators (an FP8 operand: the eight one-of-eight passes, in that order)
 *   s_ij    raw_ij * scale + (bias_ij + mask_ij) in fp32: a product, then a sum, the bias and the mask added first
 *   p       the row softmax of s over j < N in fp32: maximum, __expf(s - max), sum, multiplication by the reciprocal of the sum
 *   Pp      p [N, N] zero-padded along j to Np and quantised to `p_format` in blocks of 32 along j
 *   Vt      v transposed to [hd, N], zero-padded along the tokens to Np and quantised to `format` in blocks of 32 ALONG THE TOKENS, the
 *           reduction axis of the second product
 *   out_id  rdo_mx_gemm(Pp, Vt), written to the token's pixel as rdo_window_attention_fwd writes it
 * A block of a quantisation step that holds a NaN or an infinity gets the scale byte 255 and zero codes, as in rdo_ptq_mxchain.h; outputs
 * that sum over such a block are unspecified.  This is NOT what rdo_window_attention_fwd computes: Q, K, P and V are each rounded to an MX
 * grid, V along another axis than any Linear would round it.
 *
 * rdo_mx_window_attention: one launch.  out fp32 [B, H, W, C]; scores and probs (each nullable) fp32 [windows, N, N, heads], the layout of
 * rdo_window_attention_fwd's probs: s and p (before its quantisation) of every pair.
 * RDO_EINVAL, with a message that starts with the entry's name and before any launch, for: everything rdo_window_attention_fwd refuses
 * of a descriptor; a head dim that is no multiple of 4 (there is no scalar path); an unknown format; a NULL qkv, bias or out; qkv or out
 * not 16-byte aligned; bias, scores or probs not 4-byte aligned.
 */
#ifndef RDO_PTQ_MXATTN_H
#define RDO_PTQ_MXATTN_H
#include "rdo_ptq_mxgemm.h"

#ifdef __cplusplus
extern "C" {
#endif

int rdo_mx_window_attention(const rdo_attn_desc* desc, const float* qkv, const float* bias, int32_t format, int32_t p_format, float* out,
                            float* scores, float* probs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXATTN_H */
