/*
 * rdo_ptq_attnq.h -- C ABI of librdoptq_hip.so, continued: the backward of the two products of the activation-quantised window
 * attention (csrc/attn_tape.hip).  Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status
 * codes); a header of its own because the export table of rdo_ptq_hip.h is closed (its symbol count is pinned by the suite).
 *
 * The quantised attention is evaluated in pieces: rdo_window_attention_fwd (probabilities only), the activation quantiser on the
 * probabilities, rdo_window_attention_pv, the activation quantiser on the result.  The quantisers have a backward of their own
 * (rdo_actquant_static_bwd); the two entries here are the backward of the two attention pieces between them.  Both take the
 * probabilities as GIVEN float32 data: no softmax is recomputed and no shift mask is applied (it is inside the probabilities already).
 *
 * Geometry, token order, the qkv channel order c = which * C + head * hd + d and the probs layout [windows][N][N][heads] are those of
 * rdo_attn_desc and of the header comment of csrc/swin.hip; the same limits hold (N <= 64 tokens per window, head dim <= 64, any shift).
 * qkv, dqkv [B,H,W,3C]; dout [B,H,W,C]; probs, probs_q, dprobs [windows][N][N][heads].
 *
 * Each entry writes EVERY element of every output: the thirds of dqkv an entry does not own get zeros, so the sum of the two dqkv
 * tensors is the whole gradient and an output that held NaNs comes back finite.  No atomics, a fixed summation order: the same input
 * gives the same bits.  Pointers need no alignment beyond 4 bytes (all global accesses are 4 bytes wide).
 * RDO_EINVAL before any launch for: a null pointer; a descriptor the other attention entries refuse; an output that overlaps another
 * operand of the call (dqkv over qkv included).
 */
#ifndef RDO_PTQ_ATTNQ_H
#define RDO_PTQ_ATTNQ_H
#include "rdo_ptq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* backward of rdo_window_attention_pv.  probs_q: the probabilities that product used (fake-quantised outside), dout [B,H,W,C].
 *   dprobs[w][i][j][h] = sum_d dout_id v_jd          every element written, pairs of different shift regions included (no mask here:
 *                                                    it is already in the probabilities)
 *   dqkv[.., 2C + h*hd + d] = sum_i probs_q_ij dout_id ;  dqkv[.., 0 .. 2C) = 0 */
int rdo_window_attention_pv_bwd(const rdo_attn_desc* d, const float* qkv, const float* probs_q, const float* dout,
                                float* dprobs, float* dqkv, void* stream);

/* backward of the probabilities w.r.t. q and k from GIVEN probabilities (the float32 values the forward wrote), dprobs as above:
 *   D_i = sum_j p_ij g_ij;  dS_ij = p_ij (g_ij - D_i);  dQ = scale * (dS K);  dK = dS^T (scale Q)
 *   dqkv[.., 0 .. 2C) = dQ | dK ;  dqkv[.., 2C .. 3C) = 0 */
int rdo_window_attention_probs_bwd(const rdo_attn_desc* d, const float* qkv, const float* probs, const float* dprobs,
                                   float* dqkv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_ATTNQ_H */
