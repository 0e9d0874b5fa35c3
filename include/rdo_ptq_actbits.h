/*
 * rdo_ptq_actbits.h -- C ABI of librdoptq_hip.so, continued: activation widths per unit (the width scan of csrc/actquant.hip).
 * Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status codes); a header of its own
 * because the export table of rdo_ptq_hip.h is closed (its symbol count is pinned by the suite).
 */
#ifndef RDO_PTQ_ACTBITS_H
#define RDO_PTQ_ACTBITS_H
#include "rdo_ptq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDO_ACT_WIDTH_SCAN_MAX_K 8      /* widths per call */
#define RDO_ACT_WIDTH_SCAN_MIN_BITS 2
#define RDO_ACT_WIDTH_SCAN_MAX_BITS 16

/* What ONE per-channel grid costs an activation at K widths, in one read of the tensor.  x fp32 [npix][C] (NHWC storage, channel
 * fastest), range = lo[C] | hi[C], widths: a HOST array of K distinct widths b_k in [2, 16], read before anything is launched.  With Q_k
 * the static expression of rdo_actquant_static on lo | hi at n_bits = b_k (r = max(hi_c - lo_c, 1e-6), lower clamp 0, 2^b_k - 1 steps: the
 * scanned grid is the applied grid, bit for bit),
 *   err[c][k]  = sum_p (x - Q_k(x))^2        the residual and its square formed in fp32, exactly as rdo_actquant_score forms them
 *   energy[c]  = sum_p x^2                   (may be null: err is the same bits with or without it)
 * With range = the tensor's own per-channel min | max this is the grid of rdo_actquant_perchannel too (x - min is never negative, so its
 * lower clamp at -1 and this one at 0 give the same bits): one kernel serves static and dynamic quantisers.
 * Both outputs are WRITTEN, not accumulated into: a caller that adds batches does so itself (the host adds them in float64).
 * One read of x (16-byte accesses when C % 4 == 0 and x is 16-byte aligned, 4-byte ones otherwise); per-workgroup partial sums in ws,
 * folded in the fixed order the head comment of csrc/actquant.hip states (no atomics: the same input gives the same bits); no serial fp32
 * chain longer than 1024 terms.
 * Refused with RDO_EINVAL before any launch: a null x, range, widths, err or ws, npix <= 0 or npix >= 2^31, C <= 0 (or so many channels
 * that 9 C entries are beyond 32-bit indices), K outside [1, RDO_ACT_WIDTH_SCAN_MAX_K], a width outside [2, 16], a width given twice. */
int rdo_actquant_width_scan(const float* x, int64_t npix, int32_t C, const float* range /* [2 C] lo | hi */,
                            const int32_t* widths /* HOST array [K], read before the launch */, int32_t K,
                            float* err /* [C][K], written */, float* energy /* [C] or null, written */,
                            float* ws /* rdo_actquant_width_scan_workspace(C, K) floats, no initial state needed */, void* stream);
/* floats; 0 for C <= 0, too many channels or K outside [1, RDO_ACT_WIDTH_SCAN_MAX_K] */
int64_t rdo_actquant_width_scan_workspace(int32_t C, int32_t K);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_ACTBITS_H */
