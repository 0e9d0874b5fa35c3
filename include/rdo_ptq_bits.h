/*
 * rdo_ptq_bits.h -- C ABI of librdoptq_hip.so, continued: mixed-precision weight widths (csrc/bit_alloc.hip).
 * Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status codes); a header of its own
 * because the export table of rdo_ptq_hip.h is closed (its symbol count is pinned by the suite).
 */
#ifndef RDO_PTQ_BITS_H
#define RDO_PTQ_BITS_H
#include "rdo_ptq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDO_WIDTH_SCAN_MAX_K 8          /* widths per call */
#define RDO_WIDTH_SCAN_MIN_BITS 2
#define RDO_WIDTH_SCAN_MAX_BITS 16
#define RDO_WIDTH_SCAN_LDS_ROW 8192     /* the longest row (floats) that one workgroup stages in LDS; longer rows are split over workgroups */
#define RDO_WIDTH_SCAN_CHUNK 4096       /* floats of a split row per workgroup */

/* What round-to-nearest costs a weight at K widths, in one call.  w fp32 [rows][inner] (the row matrix of a weight quantiser: rows =
 * quantisation channels), widths: a HOST array of K distinct widths b_k in [2, 16], read before anything is launched; n_levels = 2^b_k.
 *   delta, zp   fp32 [K][rows]: with delta_in == zp_in == NULL the grids of rdo_uaq_init_minmax(w, rows, inner, 2^b_k) bit for bit (row
 *               min / max clamped through 0, the range divided in double and rounded once, floor 1e-8, zp = rintf(rcp(delta) * -min));
 *               with both given (fp32 [K][rows]) those grids, copied through.  Exactly one of the two given is refused.
 *   err         double [K][rows]: sum_i d^2, d = w_i - wq_i formed in fp32 with wq_i the expression of rdo_uaq_fakequant
 *               (clamp(rintf(w_i / delta) + zp, 0, 2^b_k - 1) - zp) * delta -- one device function shared with it (csrc/uaq_device.h)
 *   energy      double [rows]: sum_i w_i^2
 * The squares are formed in double ((double)d * (double)d is exact) and added in double in a fixed order: thread t of 256 adds the
 * elements t, t + 256, .. of its share in ascending order, the 64 lanes of a wave fold by __shfl_down 32 .. 1, the four waves add as
 * ((w0 + w1) + w2) + w3, and the shares of a split row add the same way.  No atomics: the same input gives the same bits.
 * A row of inner <= RDO_WIDTH_SCAN_LDS_ROW is read from memory once by one workgroup, staged in LDS while its min / max are taken, and
 * all K widths are scored from LDS: one launch.  A longer row is split into shares of RDO_WIDTH_SCAN_CHUNK floats, one workgroup each:
 * share min / max -> ws, the rows' grids, the shares' sums -> ws, the fixed-order sum of the shares -- launches on the same stream (the
 * second pass over w of the min-max mode reads what the first left in the caches; with given grids there is one pass).
 * ws: rdo_uaq_width_scan_workspace(rows, inner, K) bytes, 8-byte aligned, no initial state needed; err and energy 8-byte aligned. */
int rdo_uaq_width_scan(const float* w, int32_t rows, int64_t inner, const int32_t* widths, int32_t K, const float* delta_in,
                       const float* zp_in, float* delta, float* zp, double* err, double* energy, void* ws, void* stream);
/* bytes (> 0 for every accepted geometry, so that ws is never NULL); 0 for rows <= 0, inner <= 0, K outside [1, 8] or more than 2^31 - 1
 * shares */
int64_t rdo_uaq_width_scan_workspace(int32_t rows, int64_t inner, int32_t K);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_BITS_H */
