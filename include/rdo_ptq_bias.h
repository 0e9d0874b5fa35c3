/*
 * rdo_ptq_bias.h -- C ABI of librdoptq_hip.so, continued: empirical bias correction after calibration (csrc/bias_correct.hip).
 * Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status codes); a header of its own
 * because the export table of rdo_ptq_hip.h is closed (its symbol count is pinned by the suite).
 */
#ifndef RDO_PTQ_BIAS_H
#define RDO_PTQ_BIAS_H
#include "rdo_ptq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tap sums of a layer input: out[kh][kw][c] += sum over the images and over the input pixels (h, w) that tap (kh, kw) of a k x k
 * convolution reads over all its valid outputs, of x[img][h][w][c].  With them the sum over all output pixels of the pre-activation of
 * ANY weight W[o][kh][kw][c] on this input is n b[o] + sum W[o][kh][kw][c] out[kh][kw][c]: zero padding, stride and borders exactly.
 * Row h belongs to tap kh (and likewise column w to kw) when
 *   conv (transposed = 0):   u = h + pad - kh,  u >= 0, u % stride == 0, u / stride < Ho      (Ho = (H + 2 pad - k) / stride + 1)
 *   transposed conv:         0 <= h stride - pad + kh < Ho        ((H - 1) stride - 2 pad + k <= Ho < that + stride: output_padding)
 * x fp32 NHWC, read once; 16-byte loads when C % 4 == 0 and x is 16-byte aligned, scalar loads otherwise.  out fp32 [k * k][C] is ADDED
 * TO.  ws: rdo_tap_sums_workspace(C, k) floats, no initial state needed.  No atomics: the summation order is a function of the geometry
 * alone, the same input gives the same bits; no serial fp32 chain is longer than 1024 terms.  k <= RDO_TAP_MAX_K.  A Linear layer is
 * k = 1, stride 1, pad 0 with every token a pixel (N = H = 1, W = tokens). */
#define RDO_TAP_MAX_K 7
int rdo_tap_sums(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, int32_t Ho,
                 int32_t Wo, int32_t transposed, float* out, float* ws, void* stream);
int64_t rdo_tap_sums_workspace(int32_t C, int32_t k);   /* floats; 0 for C <= 0 or k outside [1, RDO_TAP_MAX_K] */
/* The most pixels one lane of rdo_tap_sums adds into one running value between two folds for this geometry (vec: the 16-byte path), so
 * that a test of the 1024-pixel chain closure can tell whether its shape reaches it; -1 (and the message) for what rdo_tap_sums refuses. */
int64_t rdo_tap_sums_lane_pixels(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                 int32_t transposed, int32_t vec);

/* The bias shift of one layer from float64 tap sums: per output row o, in float64 and a fixed order,
 *   shift[o] = (sum_j w_ref[o][j] s_ref[j] - sum_j w_q[o][j] s_q[j]) * inv_n ,   bias_out[o] = (float)(org_bias[o] + shift[o])
 * w_ref, w_q fp32 [O][K] (rows in the order of the tap sums: [kh][kw][c]); s_ref, s_q double [K]; shift double [O]; bias_out fp32 [O].
 * s_ref may be s_q and w_ref may be w_q. */
int rdo_bias_shift(const float* w_ref, const float* w_q, const double* s_ref, const double* s_q, double inv_n, const float* org_bias,
                   int32_t O, int32_t K, double* shift, float* bias_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_BIAS_H */
