/*
 * rdo_ptq_mx.h -- C ABI of librdoptq_hip.so, continued: OCP microscaling (MX) block formats for weights (csrc/mx_quant.hip).
 * Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status codes); a header of its own
 * because the export table of rdo_ptq_hip.h is closed (its symbol count is pinned by the suite).
 *
 * A weight is its row matrix [rows][inner] (rows of the GEMM's K dimension).  Each row is cut into blocks of RDO_MX_BLOCK consecutive
 * elements; the last block of a row may be shorter, a block never spans two rows.  Per block, with amax = max |v_i|:
 *   E = clamp(floor(log2(amax)) - emax, -127, 127) (exact on the fp32 value, fp32 subnormals included; -127 when amax == 0), X = 2^E,
 *   scale code = the byte E + 127 (E8M0: 0 .. 254);
 *   element: |v / X| to the nearest representable magnitude of the element format, ties to the even mantissa, magnitudes above the
 *   format's maximum become the maximum; the code's sign bit is the sign bit of v (-0 keeps its sign);
 *   wq = q * X, exactly representable in fp32 for every format and every E.
 * Element formats (sign | exponent | mantissa in the low 4 / 6 / 8 bits of one byte per element, upper bits zero; normals
 * 2^(e - bias) (1 + m / 2^M) for e >= 1, subnormals 2^(1 - bias) m / 2^M; the E4M3 NaN pattern and the E5M2 infinities are never
 * produced from finite input):
 *   id  name          s/e/m   bias  emax  max     smallest subnormal
 *   0   mxfp4         1/2/1   1     2     6       0.5
 *   1   mxfp6_e2m3    1/2/3   1     2     7.5     0.125
 *   2   mxfp6_e3m2    1/3/2   3     4     28      2^-4
 *   3   mxfp8_e4m3    1/4/3   7     8     448     2^-9
 *   4   mxfp8_e5m2    1/5/2   15    15    57344   2^-16
 * Inputs are meant to be finite.  A block that holds a NaN or an infinity gets the scale code 255 and wq = NaN on every element; its
 * element codes are unspecified.  Other blocks are untouched.
 */
#ifndef RDO_PTQ_MX_H
#define RDO_PTQ_MX_H
#include "rdo_ptq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDO_MX_BLOCK 32
#define RDO_MX_FP4 0
#define RDO_MX_FP6_E2M3 1
#define RDO_MX_FP6_E3M2 2
#define RDO_MX_FP8_E4M3 3
#define RDO_MX_FP8_E5M2 4
#define RDO_MX_FORMATS 5

/* Quantise w fp32 [rows][inner] to `format`.  Each of the five outputs may be NULL, but not all of them:
 *   wq      fp32 [rows][inner]; may alias w
 *   scales  uint8 [rows][ceil(inner / 32)]
 *   codes   uint8 [rows][inner]
 *   err     double [rows] = sum_i d^2, d = w_i - wq_i formed in fp32, the square formed in double ((double)d * (double)d is exact)
 *   energy  double [rows] = sum_i w_i^2
 * The sums use no atomics and a fixed order: a block's 32 terms fold by xor-shuffles 16 .. 1, one wave per row then adds the blocks'
 * partials b, b + 64, .. ascending per lane and folds the 64 lanes by __shfl_down 32 .. 1.  The same input gives the same bits.
 * ws: rdo_mx_fakequant_workspace(rows, inner) bytes, 8-byte aligned, no initial state needed; read only when err or energy is
 * given (it may be NULL otherwise); err and energy 8-byte aligned.
 * RDO_EINVAL for rows <= 0, inner <= 0, an unknown format, all outputs NULL, w NULL or not 4-byte aligned, sums without ws. */
int rdo_mx_fakequant(const float* w, int32_t rows, int64_t inner, int32_t format, float* wq, uint8_t* scales, uint8_t* codes,
                     double* err, double* energy, void* ws, void* stream);
/* bytes (> 0 for every accepted geometry); 0 for rows <= 0, inner <= 0 or more than 2^40 blocks */
int64_t rdo_mx_fakequant_workspace(int32_t rows, int64_t inner);
/* fp32 [rows][inner] from codes uint8 [rows][inner] and scales uint8 [rows][ceil(inner / 32)]: bit for bit the wq of the call that
 * produced them.  A scale code of 255 gives NaN. */
int rdo_mx_dequant(const uint8_t* codes, const uint8_t* scales, int32_t rows, int64_t inner, int32_t format, float* w, void* stream);
/* element bits of a format id: 4 / 6 / 8, and 0 for an unknown id */
int32_t rdo_mx_format_bits(int32_t format);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MX_H */
