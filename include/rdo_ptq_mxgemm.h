/*
 * rdo_ptq_mxgemm.h -- C ABI of librdoptq_hip.so, continued: the MX codes of rdo_ptq_mx.h / rdo_ptq_mxround.h as operands of the MI355X's
 * block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 (csrc/mx_gemm.hip).  Same conventions as rdo_ptq_hip.h (borrowed
 * device pointers, hipStream_t as void*, integer status codes; every entry records into a plan); a header of its own because the export
 * tables of the earlier headers are closed (their symbol sets are pinned by the suite).
 *
 * Packed operand.  A matrix [rows][K], K % 32 == 0, in the format `format` of rdo_ptq_mx.h with b = 4 / 6 / 8 element bits:
 *   elements  [rows][K / 32] blocks of 4 b bytes (16 / 24 / 32), block (r, kb) at byte (r * K / 32 + kb) * 4 b;
 *             element j of the block (column 32 kb + j) occupies bits [j b, (j + 1) b) of the block's little-endian bit string:
 *             bit i of the string is bit i % 8 of byte i / 8.  FP8: byte j.  FP4: the low nibble of byte j / 2 for even j, the high
 *             nibble for odd j.  FP6: four codes in three bytes, the first code in the low six bits of the first byte.
 *   scales    uint8 [rows][K / 32], the E8M0 bytes rdo_mx_fakequant writes (E + 127); it is the instruction's own scale code.
 * What the instruction takes, as the exact-product test established on the hardware (tests/test_gpu_mx_gemm.py: all 25 format pairs,
 * a scale of its own on every block, A and B drawn independently): lane l of a wave serves row l & 15 of a 16-row tile and k group
 * g = l >> 4 of a 128-wide K step, and holds the scale of block g of the step in byte 0 of its scale VGPR, for every format.
 *   FP4, FP6  the lane's 4 / 6 operand VGPRs are block g itself, dword d of the block in VGPR d: the byte image above is the register
 *             image, FP6 in the same dense order as FP4.
 *   FP8       the lane's 8 operand VGPRs are two half blocks: VGPRs 0 .. 3 hold elements 16 g .. 16 g + 15 of the step, VGPRs 4 .. 7
 *             elements 64 + 16 g .. 64 + 16 g + 15, byte j of a VGPR quadruple being element j of its sixteen (the scales still go by
 *             block: elements 32 g .. 32 g + 31 are scaled by lane g's byte).  Contiguous blocks of 32 per lane give right FP8 x FP8
 *             products only under uniform scales and wrong ones against an FP4 / FP6 operand.
 * In every case a lane loads its operand from the packed image with dword loads (one run of 4 / 6 dwords, or two runs of 4) and moves
 * no bit.
 * The instruction numbers the element formats {0 E4M3, 1 E5M2, 2 E2M3, 3 E3M2, 4 FP4}; the entries take this project's ids
 * (RDO_MX_FP4 = 0 .. RDO_MX_FP8_E5M2 = 4) and map them.
 *
 * Every entry returns RDO_EINVAL, with a message that starts with its name, for: a NULL required pointer; rows / M / N <= 0 or K <= 0;
 * K % 32 != 0; an unknown format; a packed or fp32 pointer that is not 4-byte aligned; more than 2^40 blocks in one operand.
 * A scale code of 255 (a block that held a non-finite value) leaves every output that sums over that block unspecified; every other
 * output is unaffected.
 */
#ifndef RDO_PTQ_MXGEMM_H
#define RDO_PTQ_MXGEMM_H
#include "rdo_ptq_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the packed elements of [rows][K]: rows * (K / 32) * 4 b; 0 for a refused geometry or format */
int64_t rdo_mx_packed_bytes(int32_t rows, int64_t K, int32_t format);

/* codes uint8 [rows][K], one code per byte in the low b bits (what rdo_mx_fakequant and rdo_mx_round_fwd write; upper bits are
 * ignored) -> packed.  The weight side, learned rounding included. */
int rdo_mx_pack_codes(const uint8_t* codes, int32_t rows, int64_t K, int32_t format, void* packed, void* stream);

/* The activation-side producer: x fp32 [rows][K] -> packed elements and scales uint8 [rows][K / 32] in one read of x; xq (nullable)
 * fp32 [rows][K], the decoded values.  packed and scales are bit for bit rdo_mx_fakequant(codes, scales) followed by
 * rdo_mx_pack_codes, xq is its wq (NaN on a block that is not finite, scale code 255, element codes 0). */
int rdo_mx_quant_pack(const float* x, int32_t rows, int64_t K, int32_t format, void* packed, uint8_t* scales, float* xq, void* stream);

/* packed -> codes uint8 [rows][K]: the inverse of rdo_mx_pack_codes */
int rdo_mx_unpack_codes(const void* packed, int32_t rows, int64_t K, int32_t format, uint8_t* codes, void* stream);

/* y fp32 [M][N] = sum_k A[m][k] B[n][k] (+ bias[n]); a packed [M][K] in a_format with a_scales uint8 [M][K / 32], b packed [N][K] in
 * b_format with b_scales uint8 [N][K / 32]; any of the 5 x 5 format pairs; bias fp32 [N], nullable.  The sum is the instruction's:
 * dependent steps per output, an fp32 sum of exact products within K 2^-23 (sum |a b| + |bias|) of the real sum for every format
 * pair (measured: the error of a k-ordered fp32 chain).  For an FP8 operand that takes care: given eight neighbouring FP8 products
 * the instruction adds them aligned to the largest and drops what lies more than about 14 bits below it (448 + 2^-6 comes out 448;
 * measured on Student-t rows: up to 7.7e-5 of sum |a b|), so a pair with an FP8 operand runs eight instructions per K step, each with
 * one element of every eight of one FP8 operand kept and the rest cleared: every such sum then holds a single product.
 * Also RDO_EINVAL for more than 2^31 - 1 output tiles of 64 x 64. */
int rdo_mx_gemm(const void* a, const uint8_t* a_scales, int32_t a_format, const void* b, const uint8_t* b_scales, int32_t b_format,
                int32_t M, int32_t N, int64_t K, const float* bias, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXGEMM_H */
