/*
 * rdo_ptq_mxfile.h -- C ABI of librdoptq_hip.so, continued: the bytes a packed MX checkpoint stores for a weight, for rows of any length
 * (csrc/mx_container.hip).  Same conventions as rdo_ptq_mxgemm.h (borrowed device pointers, hipStream_t as void*, integer status codes;
 * every entry records into a plan); a header of its own because the export tables of the earlier headers are closed.
 *
 * Stored row.  A weight is its row matrix [rows][inner], inner >= 1, in the format `format` of rdo_ptq_mx.h with b = 4 / 6 / 8 element
 * bits.  A row is nb = ceil(inner / 32) blocks of 4 b bytes, block (r, kb) at byte (r * nb + kb) * 4 b; element j of a block (column
 * 32 kb + j) occupies bits [j b, (j + 1) b) of the block's little-endian bit string -- the packed operand of rdo_ptq_mxgemm.h.  The
 * last block of a row with inner % 32 != 0 is short: its missing elements are zero codes.  With it go the scales uint8 [rows][nb], the
 * E8M0 bytes of rdo_mx_fakequant.  For inner % 32 == 0 the rows are the operand of rdo_mx_pack_codes bit for bit, so a file's arrays
 * are what the block-scaled matrix instruction reads.
 *
 * Every entry but rdo_mx_row_bytes returns RDO_EINVAL, with a message that starts with its name, for: a NULL required pointer;
 * rows <= 0 or inner <= 0; an unknown format; a packed pointer that is not 4-byte aligned (w as well); more than 2^40 blocks.
 */
#ifndef RDO_PTQ_MXFILE_H
#define RDO_PTQ_MXFILE_H
#include "rdo_ptq_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of one stored row: ceil(inner / 32) * 4 b, for any inner >= 1; 0 for inner <= 0, an unknown format, or a count beyond int64_t */
int64_t rdo_mx_row_bytes(int64_t inner, int32_t format);

/* codes uint8 [rows][inner], one code per byte in the low b bits (upper bits are ignored) -> packed [rows][rdo_mx_row_bytes]; every
 * byte of packed is written, the padding of a short last block with zero bits */
int rdo_mx_pack_rows(const uint8_t* codes, int32_t rows, int64_t inner, int32_t format, void* packed, void* stream);

/* One launch from a file's bytes to the weight: packed [rows][rdo_mx_row_bytes] and scales uint8 [rows][ceil(inner / 32)] ->
 * w fp32 [rows][inner], bit for bit rdo_mx_dequant(codes, scales) (a scale code of 255 gives NaN), and codes uint8 [rows][inner] with
 * zero upper bits.  w and codes may each be NULL, but not both.  The padding of a short last block is read past, never written: both
 * outputs have exactly rows * inner elements. */
int rdo_mx_unpack_dequant(const void* packed, const uint8_t* scales, int32_t rows, int64_t inner, int32_t format, float* w,
                          uint8_t* codes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_MXFILE_H */
