/*
 * rdo_ptq_pack.h -- C ABI of librdoptq_hip.so, continued: n-bit weight levels packed at their own width (csrc/weight_pack.hip).
 * Same conventions as rdo_ptq_hip.h (borrowed device pointers, hipStream_t as void*, integer status codes); a header of its own
 * because the export table of rdo_ptq_hip.h is closed (its symbol count is pinned by the suite).
 *
 * Bit layout (the one statement of it; quantization/packed_io.py and INTEGRATION.md refer here).  A level matrix [rows][inner] at width
 * b = bits, every level in [0, 2^b - 1]:
 *   - row r occupies W = ceil(inner * b / 32) 32-bit words, starting at word r * W (rdo_pack_row_words);
 *   - code i of the row is the bits [i * b, (i + 1) * b) of the row's bit string, its least significant bit first;
 *   - bit j of the string is bit j % 32 of word j / 32 (LSB first); in a file the words are little-endian, so bit j of the string is
 *     bit j % 8 of byte j / 8 of the row;
 *   - the 32 W - inner * b padding bits of a row's last word are zero;
 *   - bit offsets are computed in 64-bit.
 */
#ifndef RDO_PTQ_PACK_H
#define RDO_PTQ_PACK_H
#include "rdo_ptq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDO_PACK_MIN_BITS 2
#define RDO_PACK_MAX_BITS 16

/* Quantise a weight-row matrix to integer levels and pack them.  w fp32 [rows][inner] (the row matrix of a weight quantiser: rows =
 * quantisation channels), delta, zp fp32 [rows], packed uint32 [rows][W], 4-byte aligned; every word of it is written.
 *   alpha == NULL   level = clamp(rintf(w / delta) + zp, 0, 2^bits - 1): the integer inside rdo_uaq_fakequant
 *   alpha given     fp32 [rows][inner]: level = clamp(floorf(w / delta) + (alpha >= 0 ? 1 : 0) + zp, 0, 2^bits - 1): the integer inside
 *                   rdo_adaround_fwd with soft == 0
 * Both expressions are device functions of csrc/uaq_device.h.  One thread per output word: it forms the codes that overlap its word,
 * ORs their bits in and stores once -- no atomics, no two threads write one word, nothing beyond element inner - 1 of a row is read.
 * RDO_EINVAL before any launch for: a null w, delta, zp or packed; rows <= 0; inner <= 0; bits outside [2, 16]; a row of more than
 * 2^31 - 1 words; rows * W above 2^40 words; packed not 4-byte aligned. */
int rdo_weight_pack(const float* w, const float* alpha, const float* delta, const float* zp, int32_t rows, int64_t inner, int32_t bits,
                    uint32_t* packed, void* stream);

/* Unpack.  packed uint32 [rows][W]; levels int32 [rows][inner] or NULL; wq fp32 [rows][inner] or NULL: ((float)level - zp) * delta, the
 * tail expression of rdo_uaq_fakequant and rdo_adaround_fwd (fp32, unfused).  At least one of levels and wq; delta and zp fp32 [rows] may
 * be NULL only if wq is NULL.  One thread per code: it reads word k = (i * bits) >> 5, and word k + 1 only when
 * ((i * bits) & 31) + bits > 32 -- a word past the row's last is never read.  Refusals as rdo_weight_pack. */
int rdo_weight_unpack(const uint32_t* packed, const float* delta, const float* zp, int32_t rows, int64_t inner, int32_t bits,
                      int32_t* levels, float* wq, void* stream);

/* W = ceil(inner * bits / 32); 0 for inner <= 0, bits outside [2, 16] or a W above 2^31 - 1 */
int64_t rdo_pack_row_words(int64_t inner, int32_t bits);

#ifdef __cplusplus
}
#endif
#endif /* RDO_PTQ_PACK_H */
