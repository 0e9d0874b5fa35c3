// The bit placement of one MX block (include/rdo_ptq_mxgemm.h: element j of a block in bits [j b, (j + 1) b) of the block's little-endian
// bit string, b = 4 / 6 / 8, the string read as b dwords), packing and unpacking, for a block that may be short (the last block of a
// ragged row: n < 32 elements, the missing ones zero codes).  Plain integer C++ without a HIP header, so that a host program can run
// the very functions the kernels of mx_container.hip call (tools/mx_block_bits_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RDO_MXBITS_HD __host__ __device__ __forceinline__
#else
#define RDO_MXBITS_HD inline
#endif

// dword d (0 <= d < bits) of the block whose elements are codes[0 .. n), 1 <= n <= 32, one code per byte (upper bits ignored).
// Reads codes[j] for j < n only.
RDO_MXBITS_HD uint32_t mx_block_word(const uint8_t* codes, int n, int bits, int d) {
    const uint32_t mask = (1u << bits) - 1u;
    const int first = (32 * d) / bits;                                          // the first element that reaches into dword d
    uint32_t word = 0u;
    for (int i = 0; i < 8; ++i) {                                               // FP4: eight elements a dword, FP6: up to seven, FP8: four
        const int j = first + i;
        const int pos = j * bits - 32 * d;
        if (j < 32 && pos < 32) {
            const uint32_t c = j < n ? (uint32_t)codes[j] & mask : 0u;
            word |= pos >= 0 ? c << pos : c >> (-pos);
        }
    }
    return word;
}

// element j (0 <= j < 32) of the block whose dwords are words[0 .. bits): reads inside the block only (its last element ends on its end)
RDO_MXBITS_HD uint32_t mx_block_element(const uint32_t* words, int bits, int j) {
    const int at = j * bits, d = at >> 5, s = at & 31;
    uint32_t v = words[d] >> s;
    if (s + bits > 32) v |= words[d + 1] << (32 - s);
    return v & ((1u << bits) - 1u);
}
