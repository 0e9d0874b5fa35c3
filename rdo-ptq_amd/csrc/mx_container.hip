// The bytes a packed MX checkpoint stores for a weight (include/rdo_ptq_mxfile.h): the packed operand of rdo_ptq_mxgemm.h for rows of
// any length, and one launch from those bytes and the E8M0 scales back to the fp32 weight.  Built with -ffp-contract=off like the other
// MX files; no floating-point operation decides a bit here: the weight is put together as an fp32 bit pattern by mx_decode.
//
// Pack: one thread per dword of the packed image, a grid-stride loop over rows * nb * b dwords.  The thread reads the up to eight codes
// that reach into its dword straight from the row (byte loads; a code is read by at most two threads) and stores the dword: no
// shuffles, so a short last block only shortens the reads (mx_block_word takes the count n of live elements), and every dword of the
// image is written, the padding with zero bits.
// Unpack + dequant: the layout of mx_dequant_kernel, a block is 32 lanes and a workgroup of 256 threads eight blocks, grid-stride over
// (row, block) pairs.  Lane l reads the one or two dwords of its block that hold element l (mx_block_element: never past the block),
// the block's scale byte, and writes element 32 kb + l of the row to w and / or codes; lanes past the end of a short last block do
// nothing.  Nothing assumes more than the 4-byte alignment of packed: a row is a whole number of dwords.
// These operands are weights, a few MB at the most: a call measures enqueue rate, and no timing claim is made.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxfile.h"
#include "mx_device.h"
#include "mx_block_bits.h"

namespace {

__global__ __launch_bounds__(256) void mx_pack_rows_kernel(const uint8_t* __restrict__ codes, long words, long nb, long inner, int bits,
                                                           uint32_t* __restrict__ packed) {
    const long stride = (long)gridDim.x * 256;
    for (long at = (long)blockIdx.x * 256 + threadIdx.x; at < words; at += stride) {
        const long g = at / bits;
        const int d = (int)(at - g * bits);
        const long row = g / nb, kb = g - row * nb;
        const long left = inner - kb * kBlock;                                  // >= 1: kb < nb = ceil(inner / 32)
        packed[at] = mx_block_word(codes + row * inner + kb * kBlock, left < kBlock ? (int)left : kBlock, bits, d);
    }
}

__global__ __launch_bounds__(256) void mx_unpack_dequant_kernel(const uint32_t* __restrict__ packed, const uint8_t* __restrict__ scales,
                                                                long total, long nb, long inner, MxFormat f, float* __restrict__ w,
                                                                uint8_t* __restrict__ codes) {
    const int lane = threadIdx.x & 31;
    const long stride = (long)gridDim.x * 8;
    for (long g = (long)blockIdx.x * 8 + (threadIdx.x >> 5); g < total; g += stride) {
        const long row = g / nb, kb = g - row * nb;
        const long i = kb * kBlock + lane;
        if (i >= inner) continue;
        const long at = row * inner + i;
        const unsigned c = mx_block_element(packed + g * f.bits, f.bits, lane);
        if (codes) codes[at] = (uint8_t)c;
        if (w) {
            const unsigned sc = scales[g];
            const unsigned sign = (c >> (f.bits - 1)) & 1u, magc = c & ((1u << (f.bits - 1)) - 1u);
            const unsigned qbits = sc == 255u ? 0x7FC00000u : (mx_decode(magc, (int)sc - 127, f) | (sign << 31));
            w[at] = __builtin_bit_cast(float, qbits);
        }
    }
}

inline bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace

// the argument checks both launching entries share: sizes, the format, the block count
#define RDO_MXF_GEOMETRY(who, rows, inner, format, f, nb, total)                                                                    \
    RDO_REQUIRE((rows) > 0 && (inner) > 0, who ": non-positive size rows %d inner %lld", (int)(rows), (long long)(inner));          \
    MxFormat f;                                                                                                                     \
    RDO_REQUIRE(mx_format(format, f), who ": unknown format %d (0 .. %d)", (int)(format), RDO_MX_FORMATS - 1);                      \
    long nb = 0;                                                                                                                    \
    const long total = mx_blocks(rows, inner, nb);                                                                                  \
    RDO_REQUIRE(total > 0, who ": rows %d of inner %lld make more than 2^40 blocks", (int)(rows), (long long)(inner))

extern "C" {

int64_t rdo_mx_row_bytes(int64_t inner, int32_t format) {
    MxFormat f;
    if (inner <= 0 || !mx_format(format, f)) return 0;
    const int64_t nb = (inner - 1) / kBlock + 1;                                // (no inner + 31: inner may be INT64_MAX)
    return nb > INT64_MAX / (4 * f.bits) ? 0 : nb * 4 * f.bits;
}

int rdo_mx_pack_rows(const uint8_t* codes, int32_t rows, int64_t inner, int32_t format, void* packed, void* stream) {
    RDO_REQUIRE(codes && packed, "rdo_mx_pack_rows: null pointer");
    RDO_MXF_GEOMETRY("rdo_mx_pack_rows", rows, inner, format, f, nb, total);
    RDO_REQUIRE(aligned4(packed), "rdo_mx_pack_rows: packed must be 4-byte aligned");
    const int bits = f.bits;
    const long in = (long)inner, words = total * bits;                          // <= 2^43
    uint32_t* out = static_cast<uint32_t*>(packed);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_pack_rows_kernel, dim3(rdo::grid_for(words)), dim3(256), 0, s, codes, words, nb, in, bits, out);
            return rdo::check_launch("mx_pack_rows");
        },
        stream, "mx_pack_rows", 0.0, (double)rows * (double)inner + (double)words * 4.0);
}

int rdo_mx_unpack_dequant(const void* packed, const uint8_t* scales, int32_t rows, int64_t inner, int32_t format, float* w,
                          uint8_t* codes, void* stream) {
    RDO_REQUIRE(packed && scales, "rdo_mx_unpack_dequant: null pointer");
    RDO_REQUIRE(w || codes, "rdo_mx_unpack_dequant: both outputs w and codes are NULL");
    RDO_MXF_GEOMETRY("rdo_mx_unpack_dequant", rows, inner, format, f, nb, total);
    RDO_REQUIRE(aligned4(packed) && aligned4(w), "rdo_mx_unpack_dequant: packed and w must be 4-byte aligned");
    const long in = (long)inner;
    const uint32_t* src = static_cast<const uint32_t*>(packed);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_unpack_dequant_kernel, dim3(mx_grid(total)), dim3(256), 0, s, src, scales, total, nb, in, f, w, codes);
            return rdo::check_launch("mx_unpack_dequant");
        },
        stream, "mx_unpack_dequant", 0.0, (double)total * (4.0 * f.bits + 1.0) + (double)rows * (double)inner * ((w ? 4.0 : 0.0) + (codes ? 1.0 : 0.0)));
}

}  // extern "C"
