// MX codes as operands of the block-scaled matrix instruction (include/rdo_ptq_mxgemm.h): the packed operand format, its producers
// (pack the one-code-per-byte weights; quantise-and-pack fp32 activation rows), the inverse, and the GEMM on
// v_mfma_scale_f32_16x16x128_f8f6f4.  Built with -ffp-contract=off like mx_quant.hip; the cast, the format table, the block amax and
// floor_log2_bits are mx_device.h's.
//
// Producers: K % 32 == 0, so the blocks of a [rows][K] matrix are contiguous and a call is a flat run of `total` blocks: block g holds
// elements 32 g .. 32 g + 31, its scale is scales[g], its packed image the dwords g b .. g b + b - 1 (b = element bits).  The layout of
// mx_fakequant_kernel: a block is 32 lanes, a wave handles two, a workgroup of 256 threads eight, grid-stride over blocks.  After the
// amax shuffles every lane holds its element's code; lane t < b of the block then gathers the (at most eight) codes that touch dword t
// of the block's bit string by __shfl and stores that one dword: b lanes of 32 write, 4-byte stores, no byte traffic.
//
// GEMM: no LDS.  One wave owns a 32 x 32 output (2 x 2 tiles of 16 x 16), a workgroup of four waves 64 x 64.  Per K step of 128 (four
// blocks) lane l = (row l & 15, k group l >> 4) loads, for each of its two A tiles and two B tiles, its operand registers with dword
// loads that move no bit -- FP4 / FP6: the 4 / 6 consecutive dwords of block (row, k group); FP8: the instruction wants two half blocks
// per lane (load_fragment states which), 4 consecutive dwords each -- and the scale byte of block (row, k group); each fragment feeds
// two MFMAs.  A lane whose row is past M / N feeds zero registers, a block past K / 32 is zeros under the scale 127.
// A pair with an FP8 operand issues eight MFMAs where the others issue one (keep_one_of_eight and the comment in the K loop say why):
// the instruction's own sum over eight neighbouring FP8 products drops small ones, one product per sum drops nothing.
// C/D: col = lane & 15, row = 4 (lane >> 4) + reg.
// The kernel is a template over the (A, B) formats, whose numbers are immediates of the instruction: 25 instantiations.
// load_fragment, keep_one_of_eight, the K step and the store are mx_mfma_device.h's, shared with the convolution (mx_conv.hip).
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxgemm.h"
#include "mx_mfma_device.h"

namespace {

// ---- packed operand -----------------------------------------------------------------------------------------------------------------
// Called by all 64 lanes.  `code` (b bits) is the element `lane` of this half-wave's block; lane t < b puts together dword t of the
// block's little-endian bit string (element j at bits [j b, (j + 1) b)) and stores it.
__device__ __forceinline__ void store_block(unsigned code, int lane, int bits, uint32_t* dst, bool live) {
    const int half_base = threadIdx.x & 32;
    const int first = (32 * lane) / bits;                                       // the first element that reaches into dword `lane`
    unsigned word = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {                                               // FP4: eight elements a dword, FP6: up to seven, FP8: four
        const int j = first + i;
        const unsigned c = __shfl(code, half_base + (j & 31), 64);
        const int pos = j * bits - 32 * lane;
        if (j < 32 && pos < 32) word |= pos >= 0 ? c << pos : c >> (-pos);
    }
    if (live && lane < bits) dst[lane] = word;
}

__global__ __launch_bounds__(256) void mx_pack_codes_kernel(const uint8_t* __restrict__ codes, long total, int bits,
                                                            uint32_t* __restrict__ packed) {
    const int lane = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const long stride = (long)gridDim.x * 8;
    for (long base = (long)blockIdx.x * 8 + ((threadIdx.x >> 6) << 1); base < total; base += stride) {     // uniform over the wave
        const long g = base + half;
        const bool live = g < total;
        const unsigned code = live ? (unsigned)codes[g * kBlock + lane] & ((1u << bits) - 1u) : 0u;
        store_block(code, lane, bits, packed + g * bits, live);
    }
}

__global__ __launch_bounds__(256) void mx_unpack_codes_kernel(const uint32_t* __restrict__ packed, long total, int bits,
                                                              uint8_t* __restrict__ codes) {
    const int lane = threadIdx.x & 31;
    const long stride = (long)gridDim.x * 8;
    for (long g = (long)blockIdx.x * 8 + (threadIdx.x >> 5); g < total; g += stride) {
        const uint32_t* p = packed + g * bits;
        const int at = lane * bits, d = at >> 5, s = at & 31;
        unsigned v = p[d] >> s;
        if (s + bits > 32) v |= p[d + 1] << (32 - s);                           // (never past the block: its last element ends on its end)
        codes[g * kBlock + lane] = (uint8_t)(v & ((1u << bits) - 1u));
    }
}

// mx_fakequant_kernel's element arithmetic on a flat run of whole blocks, the codes going into the packed image
__global__ __launch_bounds__(256) void mx_quant_pack_kernel(const float* __restrict__ x, long total, MxFormat f, uint32_t* __restrict__ packed,
                                                            uint8_t* __restrict__ scales, float* __restrict__ xq) {
    const int lane = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const long stride = (long)gridDim.x * 8;
    for (long base = (long)blockIdx.x * 8 + ((threadIdx.x >> 6) << 1); base < total; base += stride) {     // uniform over the wave
        const long g = base + half;
        const bool live = g < total;
        const long at = g * kBlock + lane;
        const unsigned bits = live ? __builtin_bit_cast(unsigned, x[at]) : 0u;
        const unsigned mag = bits & 0x7FFFFFFFu;
        const unsigned amax = half_wave_max(mag);
        const bool finite = amax < 0x7F800000u;
        const int E = finite ? mx_block_exponent(amax, f) : -127;
        unsigned code = 0u, qbits = 0x7FC00000u;
        if (finite) {
            const unsigned c = mx_encode(mag, E, f);
            const unsigned sign = bits & 0x80000000u;
            code = c | (sign >> (32 - f.bits));
            qbits = mx_decode(c, E, f) | sign;
        }
        if (live) {
            if (xq) xq[at] = __builtin_bit_cast(float, qbits);
            if (lane == 0) scales[g] = (uint8_t)(finite ? E + 127 : 255);
        }
        store_block(code, lane, f.bits, packed + g * f.bits, live);
    }
}

// ---- the GEMM -----------------------------------------------------------------------------------------------------------------------
template <int FA, int FB>
__global__ __launch_bounds__(256) void mx_gemm_kernel(const uint32_t* __restrict__ a, const uint8_t* __restrict__ sa,
                                                      const uint32_t* __restrict__ b, const uint8_t* __restrict__ sb, int M, int N, long nb,
                                                      int tiles_n, const float* __restrict__ bias, float* __restrict__ y) {
    constexpr int DA = hw_dwords(FA), DB = hw_dwords(FB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kg = lane >> 4;
    const long tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const long m0 = tm * 64 + (wave >> 1) * 32, n0 = tn * 64 + (wave & 1) * 32;
    if (m0 >= M || n0 >= N) return;                                             // uniform over the wave; the kernel has no barrier
    long arow[2], brow[2];
    bool aok[2], bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        aok[i] = m0 + 16 * i + r < M;
        bok[i] = n0 + 16 * i + r < N;
        arow[i] = (m0 + 16 * i + r) * nb;
        brow[i] = (n0 + 16 * i + r) * nb;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long k0 = 0; k0 < nb; k0 += 4) {
        const long kb = k0 + kg;
        const bool kok = kb < nb;
        i32x8 fa[2], fb[2];
        int xa[2], xb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fa[i] = load_fragment<DA>(a + arow[i] * DA, k0, kg, nb, aok[i]);
            fb[i] = load_fragment<DB>(b + brow[i] * DB, k0, kg, nb, bok[i]);
            xa[i] = aok[i] && kok ? (int)sa[arow[i] + kb] : 127;
            xb[i] = bok[i] && kok ? (int)sb[brow[i] + kb] : 127;
        }
        mx_mfma_step<FA, FB>(fa, fb, xa, xb, acc);
    }
    mx_store_tiles(acc, bias, y, m0, n0, M, N, r, kg);
}

using GemmKernel = void (*)(const uint32_t*, const uint8_t*, const uint32_t*, const uint8_t*, int, int, long, int, const float*, float*);

#define RDO_MXG_ROW(FA) {mx_gemm_kernel<FA, 0>, mx_gemm_kernel<FA, 1>, mx_gemm_kernel<FA, 2>, mx_gemm_kernel<FA, 3>, mx_gemm_kernel<FA, 4>}
const GemmKernel kGemm[5][5] = {RDO_MXG_ROW(0), RDO_MXG_ROW(1), RDO_MXG_ROW(2), RDO_MXG_ROW(3), RDO_MXG_ROW(4)};
#undef RDO_MXG_ROW

// blocks of a packed [rows][K]; 0 for a refused geometry
inline long packed_blocks(int32_t rows, int64_t K) {
    if (K <= 0 || K % kBlock != 0) return 0;
    long nb = 0;
    return mx_blocks(rows, K, nb);
}

}  // namespace

// the argument checks every entry shares: sizes, K % 32, the format, the block count
#define RDO_MXG_GEOMETRY(who, rows, K, format, f, total)                                                                            \
    RDO_REQUIRE((rows) > 0 && (K) > 0, who ": non-positive size rows %d K %lld", (int)(rows), (long long)(K));                      \
    RDO_REQUIRE((K) % kBlock == 0, who ": K %lld is no multiple of the block size %d", (long long)(K), kBlock);                     \
    MxFormat f;                                                                                                                     \
    RDO_REQUIRE(mx_format(format, f), who ": unknown format %d (0 .. %d)", (int)(format), RDO_MX_FORMATS - 1);                      \
    const long total = packed_blocks(rows, K);                                                                                      \
    RDO_REQUIRE(total > 0, who ": rows %d of K %lld make more than 2^40 blocks", (int)(rows), (long long)(K))

extern "C" {

int64_t rdo_mx_packed_bytes(int32_t rows, int64_t K, int32_t format) {
    MxFormat f;
    if (!mx_format(format, f)) return 0;
    return packed_blocks(rows, K) * 4 * f.bits;
}

int rdo_mx_pack_codes(const uint8_t* codes, int32_t rows, int64_t K, int32_t format, void* packed, void* stream) {
    RDO_REQUIRE(codes && packed, "rdo_mx_pack_codes: null pointer");
    RDO_MXG_GEOMETRY("rdo_mx_pack_codes", rows, K, format, f, total);
    RDO_REQUIRE(aligned4(packed), "rdo_mx_pack_codes: packed must be 4-byte aligned");
    const int bits = f.bits;
    uint32_t* out = static_cast<uint32_t*>(packed);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_pack_codes_kernel, dim3(mx_grid(total)), dim3(256), 0, s, codes, total, bits, out);
            return rdo::check_launch("mx_pack_codes");
        },
        stream, "mx_pack_codes", 0.0, (double)total * (32.0 + 4.0 * bits));
}

int rdo_mx_unpack_codes(const void* packed, int32_t rows, int64_t K, int32_t format, uint8_t* codes, void* stream) {
    RDO_REQUIRE(codes && packed, "rdo_mx_unpack_codes: null pointer");
    RDO_MXG_GEOMETRY("rdo_mx_unpack_codes", rows, K, format, f, total);
    RDO_REQUIRE(aligned4(packed), "rdo_mx_unpack_codes: packed must be 4-byte aligned");
    const int bits = f.bits;
    const uint32_t* in = static_cast<const uint32_t*>(packed);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_unpack_codes_kernel, dim3(mx_grid(total)), dim3(256), 0, s, in, total, bits, codes);
            return rdo::check_launch("mx_unpack_codes");
        },
        stream, "mx_unpack_codes", 0.0, (double)total * (32.0 + 4.0 * bits));
}

int rdo_mx_quant_pack(const float* x, int32_t rows, int64_t K, int32_t format, void* packed, uint8_t* scales, float* xq, void* stream) {
    RDO_REQUIRE(x && packed && scales, "rdo_mx_quant_pack: null pointer");
    RDO_MXG_GEOMETRY("rdo_mx_quant_pack", rows, K, format, f, total);
    RDO_REQUIRE(aligned4(x) && aligned4(packed) && aligned4(xq), "rdo_mx_quant_pack: x, packed and xq must be 4-byte aligned");
    uint32_t* out = static_cast<uint32_t*>(packed);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_quant_pack_kernel, dim3(mx_grid(total)), dim3(256), 0, s, x, total, f, out, scales, xq);
            return rdo::check_launch("mx_quant_pack");
        },
        stream, "mx_quant_pack", 0.0, (double)total * (128.0 + 4.0 * f.bits + 1.0 + (xq ? 128.0 : 0.0)));
}

int rdo_mx_gemm(const void* a, const uint8_t* a_scales, int32_t a_format, const void* b, const uint8_t* b_scales, int32_t b_format,
                int32_t M, int32_t N, int64_t K, const float* bias, float* y, void* stream) {
    RDO_REQUIRE(a && a_scales && b && b_scales && y, "rdo_mx_gemm: null pointer");
    RDO_MXG_GEOMETRY("rdo_mx_gemm", M, K, a_format, fa, total_a);
    RDO_MXG_GEOMETRY("rdo_mx_gemm", N, K, b_format, fb, total_b);
    RDO_REQUIRE(aligned4(a) && aligned4(b) && aligned4(bias) && aligned4(y), "rdo_mx_gemm: a, b, bias and y must be 4-byte aligned");
    const long tiles_m = rdo::ceil_div(M, 64), tiles_n = rdo::ceil_div(N, 64);
    RDO_REQUIRE(tiles_m * tiles_n <= 0x7fffffffL, "rdo_mx_gemm: M %d x N %d make more than 2^31 - 1 output tiles", M, N);
    const GemmKernel kern = kGemm[hw_format(a_format)][hw_format(b_format)];
    const uint32_t* pa = static_cast<const uint32_t*>(a);
    const uint32_t* pb = static_cast<const uint32_t*>(b);
    const long nb = (long)(K / kBlock);
    const int tn = (int)tiles_n;
    const unsigned grid = (unsigned)(tiles_m * tiles_n);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, pa, a_scales, pb, b_scales, M, N, nb, tn, bias, y);
            return rdo::check_launch("mx_gemm");
        },
        stream, "mx_gemm", 2.0 * (double)M * (double)N * (double)K,
        (double)total_a * (4.0 * fa.bits + 1.0) + (double)total_b * (4.0 * fb.bits + 1.0) + (double)M * (double)N * 4.0);
}

}  // extern "C"
