// n-bit weight levels packed at their own width (include/rdo_ptq_pack.h, which states the bit layout): what a packed checkpoint stores.
// Built with -ffp-contract=off (the level and dequantisation expressions round as in adaround.hip; all take them from uaq_device.h).
//
// rdo_weight_pack.  One thread per OUTPUT word (k of row r): the codes that overlap the bits [32 k, 32 k + 32) of the row's bit string
// are i0 = 32 k / b .. i1 = min(inner - 1, (32 k + 31) / b); the thread forms each one's level, shifts it to its place (left by
// i b - 32 k >= 0, or right by 32 k - i b for the code that began in the word before) and ORs it in.  A code that straddles two words is
// formed by both their threads -- the weight is read twice, from the same cache line -- so no two threads write one word and nothing is
// atomic.  i1 <= inner - 1 keeps every read inside the row, and the bits of the last word past inner * b stay zero.
// rdo_weight_unpack.  One thread per code i of row r: word k = (i b) >> 5 shifted right by s = (i b) & 31, and, only when s + b > 32, word
// k + 1 shifted left by 32 - s.  The last bit of code i is bit i b + b - 1 <= inner b - 1 < 32 W of the row, so word k + 1 is read only
// where it belongs to the row.
// Both kernels are launch-latency sized for the weights of a codec (a 192 x 1728 weight is 1.3 MB); nothing is staged in LDS.
#include "rdo_common.h"
#include "uaq_device.h"
#include "../../include/rdo_ptq_pack.h"

namespace {

constexpr int kMinBits = RDO_PACK_MIN_BITS, kMaxBits = RDO_PACK_MAX_BITS;
constexpr int64_t kMaxRowWords = 0x7fffffffLL;
constexpr int64_t kMaxWords = 1LL << 40;
constexpr int64_t kMaxBlocks = 1LL << 23;                  // 2^31 threads: beyond that the grid-stride loop covers the rest

inline int64_t row_words(int64_t inner, int32_t bits) {
    if (inner <= 0 || bits < kMinBits || bits > kMaxBits) return 0;
    if (inner > kMaxRowWords * 32 / bits) return 0;        // (also keeps inner * bits inside 64 bits)
    return (inner * bits + 31) / 32;
}

inline unsigned blocks_for(int64_t n) {
    const int64_t g = rdo::ceil_div(n, 256);
    return (unsigned)(g > kMaxBlocks ? kMaxBlocks : g);
}

__global__ __launch_bounds__(256) void weight_pack_kernel(const float* __restrict__ w, const float* __restrict__ alpha,
                                                          const float* __restrict__ delta, const float* __restrict__ zp, long rows, long inner,
                                                          int bits, long W, uint32_t* __restrict__ packed) {
    const float Lm1 = (float)((1 << bits) - 1);
    const long total = rows * W;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
        const long r = g / W, k = g - r * W;
        const long bit0 = 32 * k;                          // the word holds the bits [bit0, bit0 + 32) of the row
        const long i0 = bit0 / bits;
        long i1 = (bit0 + 31) / bits;
        if (i1 > inner - 1) i1 = inner - 1;
        const float dl = delta[r], z = zp[r];
        const float* wr = w + r * inner;
        const float* ar = alpha ? alpha + r * inner : nullptr;
        uint32_t word = 0u;
        for (long i = i0; i <= i1; ++i) {
            const float lv = ar ? rdo::uaq_level_hard(wr[i], ar[i], dl, z, Lm1) : rdo::uaq_level_nearest(wr[i], dl, z, Lm1);
            const uint32_t code = (uint32_t)lv;            // an integer in [0, 2^bits - 1] (a NaN clamps to 0)
            const long off = i * bits - bit0;              // in (-bits, 32)
            word |= off >= 0 ? code << off : code >> -off;
        }
        packed[g] = word;
    }
}

__global__ __launch_bounds__(256) void weight_unpack_kernel(const uint32_t* __restrict__ packed, const float* __restrict__ delta,
                                                            const float* __restrict__ zp, long rows, long inner, int bits, long W,
                                                            int32_t* __restrict__ levels, float* __restrict__ wq) {
    const uint32_t mask = (1u << bits) - 1u;
    const long total = rows * inner;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / inner, i = e - r * inner;
        const long bit = i * bits;
        const long k = bit >> 5;
        const int s = (int)(bit & 31);
        const uint32_t* pr = packed + r * W;
        uint32_t v = pr[k] >> s;
        if (s + bits > 32) v |= pr[k + 1] << (32 - s);      // s > 16 here: the shift is in [1, 15]
        const uint32_t code = v & mask;
        if (levels) levels[e] = (int32_t)code;
        if (wq) wq[e] = rdo::uaq_dequant((float)code, delta[r], zp[r]);
    }
}

// the refusals both entries share; W is set for an accepted geometry
int check_geometry(const char* who, int32_t rows, int64_t inner, int32_t bits, const void* packed, int64_t* W) {
    RDO_REQUIRE(rows > 0 && inner > 0, "%s: non-positive size rows %d inner %lld", who, rows, (long long)inner);
    RDO_REQUIRE(bits >= kMinBits && bits <= kMaxBits, "%s: bits %d outside [%d, %d]", who, bits, kMinBits, kMaxBits);
    *W = row_words(inner, bits);
    RDO_REQUIRE(*W > 0, "%s: a row of inner %lld at %d bits is more than 2^31 - 1 words", who, (long long)inner, bits);
    RDO_REQUIRE((int64_t)rows * *W <= kMaxWords, "%s: rows %d of %lld words are more than 2^40 words", who, rows, (long long)*W);
    RDO_REQUIRE(reinterpret_cast<uintptr_t>(packed) % 4 == 0, "%s: packed must be 4-byte aligned", who);
    return RDO_OK;
}

}  // namespace

extern "C" {

int64_t rdo_pack_row_words(int64_t inner, int32_t bits) { return row_words(inner, bits); }

int rdo_weight_pack(const float* w, const float* alpha, const float* delta, const float* zp, int32_t rows, int64_t inner, int32_t bits,
                    uint32_t* packed, void* stream) {
    RDO_REQUIRE(w && delta && zp && packed, "rdo_weight_pack: null pointer");
    int64_t W = 0;
    if (int rc = check_geometry("rdo_weight_pack", rows, inner, bits, packed, &W)) return rc;
    const int64_t words = (int64_t)rows * W;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(weight_pack_kernel, dim3(blocks_for(words)), dim3(256), 0, s, w, alpha, delta, zp, (long)rows, (long)inner, (int)bits,
                               (long)W, packed);
            return rdo::check_launch("weight_pack");
        },
        stream, "weight_pack", 0.0, (alpha ? 8.0 : 4.0) * (double)rows * (double)inner + 4.0 * (double)words);
}

int rdo_weight_unpack(const uint32_t* packed, const float* delta, const float* zp, int32_t rows, int64_t inner, int32_t bits,
                      int32_t* levels, float* wq, void* stream) {
    RDO_REQUIRE(packed, "rdo_weight_unpack: null pointer");
    RDO_REQUIRE(levels || wq, "rdo_weight_unpack: at least one of levels and wq must be given");
    RDO_REQUIRE(!wq || (delta && zp), "rdo_weight_unpack: wq needs delta and zp");
    int64_t W = 0;
    if (int rc = check_geometry("rdo_weight_unpack", rows, inner, bits, packed, &W)) return rc;
    const int64_t codes = (int64_t)rows * inner;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(weight_unpack_kernel, dim3(blocks_for(codes)), dim3(256), 0, s, packed, delta, zp, (long)rows, (long)inner,
                               (int)bits, (long)W, levels, wq);
            return rdo::check_launch("weight_unpack");
        },
        stream, "weight_unpack", 0.0, 4.0 * (double)rows * (double)W + ((levels ? 4.0 : 0.0) + (wq ? 4.0 : 0.0)) * (double)codes);
}

}  // extern "C"
