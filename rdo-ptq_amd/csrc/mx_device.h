// What mx_quant.hip (round to nearest) and mx_round.hip (learned rounding) share of the MX block formats: the format table, the integer
// cast between an fp32 bit pattern and a magnitude code, and the half-wave fold of a block.  Plain integer C++: the cast functions run
// on the host as well as on the device.  Included once per translation unit, hence the unnamed namespace.
#pragma once
#include "rdo_common.h"
#include "../../include/rdo_ptq_mx.h"

namespace {

constexpr int kBlock = RDO_MX_BLOCK;
constexpr long kMaxBlocks = 1L << 40;

// what the cast needs of an element format: mantissa bits M, the exponent of the smallest normal emin = 1 - bias, the exponent of the
// largest normal emax, the largest magnitude code, the element bits
struct MxFormat {
    int M, emin, emax, max_code, bits;
};

inline bool mx_format(int id, MxFormat& f) {
    switch (id) {
        case RDO_MX_FP4: f = {1, 0, 2, 7, 4}; return true;
        case RDO_MX_FP6_E2M3: f = {3, 0, 2, 31, 6}; return true;
        case RDO_MX_FP6_E3M2: f = {2, -2, 4, 31, 6}; return true;
        case RDO_MX_FP8_E4M3: f = {3, -6, 8, 126, 8}; return true;
        case RDO_MX_FP8_E5M2: f = {2, -14, 15, 123, 8}; return true;
    }
    return false;
}

// __clz for both passes of the compiler: the cast functions are plain integer C++ and run on the host as well as on the device
__host__ __device__ __forceinline__ int lead_zeros(unsigned x) { return __builtin_clz(x); }

// floor(log2(x)) of the positive finite fp32 value with the bit pattern `mag` (sign cleared, not zero)
__host__ __device__ __forceinline__ int floor_log2_bits(unsigned mag) {
    const int ef = (int)(mag >> 23);
    return ef > 0 ? ef - 127 : (31 - lead_zeros(mag)) - 149;
}

// the magnitude code of |v| / 2^E for the finite fp32 magnitude pattern `mag`: nearest representable, ties to the even mantissa,
// saturating at f.max_code
__host__ __device__ __forceinline__ unsigned mx_encode(unsigned mag, int E, const MxFormat& f) {
    if (mag == 0u) return 0u;
    const int ef = (int)(mag >> 23);
    const unsigned sig = ef > 0 ? ((mag & 0x7FFFFFu) | 0x800000u) : mag;      // |v| = sig * 2^(ev - 23)
    const int ev = (ef > 0 ? ef : 1) - 127;
    const int msb = 31 - lead_zeros(sig);
    const int eu = msb + ev - 23 - E;                                           // floor(log2(|v| / 2^E))
    if (eu > f.emax) return (unsigned)f.max_code;
    const int eq = eu > f.emin ? eu : f.emin;                                   // the binade whose spacing applies: 2^(eq - M)
    int s = eq - f.M + 23 + E - ev;                                             // |v| / 2^E / 2^(eq - M) = sig / 2^s
    unsigned n;
    if (s <= 0) {
        n = sig << (-s);                                                        // exact (an fp32 subnormal under E = -127): s >= msb - M
    } else {
        s = s > 31 ? 31 : s;                                                    // sig < 2^24: from s = 25 on the quotient is below one half
        n = sig >> s;
        const unsigned rem = sig & ((1u << s) - 1u), half = 1u << (s - 1);
        n += (rem > half || (rem == half && (n & 1u))) ? 1u : 0u;
    }
    // subnormals and the first binade are n itself; above, the implicit one of n (2^M) is the step of the exponent field
    const unsigned code = ((unsigned)(eq - f.emin) << f.M) + n;
    return code > (unsigned)f.max_code ? (unsigned)f.max_code : code;
}

// the fp32 bit pattern (sign clear) of the magnitude code times 2^E: exact for every format and every E in [-127, 127]
__host__ __device__ __forceinline__ unsigned mx_decode(unsigned code, int E, const MxFormat& f) {
    const unsigned ex = code >> f.M, m = code & ((1u << f.M) - 1u);
    const unsigned k = ex ? ((1u << f.M) | m) : m;                             // value = k * 2^p
    if (k == 0u) return 0u;
    const int p = (int)(ex ? ex - 1u : 0u) + f.emin - f.M + E;
    const int msb = 31 - lead_zeros(k);
    const int e = p + msb;
    if (e >= -126) return ((unsigned)(e + 127) << 23) | ((k << (23 - msb)) & 0x7FFFFFu);
    return k << (p + 149);                                                      // an fp32 subnormal; p >= -14 - 2 - 127 = -143
}

// the shared exponent of a block from the largest magnitude pattern of its elements (finite): E = clamp(floor(log2(amax)) - emax, -127, .)
__host__ __device__ __forceinline__ int mx_block_exponent(unsigned amax, const MxFormat& f) {
    if (amax == 0u) return -127;
    const int E = floor_log2_bits(amax) - f.emax;
    return E < -127 ? -127 : E;                                                 // (never above 127 - emax)
}

#if defined(__HIPCC__)
template <typename T>
__device__ __forceinline__ T half_wave_max(T v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        const T u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}
#endif

// (row, block) pairs of a call; 0 for a geometry that is refused
inline long mx_blocks(int32_t rows, int64_t inner, long& nb) {
    if (rows <= 0 || inner <= 0) return 0;
    nb = (long)rdo::ceil_div(inner, (int64_t)kBlock);
    if (nb > kMaxBlocks / rows) return 0;
    return nb * rows;
}

// workgroups of eight blocks for a grid-stride loop: enough waves to keep 4-byte accesses in flight on 256 CUs
inline unsigned mx_grid(long total) {
    const long g = rdo::ceil_div(total, 8);
    return (unsigned)(g > 4L * rdo::kGridCap ? 4L * rdo::kGridCap : g);
}

}  // namespace
