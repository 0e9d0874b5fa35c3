// OCP microscaling (MX) block formats for weights (include/rdo_ptq_mx.h): blocks of 32 elements along a row, one shared power-of-two
// scale (E8M0) per block, FP4 / FP6 / FP8 elements.  Built with -ffp-contract=off.
//
// Everything that decides a bit is integer arithmetic on the fp32 bit pattern: the exponent field (with __clz on the fraction of an fp32
// subnormal) gives floor(log2(amax)); the cast is one shift of the 24-bit significand with round-to-nearest-even, added onto the
// exponent part of the code so that a mantissa carry moves into the next binade by itself; wq is put together as an fp32 bit pattern.
// Denormal flushing, log2f and ldexpf cannot move a bit.  The only fp32 operation is d = w - wq of the error sum.
//
// Layout: a block is 32 lanes, a wave handles two blocks, a workgroup of 256 threads eight.  The grid runs over (row, block) pairs
// g = row * nb + b in a grid-stride loop, so an activation-shaped operand ([65536, 192]: six blocks a row) streams like a long weight
// row does: lane l of block b reads and writes element 32 b + l of its row with 4-byte accesses, neighbouring blocks of a row are
// neighbours in memory (a row whose inner is no multiple of 32 starts unaligned to the block size: nothing assumes more than 4-byte
// alignment).  amax comes from five xor-shuffle steps inside the half-wave on the magnitudes' bit patterns (an integer max: inf and NaN
// patterns are larger than every finite one, which is how a non-finite block is seen).
// Sums: the 32 exact float64 terms of a block fold by the same xor-shuffles into a per-block partial in the workspace; a second launch
// gives every row one wave that adds the row's partials in ascending order per lane and folds its 64 lanes.  No atomics.
// The format table, the cast (mx_encode / mx_decode) and the block amax are in mx_device.h, shared with mx_round.hip.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mx.h"
#include "mx_device.h"

namespace {

__device__ __forceinline__ double half_wave_sum(double v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// w and wq may be the same buffer: no __restrict__, every thread reads its element before it writes it and touches no other
__global__ __launch_bounds__(256) void mx_fakequant_kernel(const float* w, long total, long nb, long inner, MxFormat f, float* wq,
                                                           uint8_t* scales, uint8_t* codes, double* perr, double* pen) {
    const int lane = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const long stride = (long)gridDim.x * 8;
    // `base` is uniform over the wave: all 64 lanes stay in the loop together, a block past the end only masks its accesses
    // (row, b) of g = base + half walk along with it: one 64-bit division a thread, none in the loop
    const long base0 = (long)blockIdx.x * 8 + ((threadIdx.x >> 6) << 1);
    const long drow = stride / nb, db = stride - drow * nb;
    long row = (base0 + half) / nb, b = (base0 + half) - row * nb;
    for (long base = base0; base < total; base += stride, row += drow, b += db) {
        if (b >= nb) {
            b -= nb;
            ++row;
        }
        const long g = base + half;
        const long i = b * kBlock + lane;
        const bool live = g < total && i < inner;
        const long at = row * inner + i;
        const unsigned bits = live ? __builtin_bit_cast(unsigned, w[at]) : 0u;
        const unsigned mag = bits & 0x7FFFFFFFu;
        const unsigned amax = half_wave_max(mag);
        const bool finite = amax < 0x7F800000u;
        int E = -127;
        if (finite && amax != 0u) {
            E = floor_log2_bits(amax) - f.emax;
            E = E < -127 ? -127 : E;                                            // (never above 127 - emax)
        }
        unsigned code = 0u, qbits = 0x7FC00000u;
        if (finite) {
            const unsigned c = mx_encode(mag, E, f);
            const unsigned sign = bits & 0x80000000u;
            code = c | (sign >> (32 - f.bits));
            qbits = mx_decode(c, E, f) | sign;
        }
        const float v = __builtin_bit_cast(float, bits), q = __builtin_bit_cast(float, qbits);
        if (live) {
            if (wq) wq[at] = q;
            if (codes) codes[at] = (uint8_t)code;
            if (scales && lane == 0) scales[g] = (uint8_t)(finite ? E + 127 : 255);
        }
        if (perr) {
            const float d = live ? v - q : 0.f;
            const double se = half_wave_sum((double)d * (double)d), sw = half_wave_sum((double)v * (double)v);
            if (lane == 0 && g < total) {
                perr[g] = se;
                pen[g] = sw;
            }
        }
    }
}

// one wave per row: lane l adds the partials l, l + 64, .. of the row in ascending order, the 64 lanes fold by __shfl_down 32 .. 1
__global__ __launch_bounds__(256) void mx_row_sum_kernel(int rows, long nb, const double* perr, const double* pen, double* err,
                                                         double* energy) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    double se = 0.0, sw = 0.0;
    if (row < rows) {
        for (long b = lane; b < nb; b += 64) {
            se = se + perr[row * nb + b];
            sw = sw + pen[row * nb + b];
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        se = se + __shfl_down(se, o, 64);
        sw = sw + __shfl_down(sw, o, 64);
    }
    if (lane == 0 && row < rows) {
        if (err) err[row] = se;
        if (energy) energy[row] = sw;
    }
}

__global__ __launch_bounds__(256) void mx_dequant_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, long total,
                                                         long nb, long inner, MxFormat f, float* __restrict__ w) {
    const int lane = threadIdx.x & 31;
    const long stride = (long)gridDim.x * 8;
    for (long g = (long)blockIdx.x * 8 + (threadIdx.x >> 5); g < total; g += stride) {
        const long row = g / nb, b = g - row * nb;
        const long i = b * kBlock + lane;
        if (i >= inner) continue;
        const long at = row * inner + i;
        const unsigned sc = scales[g], c = codes[at];
        const unsigned sign = (c >> (f.bits - 1)) & 1u, magc = c & ((1u << (f.bits - 1)) - 1u);
        const unsigned qbits = sc == 255u ? 0x7FC00000u : (mx_decode(magc, (int)sc - 127, f) | (sign << 31));
        w[at] = __builtin_bit_cast(float, qbits);
    }
}

}  // namespace

extern "C" {

int32_t rdo_mx_format_bits(int32_t format) {
    MxFormat f;
    return mx_format(format, f) ? f.bits : 0;
}

int64_t rdo_mx_fakequant_workspace(int32_t rows, int64_t inner) {
    long nb = 0;
    const long total = mx_blocks(rows, inner, nb);
    return total * 16;                                                          // double [total] error partials | double [total] energy partials
}

int rdo_mx_fakequant(const float* w, int32_t rows, int64_t inner, int32_t format, float* wq, uint8_t* scales, uint8_t* codes, double* err,
                     double* energy, void* ws, void* stream) {
    RDO_REQUIRE(rows > 0 && inner > 0, "rdo_mx_fakequant: non-positive size rows %d inner %lld", rows, (long long)inner);
    MxFormat f;
    RDO_REQUIRE(mx_format(format, f), "rdo_mx_fakequant: unknown format %d (0 .. %d)", format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(wq || scales || codes || err || energy, "rdo_mx_fakequant: all five outputs are NULL");
    RDO_REQUIRE(w, "rdo_mx_fakequant: null pointer w");
    RDO_REQUIRE(reinterpret_cast<uintptr_t>(w) % 4 == 0 && reinterpret_cast<uintptr_t>(wq) % 4 == 0,
                "rdo_mx_fakequant: w and wq must be 4-byte aligned");
    long nb = 0;
    const long total = mx_blocks(rows, inner, nb);
    RDO_REQUIRE(total > 0, "rdo_mx_fakequant: rows %d of inner %lld make more than 2^40 blocks", rows, (long long)inner);
    const bool sums = err || energy;
    RDO_REQUIRE(!sums || ws, "rdo_mx_fakequant: err and energy need the workspace ws");
    RDO_REQUIRE(reinterpret_cast<uintptr_t>(err) % 8 == 0 && reinterpret_cast<uintptr_t>(energy) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(ws) % 8 == 0, "rdo_mx_fakequant: err, energy and ws must be 8-byte aligned");
    double* perr = sums ? static_cast<double*>(ws) : nullptr;
    double* pen = sums ? perr + total : nullptr;
    const long in = (long)inner;
    const double elems = (double)rows * (double)inner;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_fakequant_kernel, dim3(mx_grid(total)), dim3(256), 0, s, w, total, nb, in, f, wq, scales, codes, perr, pen);
            if (sums)
                hipLaunchKernelGGL(mx_row_sum_kernel, dim3((unsigned)rdo::ceil_div(rows, 4)), dim3(256), 0, s, rows, nb, (const double*)perr,
                                   (const double*)pen, err, energy);
            return rdo::check_launch("mx_fakequant");
        },
        stream, "mx_fakequant", 0.0, elems * (4.0 + (wq ? 4.0 : 0.0) + (codes ? 1.0 : 0.0)));
}

int rdo_mx_dequant(const uint8_t* codes, const uint8_t* scales, int32_t rows, int64_t inner, int32_t format, float* w, void* stream) {
    RDO_REQUIRE(codes && scales && w, "rdo_mx_dequant: null pointer");
    RDO_REQUIRE(rows > 0 && inner > 0, "rdo_mx_dequant: non-positive size rows %d inner %lld", rows, (long long)inner);
    MxFormat f;
    RDO_REQUIRE(mx_format(format, f), "rdo_mx_dequant: unknown format %d (0 .. %d)", format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(reinterpret_cast<uintptr_t>(w) % 4 == 0, "rdo_mx_dequant: w must be 4-byte aligned");
    long nb = 0;
    const long total = mx_blocks(rows, inner, nb);
    RDO_REQUIRE(total > 0, "rdo_mx_dequant: rows %d of inner %lld make more than 2^40 blocks", rows, (long long)inner);
    const long in = (long)inner;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_dequant_kernel, dim3(mx_grid(total)), dim3(256), 0, s, codes, scales, total, nb, in, f, w);
            return rdo::check_launch("mx_dequant");
        },
        stream, "mx_dequant", 0.0, (double)rows * (double)inner * 5.0);
}

}  // extern "C"
