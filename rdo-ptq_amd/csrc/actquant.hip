// K6 -- per-channel activation quantisers on NHWC fp32 tensors (channel = fastest dim): the dynamic quantiser (min | max of the tensor
// itself), the static one (a frozen lo | hi pair), the range search, the range scoring, the static backward, the Adam step of learned
// ranges, the per-channel histogram with its percentile and its histogram-MSE selection, the pair moments of two tensors (the
// per-unit output error report), and the width scan (one grid scored at K widths: include/rdo_ptq_actbits.h).
// Built with -ffp-contract=off (products and sums round separately, like the reference's op chains).
//
// Six of them reduce over the pixels per channel, and all six do it the same way, without atomics: up to kAqBlocks workgroups each
// leave one row of partial values for their share of the pixels (aq_partial below), a small second kernel folds the rows (aq_fold_kernel).
// (The first version let 1024 workgroups atomicMin / atomicMax into the same 2 C words: 0.4 M contended atomics per call were most of its
// time.)  The order of the fp32 additions is fixed HERE, once, and frozen ranges depend on it: a thread's running sum over its pixels in
// ascending order, closed into a second sum every kAqsChain pixels (tot + acc at the end), lane 0 adding the pixel lanes 1 .. PL - 1 in
// ascending order onto its own, the fold's lane j adding the rows j, j + 16, .. serially, then the xor tree 8, 4, 2, 1.  No serial chain
// is longer than 1024 terms: kAqsChain pixels, at most 256 pixel lanes, at most kAqBlocks / 16 rows per lane.
#include <initializer_list>
#include <type_traits>

#include "../../include/rdo_ptq_actbits.h"
#include "rdo_common.h"

namespace {

using rdo::grid_for;

constexpr int kAqBlocks = 256;
constexpr int kAqsCand = 10;
constexpr int kAqsChain = 1024;

// thread = (pixel lane, group of W channels): qpb groups side by side, PL pixel lanes of them in a workgroup of 256
struct AqGeom { int QN, qpb, PL; };
__host__ __device__ inline AqGeom aq_geom(int C, int W) {
    const int QN = C / W, qpb = QN < 256 ? QN : 256;
    return AqGeom{QN, qpb, 256 / qpb};
}
// enough workgroups to keep HBM busy, few enough that each has >= 8 pixels per lane to amortise its fold
inline int aq_blocks(long npix, int C, int W) {
    const long g = rdo::ceil_div(npix, (long)aq_geom(C, W).PL * 8);
    return (int)(g < 1 ? 1 : (g > kAqBlocks ? kAqBlocks : g));
}

// one element on the per-channel grid [zp, zp + rng] with bit_range steps; `lowest` is the lower clamp of the normalised value: -1 in the
// dynamic quantiser (the reference's clamp; x - min is never negative there), 0 with a frozen range (x may lie below it).  The dynamic
// and the static quantiser, the range search and the backward all evaluate THIS expression: same numbers in, same bits out.
__device__ __forceinline__ float aq_quant(float x, float zp, float rng, float bit_range, float lowest) {
    const float xn = x - zp;
    const float q = rintf(fminf(fmaxf(xn / rng, lowest), 1.f) * bit_range);
    return (q / bit_range) * rng + zp;
}

// ---- the partial skeleton: W-wide loads down the pixels, FLIGHT of them in flight, then an LDS fold over the pixel lanes.  A Body gives
// what differs: N values per channel, their start value zero(e) and combine(a, b, e), begin(q, C) for a new channel group, load(off) of
// one pixel's operands and pixel(in, off, acc) on them (off = element offset of the group's first channel in that pixel), kChain
// (close the running values every kAqsChain pixels: sums only) and the row layout ([channel][N] or [N][channel]).
template <int W, int FLIGHT, class Body>
__device__ __forceinline__ void aq_partial(Body b, long npix, int C, float* part) {
    constexpr int N = Body::N;
    const AqGeom m = aq_geom(C, W);
    const int pl = threadIdx.x / m.qpb, ql = threadIdx.x - pl * m.qpb;
    __shared__ float sm[W * N * 256];                      // [channel of the group][value][thread]: conflict-free both ways
    const long step = (long)gridDim.x * m.PL;
    for (int qb = 0; qb < m.QN; qb += m.qpb) {
        const int q = qb + ql;
        const bool live = pl < m.PL && q < m.QN;
        if (live) {
            float acc[W][N], tot[W][N];
#pragma unroll
            for (int k = 0; k < W; ++k)
#pragma unroll
                for (int e = 0; e < N; ++e) acc[k][e] = tot[k][e] = Body::zero(e);
            b.begin(q, C);
            const long off = (long)q * W;
            int run = 0;
            auto one = [&](const typename Body::in_t& v, long p) {
                b.pixel(v, off + p * C, acc);
                if (Body::kChain && ++run == kAqsChain) {
                    run = 0;
#pragma unroll
                    for (int k = 0; k < W; ++k)
#pragma unroll
                        for (int e = 0; e < N; ++e) { tot[k][e] += acc[k][e]; acc[k][e] = 0.f; }
                }
            };
            long p = (long)blockIdx.x * m.PL + pl;
            if constexpr (FLIGHT > 1) {
                for (; p + (FLIGHT - 1) * step < npix; p += FLIGHT * step) {
                    typename Body::in_t v[FLIGHT];
#pragma unroll
                    for (int u = 0; u < FLIGHT; ++u) v[u] = b.load(off + (p + u * step) * C);
#pragma unroll
                    for (int u = 0; u < FLIGHT; ++u) one(v[u], p + u * step);
                }
            }
            for (; p < npix; p += step) one(b.load(off + p * C), p);
#pragma unroll
            for (int k = 0; k < W; ++k)
#pragma unroll
                for (int e = 0; e < N; ++e) sm[(k * N + e) * 256 + threadIdx.x] = Body::kChain ? tot[k][e] + acc[k][e] : acc[k][e];
        }
        __syncthreads();
        if (live && pl == 0) {
            float* dst = part + (long)blockIdx.x * N * C;
#pragma unroll
            for (int k = 0; k < W; ++k)
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    float r = sm[(k * N + e) * 256 + ql];
                    for (int t = 1; t < m.PL; ++t) r = Body::combine(r, sm[(k * N + e) * 256 + t * m.qpb + ql], e);
                    dst[Body::kChannelMajor ? (q * W + k) * N + e : e * C + q * W + k] = r;
                }
        }
        __syncthreads();
    }
}

// ---- dynamic quantiser: min | max of the tensor, part = [workgroup][min[C] | max[C]] behind the 2 C result floats of the workspace
template <int W>
struct AqMinMax {
    typedef float in_t __attribute__((ext_vector_type(W)));
    static constexpr int N = 2;
    static constexpr bool kChain = false, kChannelMajor = false;
    const float* x;
    __device__ static float zero(int e) { return e ? -INFINITY : INFINITY; }
    __device__ static float combine(float a, float v, int e) { return e ? fmaxf(a, v) : fminf(a, v); }
    __device__ void begin(int, int) {}
    __device__ in_t load(long off) const { return *reinterpret_cast<const in_t*>(x + off); }
    __device__ void pixel(const in_t& v, long, float (&acc)[W][N]) const {
#pragma unroll
        for (int k = 0; k < W; ++k) { acc[k][0] = fminf(acc[k][0], v[k]); acc[k][1] = fmaxf(acc[k][1], v[k]); }
    }
};
template <int W>
__global__ __launch_bounds__(256) void aq_partial_kernel(const float* x, long npix, int C, float* part) {
    aq_partial<W, 4>(AqMinMax<W>{x}, npix, C, part);
}

// ---- range search: err[c][k] = sum over pixels of (x - Q_k(x))^2 for the ten shrunk ranges lo * s_k | hi * s_k, s_k = 1 - 0.05 k
// (the candidates of UniformAffineQuantizer._init_search, quantizer.py:260-265 of the reference, on the activation grid): one read of
// x, W x 10 running sums (and as many closed ones) in registers, so one pixel in flight; part = [workgroup][C][10].
template <int W>
struct AqSearch {
    typedef float in_t __attribute__((ext_vector_type(W)));
    static constexpr int N = kAqsCand;
    static constexpr bool kChain = true, kChannelMajor = true;
    const float* x;
    const float* range;
    float bit_range;
    float lo[W], hi[W];
    __device__ static float zero(int) { return 0.f; }
    __device__ static float combine(float a, float v, int) { return a + v; }
    __device__ void begin(int q, int C) {
#pragma unroll
        for (int k = 0; k < W; ++k) { lo[k] = range[q * W + k]; hi[k] = range[C + q * W + k]; }
    }
    __device__ in_t load(long off) const { return *reinterpret_cast<const in_t*>(x + off); }
    __device__ void pixel(const in_t& v, long, float (&acc)[W][N]) const {
#pragma unroll
        for (int j = 0; j < kAqsCand; ++j) {
            const float s = (float)(1.0 - 0.05 * j);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float zp = lo[k] * s;
                const float rng = fmaxf(hi[k] * s - zp, 1e-6f);
                const float d = v[k] - aq_quant(v[k], zp, rng, bit_range, 0.f);
                acc[k][j] += d * d;
            }
        }
    }
};
template <int W>
__global__ __launch_bounds__(256) void aqs_partial_kernel(const float* x, long npix, int C, const float* range, float bit_range, float* part) {
    aq_partial<W, 1>(AqSearch<W>{x, range, bit_range}, npix, C, part);
}

// ---- backward of the static quantiser (straight-through rint): dx = g inside [lo, hi], 0 outside; per workgroup and channel the partial
// sums of d/dlo and d/dhi.  With y the forward's value (aq_quant on the forward's operands: the same bits) an inside element contributes
// g (x - y) / r to lo and g (y - x) / r to hi -- the quantisation residual over the width, which does not cancel on wide grids the way
// t - q / R does -- an element below the range g to lo, one above it g to hi.  The region is decided by fp32 comparisons of x with the
// ends, not from the normalised value.  One read of x and of g, one write of dx (dx may be g: every element is read and written by the
// same thread, and the loads of the pixels in flight come before their stores); part = [workgroup][lo[C] | hi[C]].  A channel narrower
// than 1e-6 (the forward's floor on the width) gets no range gradient.
template <int W>
struct AqBackward {
    typedef float vec_t __attribute__((ext_vector_type(W)));
    struct in_t { vec_t x, g; };
    static constexpr int N = 2;
    static constexpr bool kChain = true, kChannelMajor = false;
    const float* x;
    const float* g;
    const float* range;
    float bit_range;
    float* dx;
    float lo[W], hi[W], rng[W];
    bool wide[W];
    __device__ static float zero(int) { return 0.f; }
    __device__ static float combine(float a, float v, int) { return a + v; }
    __device__ void begin(int q, int C) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            lo[k] = range[q * W + k];
            hi[k] = range[C + q * W + k];
            rng[k] = fmaxf(hi[k] - lo[k], 1e-6f);
            wide[k] = !(hi[k] - lo[k] < 1e-6f);
        }
    }
    __device__ in_t load(long off) const { return in_t{*reinterpret_cast<const vec_t*>(x + off), *reinterpret_cast<const vec_t*>(g + off)}; }
    __device__ void pixel(const in_t& v, long off, float (&acc)[W][N]) const {
        vec_t d;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const bool below = v.x[k] < lo[k], above = v.x[k] > hi[k];
            const float y = aq_quant(v.x[k], lo[k], rng[k], bit_range, 0.f);
            const float res = (v.x[k] - y) / rng[k];                 // (y - x) / r is its exact negative
            const float tl = below ? 1.f : above ? 0.f : res;
            const float th = above ? 1.f : below ? 0.f : -res;
            acc[k][0] += wide[k] ? v.g[k] * tl : 0.f;
            acc[k][1] += wide[k] ? v.g[k] * th : 0.f;
            d[k] = (below || above) ? 0.f : v.g[k];
        }
        *reinterpret_cast<vec_t*>(dx + off) = d;
    }
};
template <int W>
__global__ __launch_bounds__(256) void aqb_partial_kernel(const float* x, const float* g, long npix, int C, const float* range, float bit_range,
                                                          float* dx, float* part) {
    aq_partial<W, 4>(AqBackward<W>{x, g, range, bit_range, dx}, npix, C, part);
}

// ---- range scoring: the measured squared error of K arbitrary grids lo_k | hi_k per channel, err[c][k] = sum over pixels of
// (x - Q_k(x))^2 with Q_k the static quantiser's own expression (aq_quant on max(hi_k - lo_k, 1e-6), lower clamp 0: the scored grid is the
// applied grid), next to it the counts of the values below lo_k and above hi_k (fp32 comparisons of x with the ends, as in the backward)
// and the channel's energy sum x^2.  One read of x, W x (3 K + 1) running values (and as many closed ones) in registers, so one pixel in
// flight like the search; part = [workgroup][C][err[K] | (below, above)[K] | energy].  A count runs as an integer-valued float: a
// workgroup sees about npix / workgroups pixels of a channel, and there are kAqBlocks workgroups unless npix < 8 * 256 * kAqBlocks: below
// 2^24 for every npix < 2^31 the entry admits, so a partial row holds the exact integer, and the fold (aqc_fold_kernel) adds the rows as
// int32.
constexpr int kAqcMax = RDO_ACT_SCORE_MAX;
template <int W, int K>
struct AqScore {
    typedef float in_t __attribute__((ext_vector_type(W)));
    static constexpr int N = 3 * K + 1;
    static constexpr bool kChain = true, kChannelMajor = true;
    const float* x;
    const float* cand;                                     // [K][2C]
    float bit_range;
    float lo[K][W], hi[K][W];
    __device__ static float zero(int) { return 0.f; }
    __device__ static float combine(float a, float v, int) { return a + v; }
    __device__ void begin(int q, int C) {
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int k = 0; k < W; ++k) {
                lo[j][k] = cand[(long)j * 2 * C + q * W + k];
                hi[j][k] = cand[(long)j * 2 * C + C + q * W + k];
            }
    }
    __device__ in_t load(long off) const { return *reinterpret_cast<const in_t*>(x + off); }
    __device__ void pixel(const in_t& v, long, float (&acc)[W][N]) const {
#pragma unroll
        for (int k = 0; k < W; ++k) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float rng = fmaxf(hi[j][k] - lo[j][k], 1e-6f);
                const float d = v[k] - aq_quant(v[k], lo[j][k], rng, bit_range, 0.f);
                acc[k][j] += d * d;
                acc[k][K + 2 * j] += v[k] < lo[j][k] ? 1.f : 0.f;
                acc[k][K + 2 * j + 1] += v[k] > hi[j][k] ? 1.f : 0.f;
            }
            acc[k][3 * K] += v[k] * v[k];
        }
    }
};
template <int W, int K>
__global__ __launch_bounds__(256) void aqc_partial_kernel(const float* x, long npix, int C, const float* cand, float bit_range, float* part) {
    aq_partial<W, 1>(AqScore<W, K>{x, cand, bit_range}, npix, C, part);
}

// ---- width scan: the measured squared error of ONE grid lo | hi per channel at K widths, err[c][k] = sum over pixels of (x - Q_k(x))^2
// with Q_k the static quantiser's own expression at 2^b_k - 1 steps (aq_quant on max(hi - lo, 1e-6), lower clamp 0), next to it the
// channel's energy sum x^2: the scoring kernel with the grid fixed and the step count varied, the counts dropped.  One read of x, W x
// (K + 1) running sums (and as many closed ones) in registers, so one pixel in flight like the score; part = [workgroup][C][err[K] |
// energy].  The step counts travel as a kernel argument (a host array by contract).
constexpr int kAqwMax = RDO_ACT_WIDTH_SCAN_MAX_K;
struct AqwSteps { float v[kAqwMax]; };
template <int W, int K>
struct AqWidthScan {
    typedef float in_t __attribute__((ext_vector_type(W)));
    static constexpr int N = K + 1;
    static constexpr bool kChain = true, kChannelMajor = true;
    const float* x;
    const float* range;
    AqwSteps steps;
    float lo[W], rng[W];
    __device__ static float zero(int) { return 0.f; }
    __device__ static float combine(float a, float v, int) { return a + v; }
    __device__ void begin(int q, int C) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            lo[k] = range[q * W + k];
            rng[k] = fmaxf(range[C + q * W + k] - lo[k], 1e-6f);
        }
    }
    __device__ in_t load(long off) const { return *reinterpret_cast<const in_t*>(x + off); }
    __device__ void pixel(const in_t& v, long, float (&acc)[W][N]) const {
#pragma unroll
        for (int k = 0; k < W; ++k) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float d = v[k] - aq_quant(v[k], lo[k], rng[k], steps.v[j], 0.f);
                acc[k][j] += d * d;
            }
            acc[k][K] += v[k] * v[k];
        }
    }
};
template <int W, int K>
__global__ __launch_bounds__(256) void aqw_partial_kernel(const float* x, long npix, int C, const float* range, AqwSteps steps, float* part) {
    aq_partial<W, 1>(AqWidthScan<W, K>{x, range, steps}, npix, C, part);
}

// fold of the scan's partial rows [workgroup][C][K + 1]: the lanes and the order of aq_fold_kernel<true> (lane j adds the rows j, j + 16,
// .. serially from zero, then the xor tree 8, 4, 2, 1).  err and energy = the sum (WRITTEN); energy may be null.
__global__ __launch_bounds__(256) void aqw_fold_kernel(const float* part, int nblk, int C, int K, float* err, float* energy) {
    const int N = K + 1, n = C * N;
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4), j = threadIdx.x & 15;
    const bool live = i < n;
    const int c = i / N, e = i - c * N;
    float r = 0.f;
    if (live) {
        const float* src = part + i;
        int b = j;
        for (; b + 48 < nblk; b += 64) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[(long)(b + 16 * u) * n];
#pragma unroll
            for (int u = 0; u < 4; ++u) r = r + v[u];
        }
        for (; b < nblk; b += 16) r = r + src[(long)b * n];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) r = r + __shfl_xor(r, o, 16);
    if (live && j == 0) {
        if (e < K) err[c * K + e] = r;
        else if (energy) energy[c] = r;
    }
}

// ---- pair moments: per channel the three sums over the pixels of d = a - b (fp32), d * d and a * a, in one read of both tensors (the
// per-unit output error report: a = the full-precision output, b = the quantised one, so energy is the full-precision energy).  W x 3
// running sums (and as many closed ones) in registers, two pixels of both streams in flight; part = [workgroup][shift[C] | err[C] |
// energy[C]], the layout of the result.
template <int W>
struct AqPair {
    typedef float vec_t __attribute__((ext_vector_type(W)));
    struct in_t { vec_t a, b; };
    static constexpr int N = 3;
    static constexpr bool kChain = true, kChannelMajor = false;
    const float* a;
    const float* b;
    __device__ static float zero(int) { return 0.f; }
    __device__ static float combine(float r, float v, int) { return r + v; }
    __device__ void begin(int, int) {}
    __device__ in_t load(long off) const { return in_t{*reinterpret_cast<const vec_t*>(a + off), *reinterpret_cast<const vec_t*>(b + off)}; }
    __device__ void pixel(const in_t& v, long, float (&acc)[W][N]) const {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float d = v.a[k] - v.b[k];
            acc[k][0] += d;
            acc[k][1] += d * d;
            acc[k][2] += v.a[k] * v.a[k];
        }
    }
};
template <int W>
__global__ __launch_bounds__(256) void aqp_partial_kernel(const float* a, const float* b, long npix, int C, float* part) {
    aq_partial<W, 2>(AqPair<W>{a, b}, npix, C, part);
}

// fold of the score's partial rows [workgroup][C][3 K + 1]: the lanes and the order of aq_fold_kernel<true> (lane j adds the rows j, j + 16,
// .. serially, then the xor tree 8, 4, 2, 1); an error or energy entry is summed in fp32, a count entry in int32 (every row's value is an
// exact integer below 2^24).  err and energy += the sum, clip += the count; clip and energy may be null.
__global__ __launch_bounds__(256) void aqc_fold_kernel(const float* part, int nblk, int C, int K, float* err, int* clip, float* energy) {
    const int N = 3 * K + 1, n = C * N;
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4), j = threadIdx.x & 15;
    const bool live = i < n;
    const int c = i / N, e = i - c * N;
    const bool count = e >= K && e < 3 * K;
    float r = 0.f;
    int ri = 0;
    if (live) {
        const float* src = part + i;
        int b = j;
        for (; b + 48 < nblk; b += 64) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[(long)(b + 16 * u) * n];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                r = r + v[u];
                ri += count ? (int)v[u] : 0;
            }
        }
        for (; b < nblk; b += 16) {
            const float v = src[(long)b * n];
            r = r + v;
            ri += count ? (int)v : 0;
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        r = r + __shfl_xor(r, o, 16);
        ri += __shfl_xor(ri, o, 16);
    }
    if (live && j == 0) {
        if (e < K) err[c * K + e] += r;
        else if (count) {
            if (clip) clip[c * 2 * K + (e - K)] += ri;
        } else if (energy) energy[c] += r;
    }
}

// ---- fold of the `nblk` partial rows of n entries: sixteen lanes per entry walk the rows (independent loads, no serial chain of nblk
// round trips; the values still combine in row order), then fold across the lanes.  SUM: out[i] += the sum; else out[i] = min (first half
// of the entries) | max (second half).
template <bool SUM>
__global__ __launch_bounds__(256) void aq_fold_kernel(const float* part, int nblk, int n, float* out) {
    const int i = blockIdx.x * 16 + (threadIdx.x >> 4), j = threadIdx.x & 15;
    const bool live = i < n;
    const bool is_max = i >= n / 2;
    auto combine = [&](float a, float v) { return SUM ? a + v : is_max ? fmaxf(a, v) : fminf(a, v); };
    float r = SUM ? 0.f : is_max ? -INFINITY : INFINITY;
    if (live) {
        const float* src = part + i;
        int b = j;
        for (; b + 48 < nblk; b += 64) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[(long)(b + 16 * u) * n];
#pragma unroll
            for (int u = 0; u < 4; ++u) r = combine(r, v[u]);
        }
        for (; b < nblk; b += 16) r = combine(r, src[(long)b * n]);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) r = combine(r, __shfl_xor(r, o, 16));
    if (live && j == 0) out[i] = SUM ? out[i] + r : r;
}

// STATIC = false: ws = this tensor's own min | max (aq_fold_kernel); true: ws = a frozen lo | hi pair (rdo_actquant_static)
template <int W, bool STATIC = false>
__global__ __launch_bounds__(256) void aq_apply_kernel(const float* x, long nvec, int C, const float* ws, float bit_range, float* out) {
    typedef float vec_t __attribute__((ext_vector_type(W)));
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)((i * W) % C);
        const vec_t xv = *reinterpret_cast<const vec_t*>(x + i * W);
        vec_t o;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float zp = ws[c + k];
            const float rng = fmaxf(ws[C + c + k] - zp, 1e-6f);
            o[k] = aq_quant(xv[k], zp, rng, bit_range, STATIC ? 0.f : -1.f);
        }
        *reinterpret_cast<vec_t*>(out + i * W) = o;
    }
}

// observation: fold this batch's min | max (the first 2 C floats the dynamic call leaves in its workspace) into a running lo | hi
__global__ __launch_bounds__(256) void aq_merge_kernel(const float* ws, int C, float* range) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * C) range[i] = i < C ? fminf(range[i], ws[i]) : fmaxf(range[i], ws[i]);
}

// ---- one Adam step on a site's range [2C] = lo | hi, then the projection: thread = channel (the projection couples its two ends).  The
// step is relative to the observed width w = hi_obs - lo_obs; both ends stay inside [lo_obs, hi_obs] and at least 1e-3 w apart.
__global__ __launch_bounds__(256) void act_range_step_kernel(float* range, const float* grad, const float* obs, float* m, float* v, int C,
                                                             float lr, float bc1, float bc2) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float lo0 = obs[c], hi0 = obs[C + c], w = hi0 - lo0;
    float end[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int i = e * C + c;
        const float gr = grad[i];
        const float mi = 0.9f * m[i] + 0.1f * gr;
        const float vi = 0.999f * v[i] + 0.001f * (gr * gr);
        m[i] = mi;
        v[i] = vi;
        end[e] = range[i] - lr * w * (mi / bc1) / (sqrtf(vi / bc2) + 1e-8f);
    }
    const float gap = 1e-3f * w;
    float lo = fminf(fmaxf(end[0], lo0), hi0), hi = fminf(fmaxf(end[1], lo0), hi0);
    hi = fminf(fmaxf(hi, lo + gap), hi0);
    lo = fmaxf(fminf(lo, hi - gap), lo0);
    range[c] = lo;
    range[C + c] = hi;
}

// ---- per-channel histogram of x on the observed range lo | hi: kAqhBins integer counters per channel.  Not a Body of aq_partial (that
// keeps N running values per channel in REGISTERS): a workgroup owns a tile of up to kAqhTile channels x kAqhBins int counters in LDS
// (64 KiB: two workgroups per CU), walks its share of the pixels with W-wide loads, FLIGHT of them in flight, and counts with LDS integer
// atomicAdd; at the end it adds its NON-ZERO counters to hist with global integer atomicAdd.  Integer sums do not depend on the order of
// the adds: the same input gives the same counts from launch to launch.  thread = (pixel lane, group of W channels of the tile), the
// channel fastest: a channel whose values all sit in one bin collides on 256 / (channels of the tile) lanes of a workgroup, not on all.
// A counter sits at [row][(bin + row) & 1023]: the rotation spreads equal bins of different channels (many values at an end of their
// ranges) over the LDS banks.  grid = (pixel blocks, channel tiles).
constexpr int kAqhBins = 1024;
constexpr int kAqhTile = 16;
static_assert((kAqhBins & (kAqhBins - 1)) == 0, "the rotation masks with kAqhBins - 1");

// groups of W channels side by side in a tile
__host__ __device__ inline int aqh_qpb(int C, int W) {
    const int QN = C / W, qt = kAqhTile / W;
    return QN < qt ? QN : qt;
}

// bin of an element: the rule of include/rdo_ptq_hip.h, every operation rounded on its own.  (A NaN counts in bin 0.)
__device__ __forceinline__ int aqh_bin(float x, float lo, float w) {
    const float t = ((x - lo) / w) * (float)kAqhBins;
    return (int)fminf(fmaxf(floorf(t), 0.f), (float)(kAqhBins - 1));
}

template <int W>
__global__ __launch_bounds__(256) void aqh_kernel(const float* x, long npix, int C, const float* range, int* hist) {
    typedef float vec_t __attribute__((ext_vector_type(W)));
    constexpr int FLIGHT = 4;
    __shared__ int sm[kAqhTile * kAqhBins];
    const int QN = C / W, qpb = aqh_qpb(C, W), PL = 256 / qpb;
    const int pl = threadIdx.x / qpb, ql = threadIdx.x - pl * qpb;
    const int q = blockIdx.y * qpb + ql;                   // this thread's channel group
    for (int i = threadIdx.x; i < kAqhTile * kAqhBins; i += 256) sm[i] = 0;
    __syncthreads();
    if (pl < PL && q < QN) {
        float lo[W], w[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            lo[k] = range[q * W + k];
            w[k] = fmaxf(range[C + q * W + k] - lo[k], 1e-6f);
        }
        const float* src = x + (long)q * W;
        auto count = [&](const vec_t& v) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int row = ql * W + k;
                atomicAdd(&sm[row * kAqhBins + ((aqh_bin(v[k], lo[k], w[k]) + row) & (kAqhBins - 1))], 1);
            }
        };
        const long step = (long)gridDim.x * PL;
        long p = (long)blockIdx.x * PL + pl;
        for (; p + (FLIGHT - 1) * step < npix; p += FLIGHT * step) {
            vec_t v[FLIGHT];
#pragma unroll
            for (int u = 0; u < FLIGHT; ++u) v[u] = *reinterpret_cast<const vec_t*>(src + (p + u * step) * C);
#pragma unroll
            for (int u = 0; u < FLIGHT; ++u) count(v[u]);
        }
        for (; p < npix; p += step) count(*reinterpret_cast<const vec_t*>(src + p * C));
    }
    __syncthreads();
    const int c0 = blockIdx.y * qpb * W;                    // first channel of the tile
    const int rows = C - c0 < qpb * W ? C - c0 : qpb * W;
    for (int i = threadIdx.x; i < rows * kAqhBins; i += 256) {
        const int n = sm[i];
        if (n) {
            const int row = i / kAqhBins, bin = (i - row) & (kAqhBins - 1);
            atomicAdd(&hist[(long)(c0 + row) * kAqhBins + bin], n);
        }
    }
}

// ---- percentile range of a channel from its histogram: one wave per channel, lane l holds the bins 16 l .. 16 l + 15.  With k =
// floor(tail * n) whole bins are dropped from each end while the dropped count stays <= k: the prefix sums P(a) = sum of the bins below a
// grow with a, so the largest a in [0, 1023] with P(a) <= k is the NUMBER of a in [1, 1023] with P(a) <= k; the same from the top for d in
// [1, 1023 - a].  Integer arithmetic in 64 bits, then two fp32 operations per moved end.
__global__ __launch_bounds__(256) void aqh_select_kernel(const int* hist, int C, const float* range, double tail, float* out) {
    constexpr int PER = kAqhBins / 64;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;                                    // (a whole wave: the shuffles below stay among live lanes)
    const int* h = hist + (long)c * kAqhBins + lane * PER;
    long long cnt[PER], mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { cnt[j] = h[j]; mine += cnt[j]; }
    long long incl = mine;                                 // inclusive prefix over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const long long n = __shfl(incl, 63, 64);
    const long long k = (long long)floor(tail * (double)n);
    auto wave_sum = [](int v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
    long long run = incl - mine;                           // P(16 lane)
    int na = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        run += cnt[j];                                     // P(a), a = 16 lane + j + 1
        na += (lane * PER + j + 1 <= kAqhBins - 1 && run <= k) ? 1 : 0;
    }
    const int a = wave_sum(na);
    run = n - incl;                                        // the bins above this lane's
    int nd = 0;
#pragma unroll
    for (int j = PER - 1; j >= 0; --j) {
        run += cnt[j];                                     // the bins from 16 lane + j up: d = 1024 - (16 lane + j)
        nd += (kAqhBins - (lane * PER + j) <= kAqhBins - 1 - a && run <= k) ? 1 : 0;
    }
    const int d = wave_sum(nd);
    if (lane == 0) {
        const float lo = range[c], hi = range[C + c], wr = hi - lo;
        const bool keep = wr < 1e-6f || n == 0;
        out[c] = (keep || a == 0) ? lo : lo + ((float)a / (float)kAqhBins) * wr;
        out[C + c] = (keep || d == 0) ? hi : lo + ((float)(kAqhBins - d) / (float)kAqhBins) * wr;
    }
}

// ---- histogram-MSE range of a channel from its histogram (the rule of include/rdo_ptq_hip.h): the exhaustive search over all 524 800 clip
// pairs (a bins off the bottom, d off the top, a + d <= 1023), one workgroup of 1024 per channel.  Tables in LDS (32 KiB): for every cut the
// clipped count and the clipped squared distance E.  Both are exact integers below 2^53 and are kept as DOUBLES: the sum of two E and the
// difference N - C_lo - C_hi are exact in binary64 too, so (double)(E_lo + E_hi) and (double)(N - C_lo - C_hi) of the rule are one fp64 add
// each, the very values, and the top side's pair is ONE 16-byte LDS read.  A side's table is the exclusive block scan of the three moments
// sum n, sum n b, sum n b^2 in 64-bit integers, thread t holding bin t (the top side scans the bins reversed); E(p) = (3 p^2 - 3 p + 1) M0
// - (6 p - 3) M1 + 3 M2.  Thread t then owns ONE a -- t for the first 512 threads, 1023 - (t - 512) for the others, so the waves w, w + 4,
// w + 8, w + 12 walk 2176 values of d between them for every w: the four SIMDs of the CU carry the same load -- and walks d upwards, four
// candidates in flight: all lanes read the same hi[d], an LDS broadcast.  Within a thread a + d grows with d, so it keeps the first
// strictly smaller S; across threads the key (S, a + d, a), a strict total order: a wave xor tree, then sixteen rows in LDS.  No atomics,
// no floating-point reduction: every launch gives the same bits.
// What bounds it: the issue of the candidate loop on the CU's four SIMDs -- per candidate a quarter of a 16-byte LDS broadcast
// instruction's issue, three fp64 adds, two fp64 products, the integer W^2 and its conversion, one fp64 compare and three selects, times
// 2176 trips of four waves per SIMD.  There is no memory stream (a channel reads its 4 KiB of counts twice); with C below the 256 CUs
// every channel has a CU of its own, and the call does not grow with the pixels.
constexpr int kAqmThreads = 1024;
static_assert(kAqmThreads == kAqhBins, "thread = bin in the scans, thread = a in the search");
struct AqmBest { double s; int a, d; };
struct AqmTop { double e, c; };
__device__ __forceinline__ bool aqm_better(double s, int a, int d, const AqmBest& b) {
    return s < b.s || (s == b.s && (a + d < b.a + b.d || (a + d == b.a + b.d && a < b.a)));
}

// exclusive scan of one side: for the cut p = threadIdx.x in [0, 1023], cnt = the values in the p outermost bins, e = their squared
// distance sum; `tot`: the waves' moment sums
template <bool TOP>
__device__ __forceinline__ void aqm_side(const int* h, long long (*tot)[3], long long& cnt, long long& e) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long p = threadIdx.x;                       // position from this side's end
    const long long n = h[TOP ? kAqhBins - 1 - threadIdx.x : threadIdx.x];
    const long long m[3] = {n, n * p, n * p * p};
    long long incl[3] = {m[0], m[1], m[2]};
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long up = __shfl_up(incl[j], o, 64);
            if (lane >= o) incl[j] += up;
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int j = 0; j < 3; ++j) tot[wave][j] = incl[j];
    }
    __syncthreads();
    long long run[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        run[j] = incl[j] - m[j];
        for (int w = 0; w < wave; ++w) run[j] += tot[w][j];
    }
    cnt = run[0];
    e = (3 * p * p - 3 * p + 1) * run[0] - (6 * p - 3) * run[1] + 3 * run[2];
}

__global__ __launch_bounds__(kAqmThreads) void aqm_select_kernel(const int* hist, int C, const float* range, double k4l2, float* out,
                                                                 double* score) {
    constexpr int NW = kAqmThreads / 64;
    __shared__ double c_lo[kAqhBins], e_lo[kAqhBins];
    __shared__ AqmTop hi_t[kAqhBins];
    __shared__ long long tot[2][NW][3];
    __shared__ AqmBest red[NW];
    const int c = blockIdx.x, t = threadIdx.x;             // grid = C
    const int* h = hist + (long)c * kAqhBins;
    long long cnt, e;
    aqm_side<false>(h, tot[0], cnt, e);
    c_lo[t] = (double)cnt;
    e_lo[t] = (double)e;
    const long long total = t == kAqhBins - 1 ? cnt + h[t] : 0;
    aqm_side<true>(h, tot[1], cnt, e);
    hi_t[t] = AqmTop{(double)e, (double)cnt};
    __shared__ long long total_sm;
    if (t == kAqhBins - 1) total_sm = total;
    __syncthreads();
    const long long n = total_sm;
    const float lo = range[c], hi = range[C + c], wr = hi - lo;
    if (wr < 1e-6f || n == 0) {                            // (the whole workgroup: nothing below is skipped by a part of it)
        if (t == 0) {
            out[c] = lo;
            out[C + c] = hi;
            if (score) score[2 * c] = score[2 * c + 1] = 0.0;
        }
        return;
    }
    const int a = t < 512 ? t : kAqhBins - 1 - (t - 512);
    const int nd = kAqhBins - a;                           // d = 0 .. nd - 1
    const double ea = e_lo[a], keep_a = (double)n - c_lo[a];
    auto cand = [&](int d) {
        const AqmTop v = hi_t[d];
        const int w = nd - d;
        return k4l2 * (ea + v.e) + (keep_a - v.c) * (double)(w * w);
    };
    double bs = INFINITY;
    int bd = 0;
    int d = 0;
    for (; d + 4 <= nd; d += 4) {
        double s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] = cand(d + u);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool lt = s[u] < bs;
            bs = lt ? s[u] : bs;
            bd = lt ? d + u : bd;
        }
    }
    for (; d < nd; ++d) {
        const double s = cand(d);
        const bool lt = s < bs;
        bs = lt ? s : bs;
        bd = lt ? d : bd;
    }
    AqmBest best{bs, a, bd};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double s = __shfl_xor(best.s, o, 64);
        const int a2 = __shfl_xor(best.a, o, 64), d2 = __shfl_xor(best.d, o, 64);
        if (aqm_better(s, a2, d2, best)) best = AqmBest{s, a2, d2};
    }
    if ((t & 63) == 0) red[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < NW; ++w)
            if (aqm_better(red[w].s, red[w].a, red[w].d, best)) best = red[w];
        out[c] = best.a == 0 ? lo : lo + ((float)best.a / (float)kAqhBins) * wr;
        out[C + c] = best.d == 0 ? hi : lo + ((float)(kAqhBins - best.d) / (float)kAqhBins) * wr;
        if (score) {
            score[2 * c] = best.s;
            score[2 * c + 1] = k4l2 * (e_lo[0] + hi_t[0].e) + ((double)n - c_lo[0] - hi_t[0].c) * (double)(kAqhBins * kAqhBins);
        }
    }
}

// ---- host helpers
int aq_bit_range(int n_bits, const char* who, float* bit_range) {
    RDO_REQUIRE(n_bits >= 2 && n_bits <= 16, "%s: n_bits %d outside [2, 16]", who, n_bits);
    *bit_range = (float)((1 << n_bits) - 1);
    return RDO_OK;
}
// the W = 4 kernels need whole float4 groups of channels and 16-byte aligned tensors
bool aq_vec(int C, std::initializer_list<const void*> tensors) {
    uintptr_t bits = 0;
    for (const void* p : tensors) bits |= reinterpret_cast<uintptr_t>(p);
    return C % 4 == 0 && bits % 16 == 0;
}
// launch(W as a compile-time constant) with W = 4 | 1
template <class F>
void aq_with_width(bool vec, F launch) {
    if (vec) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, 1>{});
}
inline dim3 aq_fold_grid(int n) { return dim3((unsigned)rdo::ceil_div(n, 16)); }

}  // namespace

extern "C" {

int rdo_actquant_perchannel(const float* x, int64_t npix, int32_t C, int32_t n_bits, float* out, float* ws_minmax, void* stream) {
    RDO_REQUIRE(x && out && ws_minmax && npix > 0 && C > 0, "rdo_actquant_perchannel: bad argument");
    float bit_range;
    if (const int e = aq_bit_range(n_bits, "rdo_actquant_perchannel", &bit_range)) return e;
    float* ws = ws_minmax;
    float* part = ws_minmax + 2 * (long)C;
    const bool vec = aq_vec(C, {x, out});
    return rdo::dispatch(
        [=](hipStream_t s) {
            aq_with_width(vec, [&](auto w) {
                constexpr int W = decltype(w)::value;
                const int nblk = aq_blocks(npix, C, W);
                hipLaunchKernelGGL(aq_partial_kernel<W>, dim3(nblk), dim3(256), 0, s, x, (long)npix, C, part);
                hipLaunchKernelGGL(aq_fold_kernel<false>, aq_fold_grid(2 * C), dim3(256), 0, s, part, nblk, 2 * C, ws);
                const long nvec = (long)npix * C / W;
                hipLaunchKernelGGL(aq_apply_kernel<W>, dim3(grid_for(nvec)), dim3(256), 0, s, x, nvec, C, ws, bit_range, out);
            });
            return rdo::check_launch("actquant_perchannel");
        },
        stream);
}

int64_t rdo_actquant_workspace(int32_t C) { return C > 0 ? 2 * (int64_t)C * (kAqBlocks + 1) : 0; }

int rdo_actquant_static(const float* x, int64_t npix, int32_t C, int32_t n_bits, const float* range, float* out, void* stream) {
    RDO_REQUIRE(x && out && range && npix > 0 && C > 0, "rdo_actquant_static: bad argument");
    float bit_range;
    if (const int e = aq_bit_range(n_bits, "rdo_actquant_static", &bit_range)) return e;
    const bool vec = aq_vec(C, {x, out});
    return rdo::dispatch(
        [=](hipStream_t s) {
            aq_with_width(vec, [&](auto w) {
                constexpr int W = decltype(w)::value;
                const long nvec = (long)npix * C / W;
                hipLaunchKernelGGL((aq_apply_kernel<W, true>), dim3(grid_for(nvec)), dim3(256), 0, s, x, nvec, C, range, bit_range, out);
            });
            return rdo::check_launch("actquant_static");
        },
        stream, "actquant_static", 0.0, 8.0 * npix * C);
}

int rdo_actquant_observe(const float* ws_minmax, int32_t C, float* range, void* stream) {
    RDO_REQUIRE(ws_minmax && range && C > 0, "rdo_actquant_observe: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(aq_merge_kernel, dim3((unsigned)rdo::ceil_div(2 * (long)C, 256)), dim3(256), 0, s, ws_minmax, C, range);
            return rdo::check_launch("actquant_observe");
        },
        stream, "actquant_observe", 0.0, 24.0 * C);
}

int rdo_actquant_search(const float* x, int64_t npix, int32_t C, int32_t n_bits, const float* range, float* err, float* ws, void* stream) {
    RDO_REQUIRE(x && range && err && ws && npix > 0 && C > 0, "rdo_actquant_search: bad argument");
    float bit_range;
    if (const int e = aq_bit_range(n_bits, "rdo_actquant_search", &bit_range)) return e;
    const bool vec = aq_vec(C, {x});
    return rdo::dispatch(
        [=](hipStream_t s) {
            aq_with_width(vec, [&](auto w) {
                constexpr int W = decltype(w)::value;
                const int nblk = aq_blocks(npix, C, W), n = C * kAqsCand;
                hipLaunchKernelGGL(aqs_partial_kernel<W>, dim3(nblk), dim3(256), 0, s, x, (long)npix, C, range, bit_range, ws);
                hipLaunchKernelGGL(aq_fold_kernel<true>, aq_fold_grid(n), dim3(256), 0, s, ws, nblk, n, err);
            });
            return rdo::check_launch("actquant_search");
        },
        stream, "actquant_search", 0.0, 4.0 * npix * C);
}

int64_t rdo_actquant_search_workspace(int32_t C) { return C > 0 ? (int64_t)C * kAqsCand * kAqBlocks : 0; }

int rdo_actquant_score(const float* x, int64_t npix, int32_t C, int32_t n_bits, const float* cand, int32_t K, float* err, int32_t* clip,
                       float* energy, float* ws, void* stream) {
    RDO_REQUIRE(x && cand && err && ws && npix > 0 && C > 0, "rdo_actquant_score: bad argument");
    RDO_REQUIRE(K >= 1 && K <= kAqcMax, "rdo_actquant_score: K %d outside [1, %d]", K, kAqcMax);
    float bit_range;
    if (const int e = aq_bit_range(n_bits, "rdo_actquant_score", &bit_range)) return e;
    RDO_REQUIRE(npix <= 0x7fffffffLL, "rdo_actquant_score: %lld pixels do not fit a channel's 32-bit counts", (long long)npix);
    RDO_REQUIRE((int64_t)C * (3 * kAqcMax + 1) <= 0x7fffffffLL, "rdo_actquant_score: %d channels are too many for 32-bit entry indices", C);
    const bool vec = aq_vec(C, {x});
    return rdo::dispatch(
        [=](hipStream_t s) {
            aq_with_width(vec, [&](auto w) {
                constexpr int W = decltype(w)::value;
                const int nblk = aq_blocks(npix, C, W);
                auto launch = [&](auto k) {
                    hipLaunchKernelGGL((aqc_partial_kernel<W, decltype(k)::value>), dim3(nblk), dim3(256), 0, s, x, (long)npix, C, cand,
                                       bit_range, ws);
                };
                switch (K) {
                    case 1: launch(std::integral_constant<int, 1>{}); break;
                    case 2: launch(std::integral_constant<int, 2>{}); break;
                    case 3: launch(std::integral_constant<int, 3>{}); break;
                    default: launch(std::integral_constant<int, 4>{}); break;
                }
                hipLaunchKernelGGL(aqc_fold_kernel, aq_fold_grid(C * (3 * K + 1)), dim3(256), 0, s, ws, nblk, C, K, err, clip, energy);
            });
            return rdo::check_launch("actquant_score");
        },
        stream, "actquant_score", 0.0, 4.0 * npix * C);
}

int64_t rdo_actquant_score_workspace(int32_t C, int32_t K) {
    return C > 0 && K >= 1 && K <= kAqcMax ? (int64_t)C * (3 * K + 1) * kAqBlocks : 0;
}

int rdo_actquant_width_scan(const float* x, int64_t npix, int32_t C, const float* range, const int32_t* widths, int32_t K, float* err,
                            float* energy, float* ws, void* stream) {
    RDO_REQUIRE(x && range && widths && err && ws && npix > 0 && C > 0, "rdo_actquant_width_scan: bad argument");
    RDO_REQUIRE(K >= 1 && K <= kAqwMax, "rdo_actquant_width_scan: K %d outside [1, %d]", K, kAqwMax);
    RDO_REQUIRE(npix <= 0x7fffffffLL, "rdo_actquant_width_scan: %lld pixels are beyond 32-bit pixel counts", (long long)npix);
    RDO_REQUIRE((int64_t)C * (kAqwMax + 1) <= 0x7fffffffLL, "rdo_actquant_width_scan: %d channels are too many for 32-bit entry indices", C);
    AqwSteps steps{};
    for (int k = 0; k < K; ++k) {
        if (const int e = aq_bit_range(widths[k], "rdo_actquant_width_scan", &steps.v[k])) return e;
        for (int j = 0; j < k; ++j)
            RDO_REQUIRE(widths[j] != widths[k], "rdo_actquant_width_scan: the width %d is given twice", widths[k]);
    }
    const bool vec = aq_vec(C, {x});
    return rdo::dispatch(
        [=](hipStream_t s) {
            aq_with_width(vec, [&](auto w) {
                constexpr int W = decltype(w)::value;
                const int nblk = aq_blocks(npix, C, W);
                auto launch = [&](auto k) {
                    hipLaunchKernelGGL((aqw_partial_kernel<W, decltype(k)::value>), dim3(nblk), dim3(256), 0, s, x, (long)npix, C, range, steps,
                                       ws);
                };
                switch (K) {
                    case 1: launch(std::integral_constant<int, 1>{}); break;
                    case 2: launch(std::integral_constant<int, 2>{}); break;
                    case 3: launch(std::integral_constant<int, 3>{}); break;
                    case 4: launch(std::integral_constant<int, 4>{}); break;
                    case 5: launch(std::integral_constant<int, 5>{}); break;
                    case 6: launch(std::integral_constant<int, 6>{}); break;
                    case 7: launch(std::integral_constant<int, 7>{}); break;
                    default: launch(std::integral_constant<int, 8>{}); break;
                }
                hipLaunchKernelGGL(aqw_fold_kernel, aq_fold_grid(C * (K + 1)), dim3(256), 0, s, ws, nblk, C, K, err, energy);
            });
            return rdo::check_launch("actquant_width_scan");
        },
        stream, "actquant_width_scan", 0.0, 4.0 * npix * C);
}

int64_t rdo_actquant_width_scan_workspace(int32_t C, int32_t K) {
    return C > 0 && (int64_t)C * (kAqwMax + 1) <= 0x7fffffffLL && K >= 1 && K <= kAqwMax ? (int64_t)C * (K + 1) * kAqBlocks : 0;
}

int rdo_pair_moments(const float* a, const float* b, int64_t npix, int32_t C, float* out, float* ws, void* stream) {
    RDO_REQUIRE(a && b && out && ws && npix > 0 && C > 0, "rdo_pair_moments: bad argument");
    RDO_REQUIRE(3 * (int64_t)C <= 0x7fffffffLL, "rdo_pair_moments: %d channels are too many for 32-bit entry indices", C);
    const bool vec = aq_vec(C, {a, b});
    return rdo::dispatch(
        [=](hipStream_t s) {
            aq_with_width(vec, [&](auto w) {
                constexpr int W = decltype(w)::value;
                const int nblk = aq_blocks(npix, C, W);
                hipLaunchKernelGGL(aqp_partial_kernel<W>, dim3(nblk), dim3(256), 0, s, a, b, (long)npix, C, ws);
                hipLaunchKernelGGL(aq_fold_kernel<true>, aq_fold_grid(3 * C), dim3(256), 0, s, ws, nblk, 3 * C, out);
            });
            return rdo::check_launch("pair_moments");
        },
        stream, "pair_moments", 0.0, 8.0 * npix * C);
}

int64_t rdo_pair_moments_workspace(int32_t C) { return C > 0 ? 3 * (int64_t)C * kAqBlocks : 0; }

int rdo_actquant_static_bwd(const float* x, const float* g, int64_t npix, int32_t C, int32_t n_bits, const float* range, float* dx,
                            float* drange, float* ws, void* stream) {
    RDO_REQUIRE(x && g && range && dx && drange && ws && npix > 0 && C > 0, "rdo_actquant_static_bwd: bad argument");
    float bit_range;
    if (const int e = aq_bit_range(n_bits, "rdo_actquant_static_bwd", &bit_range)) return e;
    RDO_REQUIRE(dx != x, "rdo_actquant_static_bwd: dx may alias g, not x");
    const bool vec = aq_vec(C, {x, g, dx});
    return rdo::dispatch(
        [=](hipStream_t s) {
            aq_with_width(vec, [&](auto w) {
                constexpr int W = decltype(w)::value;
                const int nblk = aq_blocks(npix, C, W);
                hipLaunchKernelGGL(aqb_partial_kernel<W>, dim3(nblk), dim3(256), 0, s, x, g, (long)npix, C, range, bit_range, dx, ws);
                hipLaunchKernelGGL(aq_fold_kernel<true>, aq_fold_grid(2 * C), dim3(256), 0, s, ws, nblk, 2 * C, drange);
            });
            return rdo::check_launch("actquant_static_bwd");
        },
        stream, "actquant_static_bwd", 0.0, 12.0 * npix * C);
}

int64_t rdo_actquant_static_bwd_workspace(int32_t C) { return C > 0 ? 2 * (int64_t)C * kAqBlocks : 0; }

int rdo_act_range_step(float* range, const float* grad, const float* obs, float* m, float* v, int32_t C, int32_t step, float lr,
                       void* stream) {
    RDO_REQUIRE(range && grad && obs && m && v && C > 0, "rdo_act_range_step: bad argument");
    RDO_REQUIRE(step >= 1, "rdo_act_range_step: step %d (the count of this step, from 1)", step);
    const float bc1 = (float)(1.0 - pow(0.9, (double)step)), bc2 = (float)(1.0 - pow(0.999, (double)step));
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(act_range_step_kernel, dim3((unsigned)rdo::ceil_div((long)C, 256L)), dim3(256), 0, s, range, grad, obs, m, v, C,
                               lr, bc1, bc2);
            return rdo::check_launch("act_range_step");
        },
        stream, "act_range_step", 0.0, 40.0 * C);
}

int32_t rdo_actquant_hist_bins(void) { return kAqhBins; }

int rdo_actquant_hist(const float* x, int64_t npix, int32_t C, const float* range, int32_t* hist, void* stream) {
    RDO_REQUIRE(x && range && hist && npix > 0 && C > 0, "rdo_actquant_hist: bad argument");
    RDO_REQUIRE(npix <= 0x7fffffffLL, "rdo_actquant_hist: %lld pixels do not fit a channel's 32-bit counters", (long long)npix);
    RDO_REQUIRE(C <= kAqhTile * 65535, "rdo_actquant_hist: %d channels are more than %d tiles of %d", C, 65535, kAqhTile);
    const bool vec = aq_vec(C, {x});
    return rdo::dispatch(
        [=](hipStream_t s) {
            aq_with_width(vec, [&](auto w) {
                constexpr int W = decltype(w)::value;
                const int qpb = aqh_qpb(C, W), PL = 256 / qpb;
                const long tiles = rdo::ceil_div((long)(C / W), (long)qpb);
                // as many pixel blocks as give every lane >= 8 pixels, at most two workgroups per CU over all tiles
                long nblk = rdo::ceil_div((long)npix, (long)PL * 8);
                const long cap = 512 / tiles < 1 ? 1 : 512 / tiles;
                nblk = nblk > cap ? cap : nblk;
                hipLaunchKernelGGL(aqh_kernel<W>, dim3((unsigned)nblk, (unsigned)tiles), dim3(256), 0, s, x, (long)npix, C, range, hist);
            });
            return rdo::check_launch("actquant_hist");
        },
        stream, "actquant_hist", 0.0, 4.0 * npix * C);
}

int rdo_act_hist_mse_select(const int32_t* hist, int32_t C, const float* range, int32_t n_bits, float* out, double* score, void* stream) {
    RDO_REQUIRE(hist && range && out && C > 0, "rdo_act_hist_mse_select: bad argument");
    float bit_range;
    if (const int e = aq_bit_range(n_bits, "rdo_act_hist_mse_select", &bit_range)) return e;
    const long long l1 = (1LL << n_bits) - 1;
    const double k4l2 = (double)(4 * l1 * l1);              // exact: below 2^34
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(aqm_select_kernel, dim3((unsigned)C), dim3(kAqmThreads), 0, s, hist, C, range, k4l2, out, score);
            return rdo::check_launch("act_hist_mse_select");
        },
        stream, "act_hist_mse_select", 0.0, 4.0 * kAqhBins * C + 32.0 * C);
}

int rdo_act_percentile_select(const int32_t* hist, int32_t C, const float* range, double tail, float* out, void* stream) {
    RDO_REQUIRE(hist && range && out && C > 0, "rdo_act_percentile_select: bad argument");
    RDO_REQUIRE(tail >= 0.0 && tail < 0.5, "rdo_act_percentile_select: tail %g outside [0, 0.5)", tail);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(aqh_select_kernel, dim3((unsigned)rdo::ceil_div((long)C, 4L)), dim3(256), 0, s, hist, C, range, tail, out);
            return rdo::check_launch("act_percentile_select");
        },
        stream, "act_percentile_select", 0.0, 4.0 * kAqhBins * C + 16.0 * C);
}

}  // extern "C"
