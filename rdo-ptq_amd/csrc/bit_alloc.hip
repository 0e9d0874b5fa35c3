// Mixed-precision weight widths (include/rdo_ptq_bits.h): what round-to-nearest costs a weight row at K widths, in one call.
// Built with -ffp-contract=off (the fake-quantisation expression rounds as in adaround.hip; both take it from uaq_device.h).
//
// rdo_uaq_width_scan.  A bit allocation needs, per weight and per candidate width b, the grid (delta, zero point) and the squared error
// sum (w - wq)^2 of round-to-nearest on it.  Done with the existing entries that is K x (rdo_uaq_init_minmax + rdo_uaq_fakequant + a
// reduction): 3 K launches and 2 K + K reads of the weight plus K writes of wq.  Here a row of up to kLdsRow floats is read ONCE by one
// workgroup, staged in LDS while its min / max are taken, and scored at all K widths from LDS; nothing but [K][rows] results is written.
// A longer row (a per-tensor quantiser sees the whole weight as one row) is split into shares of kChunk floats, one workgroup each, with
// the partials in a workspace and a fixed-order sum behind them: no workgroup waits for another inside a launch.
// Every sum is float64 of exact terms ((double)d * (double)d holds the 48-bit product of two fp32 values), in an order that depends on
// (inner, K) alone: thread t adds the elements t, t + 256, .. of its share in ascending order, then block_sum_d.  No atomics.
#include <algorithm>

#include "rdo_common.h"
#include "uaq_device.h"
#include "../../include/rdo_ptq_bits.h"

namespace {

constexpr int kMaxK = RDO_WIDTH_SCAN_MAX_K;
constexpr int kLdsRow = RDO_WIDTH_SCAN_LDS_ROW;
constexpr int kChunk = RDO_WIDTH_SCAN_CHUNK;

struct ScanWidths {
    int K;
    int n_levels[kMaxK];
};

// Sums of N doubles over a 256-thread workgroup behind one barrier, in a fixed order (rdo::block_sum in float64): per wave the 64-lane
// __shfl_down steps 32 .. 1, the four wave sums through LDS, then ((w0 + w1) + w2) + w3.  Valid on thread 0 only.
template <int N>
__device__ __forceinline__ void block_sum_d(double (&v)[N]) {
    __shared__ double red[N][4];
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = v[e] + __shfl_down(v[e], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int e = 0; e < N; ++e) red[e][threadIdx.x >> 6] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = ((red[e][0] + red[e][1]) + red[e][2]) + red[e][3];
}

// the grids of one row in registers: entry k < K from g[k * rows + r] (delta and zp alike), the rest a harmless copy of entry 0
struct RowGrids {
    float dl[kMaxK], z[kMaxK], lm1[kMaxK];
};

// thread t of 256: the elements t, t + 256, .. of src[0, n) in ascending order into acc[k] (squared error at width k) and acc[kMaxK]
// (energy)
template <typename Src>
__device__ __forceinline__ void score_share(Src src, long n, int K, const RowGrids& rg, double (&acc)[kMaxK + 1]) {
    for (long i = threadIdx.x; i < n; i += 256) {
        const float v = src[i];
        acc[kMaxK] = acc[kMaxK] + (double)v * (double)v;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k < K) {
                const float d = v - rdo::uaq_nearest(v, rg.dl[k], rg.z[k], rg.lm1[k]);
                acc[k] = acc[k] + (double)d * (double)d;
            }
        }
    }
}

// ---- rows that fit LDS: one workgroup per row, one read of the row
__global__ __launch_bounds__(256) void scan_row_kernel(const float* __restrict__ w, int rows, int inner, ScanWidths g,
                                                       const float* __restrict__ delta_in, const float* __restrict__ zp_in, float* delta,
                                                       float* zp, double* err, double* energy) {
    __shared__ float srow[kLdsRow];
    __shared__ float sdl[kMaxK], szp[kMaxK];
    const int r = blockIdx.x;
    const float* p = w + (long)r * inner;
    float mn = 0.f, mx = 0.f;                              // the range is clamped through 0
    for (int i = threadIdx.x; i < inner; i += 256) {
        const float v = p[i];
        srow[i] = v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    rdo::uaq_block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        for (int k = 0; k < g.K; ++k) {
            const long o = (long)k * rows + r;
            float dl, z;
            if (delta_in) {
                dl = delta_in[o];
                z = zp_in[o];
            } else {
                rdo::uaq_minmax_grid(mn, mx, g.n_levels[k], dl, z);
            }
            sdl[k] = delta[o] = dl;
            szp[k] = zp[o] = z;
        }
    }
    __syncthreads();                                       // srow, sdl and szp are complete
    RowGrids rg;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        const int kk = k < g.K ? k : 0;
        rg.dl[k] = sdl[kk];
        rg.z[k] = szp[kk];
        rg.lm1[k] = (float)(g.n_levels[kk] - 1);
    }
    double acc[kMaxK + 1];
#pragma unroll
    for (int k = 0; k <= kMaxK; ++k) acc[k] = 0.0;
    score_share(srow, (long)inner, g.K, rg, acc);
    block_sum_d(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < g.K) err[(long)k * rows + r] = acc[k];
        energy[r] = acc[kMaxK];
    }
}

// ---- split rows.  share b = (row b / nchunks, chunk b % nchunks) covers the elements [chunk * kChunk, min(inner, (chunk + 1) * kChunk))
__global__ __launch_bounds__(256) void scan_share_minmax_kernel(const float* __restrict__ w, long inner, int nchunks, float* pmn, float* pmx) {
    const int r = blockIdx.x / nchunks, c = blockIdx.x - r * nchunks;
    const long i0 = (long)c * kChunk, n = inner - i0 < kChunk ? inner - i0 : (long)kChunk;
    const float* p = w + (long)r * inner + i0;
    float mn = 0.f, mx = 0.f;
    for (long i = threadIdx.x; i < n; i += 256) {
        const float v = p[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    rdo::uaq_block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        pmn[blockIdx.x] = mn;
        pmx[blockIdx.x] = mx;
    }
}

// one workgroup per row: the grids of the row from the shares' min / max, or the given grids copied through
__global__ __launch_bounds__(256) void scan_row_grids_kernel(int rows, int nchunks, ScanWidths g, const float* pmn, const float* pmx,
                                                             const float* __restrict__ delta_in, const float* __restrict__ zp_in,
                                                             float* delta, float* zp) {
    const int r = blockIdx.x;
    float mn = 0.f, mx = 0.f;
    if (!delta_in) {
        for (int c = threadIdx.x; c < nchunks; c += 256) {
            mn = fminf(mn, pmn[(long)r * nchunks + c]);
            mx = fmaxf(mx, pmx[(long)r * nchunks + c]);
        }
    }
    rdo::uaq_block_minmax(mn, mx);
    if (threadIdx.x == 0) {
        for (int k = 0; k < g.K; ++k) {
            const long o = (long)k * rows + r;
            float dl, z;
            if (delta_in) {
                dl = delta_in[o];
                z = zp_in[o];
            } else {
                rdo::uaq_minmax_grid(mn, mx, g.n_levels[k], dl, z);
            }
            delta[o] = dl;
            zp[o] = z;
        }
    }
}

__global__ __launch_bounds__(256) void scan_share_score_kernel(const float* __restrict__ w, int rows, long inner, int nchunks, ScanWidths g,
                                                               const float* delta, const float* zp, double* perr, double* pen) {
    const int r = blockIdx.x / nchunks, c = blockIdx.x - r * nchunks;
    const long i0 = (long)c * kChunk, n = inner - i0 < kChunk ? inner - i0 : (long)kChunk;
    RowGrids rg;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        const int kk = k < g.K ? k : 0;
        rg.dl[k] = delta[(long)kk * rows + r];
        rg.z[k] = zp[(long)kk * rows + r];
        rg.lm1[k] = (float)(g.n_levels[kk] - 1);
    }
    double acc[kMaxK + 1];
#pragma unroll
    for (int k = 0; k <= kMaxK; ++k) acc[k] = 0.0;
    score_share(w + (long)r * inner + i0, n, g.K, rg, acc);
    block_sum_d(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < g.K) perr[(long)blockIdx.x * g.K + k] = acc[k];
        pen[blockIdx.x] = acc[kMaxK];
    }
}

// one workgroup per row: thread t adds the shares t, t + 256, .. in ascending order, then the fixed tree
__global__ __launch_bounds__(256) void scan_row_sum_kernel(int rows, int nchunks, int K, const double* perr, const double* pen, double* err,
                                                           double* energy) {
    const int r = blockIdx.x;
    double acc[kMaxK + 1];
#pragma unroll
    for (int k = 0; k <= kMaxK; ++k) acc[k] = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += 256) {
        const long b = (long)r * nchunks + c;
        acc[kMaxK] = acc[kMaxK] + pen[b];
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < K) acc[k] = acc[k] + perr[b * K + k];
    }
    block_sum_d(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
            if (k < K) err[(long)k * rows + r] = acc[k];
        energy[r] = acc[kMaxK];
    }
}

// shares of a call (rows x chunks of a split row), 0 for rows that fit LDS, -1 for more than 32-bit workgroup indices hold
inline int64_t scan_shares(int32_t rows, int64_t inner) {
    if (inner <= kLdsRow) return 0;
    const int64_t nchunks = rdo::ceil_div(inner, (int64_t)kChunk);
    if (nchunks > 0x7fffffffLL || nchunks * rows > 0x7fffffffLL) return -1;
    return nchunks * rows;
}

}  // namespace

extern "C" {

int64_t rdo_uaq_width_scan_workspace(int32_t rows, int64_t inner, int32_t K) {
    if (rows <= 0 || inner <= 0 || K < 1 || K > kMaxK) return 0;
    const int64_t shares = scan_shares(rows, inner);
    if (shares < 0) return 0;
    // double [shares][K] error partials | double [shares] energy partials | float [shares] min | float [shares] max
    return std::max<int64_t>(16, shares * (K + 1) * 8 + shares * 2 * 4);
}

int rdo_uaq_width_scan(const float* w, int32_t rows, int64_t inner, const int32_t* widths, int32_t K, const float* delta_in,
                       const float* zp_in, float* delta, float* zp, double* err, double* energy, void* ws, void* stream) {
    RDO_REQUIRE(w && widths && delta && zp && err && energy && ws, "rdo_uaq_width_scan: null pointer");
    RDO_REQUIRE(rows > 0 && inner > 0, "rdo_uaq_width_scan: non-positive size rows %d inner %lld", rows, (long long)inner);
    RDO_REQUIRE(K >= 1 && K <= kMaxK, "rdo_uaq_width_scan: K %d outside [1, %d]", K, kMaxK);
    RDO_REQUIRE((delta_in == nullptr) == (zp_in == nullptr), "rdo_uaq_width_scan: delta_in and zp_in must be given together or not at all");
    ScanWidths g{};
    g.K = K;
    for (int k = 0; k < K; ++k) {
        const int b = widths[k];
        RDO_REQUIRE(b >= RDO_WIDTH_SCAN_MIN_BITS && b <= RDO_WIDTH_SCAN_MAX_BITS, "rdo_uaq_width_scan: width %d outside [%d, %d]", b,
                    RDO_WIDTH_SCAN_MIN_BITS, RDO_WIDTH_SCAN_MAX_BITS);
        for (int j = 0; j < k; ++j) RDO_REQUIRE(widths[j] != b, "rdo_uaq_width_scan: width %d is given twice", b);
        g.n_levels[k] = 1 << b;
    }
    RDO_REQUIRE(reinterpret_cast<uintptr_t>(err) % 8 == 0 && reinterpret_cast<uintptr_t>(energy) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(ws) % 8 == 0, "rdo_uaq_width_scan: err, energy and ws must be 8-byte aligned");
    const int64_t shares = scan_shares(rows, inner);
    RDO_REQUIRE(shares >= 0, "rdo_uaq_width_scan: rows %d of inner %lld make more than 2^31 - 1 shares", rows, (long long)inner);
    const double bytes = 4.0 * (double)rows * (double)inner;
    if (shares == 0) {
        const int in = (int)inner;
        return rdo::dispatch(
            [=](hipStream_t s) {
                hipLaunchKernelGGL(scan_row_kernel, dim3(rows), dim3(256), 0, s, w, rows, in, g, delta_in, zp_in, delta, zp, err, energy);
                return rdo::check_launch("uaq_width_scan");
            },
            stream, "uaq_width_scan", 0.0, bytes);
    }
    const int nchunks = (int)(shares / rows);
    double* perr = static_cast<double*>(ws);
    double* pen = perr + shares * K;
    float* pmn = reinterpret_cast<float*>(pen + shares);
    float* pmx = pmn + shares;
    const bool given = delta_in != nullptr;
    return rdo::dispatch(
        [=](hipStream_t s) {
            const dim3 per_share((unsigned)shares), per_row((unsigned)rows), wg(256);
            if (!given) hipLaunchKernelGGL(scan_share_minmax_kernel, per_share, wg, 0, s, w, (long)inner, nchunks, pmn, pmx);
            hipLaunchKernelGGL(scan_row_grids_kernel, per_row, wg, 0, s, rows, nchunks, g, (const float*)pmn, (const float*)pmx, delta_in, zp_in,
                               delta, zp);
            hipLaunchKernelGGL(scan_share_score_kernel, per_share, wg, 0, s, w, rows, (long)inner, nchunks, g, (const float*)delta,
                               (const float*)zp, perr, pen);
            hipLaunchKernelGGL(scan_row_sum_kernel, per_row, wg, 0, s, rows, nchunks, K, (const double*)perr, (const double*)pen, err, energy);
            return rdo::check_launch("uaq_width_scan");
        },
        stream, "uaq_width_scan", 0.0, (given ? 1.0 : 2.0) * bytes);
}

}  // extern "C"
