// Learned rounding (AdaRound) on the grids of the MX block formats (include/rdo_ptq_mxround.h).  Built with -ffp-contract=off.
//
// The integer-grid kernels of adaround.hip hard-code delta * (clamp(floor(w / delta) + h + zp) - zp) with one delta per row.  On an MX
// grid the distance to the next level differs per element: it depends on the block's shared exponent and on the binade the element falls
// in.  So the grid is resolved ONCE per weight into two fp32 streams -- lo, the grid value at or below the element, and gap, the distance
// to the next one (rdo_mx_neighbours; integer arithmetic on the fp32 bit pattern with the cast of mx_device.h, a block per half-wave as
// in mx_quant.hip) -- and the soft weight of the whole calibration is lo + gap * h(alpha): no division, no floor, no per-row look-up
// and no level clamp in the step.  gap == 0 marks a pinned element (where round to nearest saturates): the step leaves its alpha, m and v
// alone and keeps its weight at lo.
//
// rdo_mx_round_step has the shape of the flat form of adaround.hip's fused step (ada_step_body: float4 streams where numel % 4 == 0, a
// scalar form otherwise) with `w, delta, zp` replaced by `lo, gap`.  The element step -- slab sum, h(alpha), the LowerBound chain, the
// rounding regulariser, Adam, the rounding-loss publish -- is the one of ada_device.h that adaround.hip runs too; this file supplies the
// grid (MxGrid) and skips the pinned elements.  The dgrad layout is a second launch of that header's wd_transpose_body.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxround.h"
#include "mx_device.h"
#include "ada_device.h"

namespace {

// ---- neighbours ------------------------------------------------------------------------------------------------------------------------
// the fp32 bit pattern of 2^e, -149 <= e <= 127
__host__ __device__ __forceinline__ unsigned pow2_bits(int e) { return e >= -126 ? (unsigned)(e + 127) << 23 : 1u << (e + 149); }

// log2 of the distance between the magnitudes of codes c and c + 1, relative to the block scale
__host__ __device__ __forceinline__ int step_exp(unsigned c, const MxFormat& f) {
    const unsigned ex = c >> f.M;
    return (int)(ex ? ex - 1u : 0u) + f.emin - f.M;
}

// The largest magnitude code whose value is <= |v| / 2^E for the finite fp32 magnitude pattern `mag`: mx_encode with the quotient cut
// off instead of rounded.  exact: |v| / 2^E is that code's value; above: |v| / 2^E is larger than the format's maximum.
__host__ __device__ __forceinline__ unsigned mx_floor_code(unsigned mag, int E, const MxFormat& f, bool& exact, bool& above) {
    exact = true;
    above = false;
    if (mag == 0u) return 0u;
    const int ef = (int)(mag >> 23);
    const unsigned sig = ef > 0 ? ((mag & 0x7FFFFFu) | 0x800000u) : mag;      // |v| = sig * 2^(ev - 23)
    const int ev = (ef > 0 ? ef : 1) - 127;
    const int msb = 31 - lead_zeros(sig);
    const int eu = msb + ev - 23 - E;                                           // floor(log2(|v| / 2^E))
    if (eu > f.emax) {
        exact = false;
        above = true;
        return (unsigned)f.max_code;
    }
    const int eq = eu > f.emin ? eu : f.emin;
    int s = eq - f.M + 23 + E - ev;                                             // |v| / 2^E / 2^(eq - M) = sig / 2^s
    unsigned n;
    if (s <= 0) {
        n = sig << (-s);
    } else {
        s = s > 31 ? 31 : s;
        n = sig >> s;
        exact = (sig & ((1u << s) - 1u)) == 0u;
    }
    const unsigned code = ((unsigned)(eq - f.emin) << f.M) + n;                 // n < 2^(M + 1): no carry out of the binade
    if (code > (unsigned)f.max_code) {                                          // (E4M3: the magnitudes of the NaN pattern's code)
        exact = false;
        above = true;
        return (unsigned)f.max_code;
    }
    above = code == (unsigned)f.max_code && !exact;
    return code;
}

// lo and gap (fp32 bit patterns) of the finite element `bits` in a block of exponent E
__host__ __device__ __forceinline__ void mx_neighbours_of(unsigned bits, int E, const MxFormat& f, unsigned& lo, unsigned& gap) {
    const unsigned mag = bits & 0x7FFFFFFFu;
    const unsigned top = (unsigned)f.max_code;
    bool exact, above;
    const unsigned c = mx_floor_code(mag, E, f, exact, above);
    if (mag == 0u || !(bits >> 31)) {                                           // w >= 0 (-0 is 0)
        const bool pinned = c == top;                                           // w >= max X
        lo = mx_decode(c, E, f);
        gap = pinned ? 0u : pow2_bits(step_exp(c, f) + E);
    } else if (above) {                                                         // w < -max X
        lo = mx_decode(top, E, f) | 0x80000000u;
        gap = 0u;
    } else if (exact) {                                                         // on the grid (c >= 1): the next value up is code c - 1
        lo = bits;
        gap = pow2_bits(step_exp(c - 1u, f) + E);
    } else {                                                                    // between codes c and c + 1 (c + 1 <= max_code)
        lo = mx_decode(c + 1u, E, f) | 0x80000000u;
        gap = pow2_bits(step_exp(c, f) + E);
    }
}

// the layout of mx_fakequant_kernel: a block is 32 lanes, a wave two blocks, a workgroup eight; `base` is uniform over the wave, a block
// past the end only masks its accesses
__global__ __launch_bounds__(256) void mx_neighbours_kernel(const float* __restrict__ w, long total, long nb, long inner, MxFormat f,
                                                            float* __restrict__ lo, float* __restrict__ gap, uint8_t* __restrict__ scales) {
    const int lane = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const long stride = (long)gridDim.x * 8;
    for (long base = (long)blockIdx.x * 8 + ((threadIdx.x >> 6) << 1); base < total; base += stride) {
        const long g = base + half;
        const long row = g / nb, b = g - row * nb;
        const long i = b * kBlock + lane;
        const bool live = g < total && i < inner;
        const long at = row * inner + i;
        const unsigned bits = live ? __builtin_bit_cast(unsigned, w[at]) : 0u;
        const unsigned amax = half_wave_max(bits & 0x7FFFFFFFu);
        const bool finite = amax < 0x7F800000u;
        const int E = finite ? mx_block_exponent(amax, f) : -127;
        unsigned lb = 0x7FC00000u, gb = 0u;
        if (finite) mx_neighbours_of(bits, E, f, lb, gb);
        if (live) {
            lo[at] = __builtin_bit_cast(float, lb);
            gap[at] = __builtin_bit_cast(float, gb);
            if (scales && lane == 0) scales[g] = (uint8_t)(finite ? E + 127 : 255);
        }
    }
}

// ---- init, forward ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mx_init_kernel(const float* __restrict__ w, const float* __restrict__ lo, const float* __restrict__ gap,
                                                      long numel, float* __restrict__ alpha) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (long)gridDim.x * blockDim.x) {
        const float gp = gap[e];
        float a = 0.f;
        if (gp > 0.f) a = ada_alpha0((w[e] - lo[e]) / gp);
        alpha[e] = a;
    }
}

// The MX grid of one weight (ada_element's Grid): lo is on the grid and so is lo + gap -- no level clamp, dq/dh = gap everywhere
struct MxGrid {
    float lo, gap;
    __device__ __forceinline__ float q(float h) const { return lo + gap * h; }
    __device__ __forceinline__ float dq_dh(float g, float) const { return g * gap; }
};

__global__ __launch_bounds__(256) void mx_fwd_kernel(rdo_ada_desc d, const float* __restrict__ lo, const float* __restrict__ gap,
                                                     const float* __restrict__ alpha, int soft, float* __restrict__ wq, float* __restrict__ wd,
                                                     uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, long nb, MxFormat f) {
    const long inner = d.numel / d.rows;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < d.numel; e += (long)gridDim.x * blockDim.x) {
        const float h = ada_h(alpha[e], soft != 0);
        const float q = MxGrid{lo[e], gap[e]}.q(h);                             // hard: lo or lo + gap, exact
        if (codes) {
            const long row = e / inner;
            const unsigned sc = scales[row * nb + (e - row * inner) / kBlock];
            const unsigned qb = __builtin_bit_cast(unsigned, q);
            unsigned code = 0u;
            if (sc != 255u) code = mx_encode(qb & 0x7FFFFFFFu, (int)sc - 127, f) | ((qb & 0x80000000u) >> (32 - f.bits));
            codes[e] = (uint8_t)code;
        }
        emit(d, e, q, wq, wd);
    }
}

// ---- the fused step --------------------------------------------------------------------------------------------------------------------
struct MxStepArgs {
    rdo_ada_desc d;
    const float* lo;
    const float* gap;
    const float* slabs;     // [nsplit][numel] data gradient w.r.t. the kernel-layout weight (w~ or gamma')
    int nsplit;
    float grad_scale, round_weight;
    const rdo_sched_row* sched;
    const int32_t* iter_ptr;
    float* alpha;
    float* m;
    float* v;
    float* wq;
    float* round_loss_out;
};

// One thread per W consecutive elements (16-byte accesses on every stream with W = 4: lo, gap, alpha, m, v, nsplit slabs, wq).
template <int W>   // W = 4: float4 streams (numel % 4 == 0); W = 1: scalar form for odd-sized tensors
__global__ __launch_bounds__(256) void mx_step_kernel(MxStepArgs a) {
    typedef float vec_t __attribute__((ext_vector_type(W)));
    const rdo_ada_desc d = a.d;
    const int it = *a.iter_ptr;
    const rdo_sched_row sc = a.sched[it];
    float rl_local = 0.f;
    const long nq = d.numel / W;
    for (long qi = (long)blockIdx.x * blockDim.x + threadIdx.x; qi < nq; qi += (long)gridDim.x * blockDim.x) {
        // ---- load the streams
        const long e0 = qi * W;
        const vec_t lo4 = *reinterpret_cast<const vec_t*>(a.lo + e0);
        const vec_t gp4 = *reinterpret_cast<const vec_t*>(a.gap + e0);
        vec_t al4 = *reinterpret_cast<const vec_t*>(a.alpha + e0);
        const vec_t g4 = slab_sum(lo4 * 0.f, a.slabs + e0, a.nsplit, d.numel);
        vec_t m4 = *reinterpret_cast<const vec_t*>(a.m + e0);
        vec_t v4 = *reinterpret_cast<const vec_t*>(a.v + e0);
        vec_t o4 = lo4;
        bool any_pinned = false;
        // ---- the element step (mode 0)
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const MxGrid grid{lo4[k], gp4[k]};
            if (!(grid.gap > 0.f)) {                                            // pinned (or a non-finite block): the weight stays lo
                any_pinned = true;
                o4[k] = lower_bound_fwd(d, grid.lo);
                continue;
            }
            ada_element(grid, d, 0, k, g4, al4, m4, v4, o4, a.grad_scale, a.round_weight, sc.b, sc.round_on, sc.step_size, sc.bc2_sqrt, rl_local);
        }
        // ---- store the state and the next soft weight
        if (!any_pinned) {
            *reinterpret_cast<vec_t*>(a.m + e0) = m4;
            *reinterpret_cast<vec_t*>(a.v + e0) = v4;
            *reinterpret_cast<vec_t*>(a.alpha + e0) = al4;
        } else {                                                                // a pinned element's alpha, m and v are never written
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (gp4[k] > 0.f) {
                    a.m[e0 + k] = m4[k];
                    a.v[e0 + k] = v4[k];
                    a.alpha[e0 + k] = al4[k];
                }
            }
        }
        *reinterpret_cast<vec_t*>(a.wq + e0) = o4;
    }
    publish_round_loss(a.round_loss_out, sc.round_on, it, blockIdx.x, rl_local);
}

// the dgrad layout, a second launch: wd_transpose_body without plane outputs
__global__ __launch_bounds__(256) void mx_wd_transpose_kernel(rdo_ada_desc d, const float* __restrict__ wq, float* __restrict__ wd) {
    wd_transpose_body(d, wq, wd, nullptr, 0.f, nullptr, blockIdx.x);
}

using rdo::grid_for;

inline bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace

extern "C" {

int rdo_mx_neighbours(const float* w, int32_t rows, int64_t inner, int32_t format, float* lo, float* gap, uint8_t* scales, void* stream) {
    RDO_REQUIRE(w && lo && gap, "rdo_mx_neighbours: null pointer");
    RDO_REQUIRE(rows > 0 && inner > 0, "rdo_mx_neighbours: non-positive size rows %d inner %lld", rows, (long long)inner);
    MxFormat f;
    RDO_REQUIRE(mx_format(format, f), "rdo_mx_neighbours: unknown format %d (0 .. %d)", format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(aligned4(w) && aligned4(lo) && aligned4(gap), "rdo_mx_neighbours: w, lo and gap must be 4-byte aligned");
    long nb = 0;
    const long total = mx_blocks(rows, inner, nb);
    RDO_REQUIRE(total > 0, "rdo_mx_neighbours: rows %d of inner %lld make more than 2^40 blocks", rows, (long long)inner);
    const long in = (long)inner;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_neighbours_kernel, dim3(mx_grid(total)), dim3(256), 0, s, w, total, nb, in, f, lo, gap, scales);
            return rdo::check_launch("mx_neighbours");
        },
        stream, "mx_neighbours", 0.0, (double)rows * (double)inner * 12.0);
}

int rdo_mx_round_init_alpha(const float* w, const float* lo, const float* gap, int64_t numel, float* alpha, void* stream) {
    RDO_REQUIRE(w && lo && gap && alpha, "rdo_mx_round_init_alpha: null pointer");
    RDO_REQUIRE(numel > 0, "rdo_mx_round_init_alpha: non-positive size numel %lld", (long long)numel);
    RDO_REQUIRE(aligned4(w) && aligned4(lo) && aligned4(gap) && aligned4(alpha), "rdo_mx_round_init_alpha: pointers must be 4-byte aligned");
    const long n = (long)numel;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_init_kernel, dim3(grid_for(n)), dim3(256), 0, s, w, lo, gap, n, alpha);
            return rdo::check_launch("mx_round_init");
        },
        stream, "mx_round_init", 0.0, 16.0 * (double)numel);
}

int rdo_mx_round_fwd(const rdo_ada_desc* d, const float* lo, const float* gap, const float* alpha, int32_t soft, float* wq, float* wd,
                     uint8_t* codes, const uint8_t* scales_in, int32_t format, void* stream) {
    if (int rc = check_desc(d, "rdo_mx_round_fwd", false)) return rc;
    RDO_REQUIRE(lo && gap && alpha && wq, "rdo_mx_round_fwd: null pointer");
    MxFormat f;
    RDO_REQUIRE(mx_format(format, f), "rdo_mx_round_fwd: unknown format %d (0 .. %d)", format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(aligned4(lo) && aligned4(gap) && aligned4(alpha) && aligned4(wq) && aligned4(wd),
                "rdo_mx_round_fwd: lo, gap, alpha, wq and wd must be 4-byte aligned");
    RDO_REQUIRE(!codes || !soft, "rdo_mx_round_fwd: codes describe the hard weight (soft must be 0)");
    RDO_REQUIRE(!codes || scales_in, "rdo_mx_round_fwd: codes need the block scales scales_in");
    const rdo_ada_desc dd = *d;
    const long nb = (long)rdo::ceil_div(dd.numel / dd.rows, (int64_t)kBlock);
    const int sf = soft ? 1 : 0;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_fwd_kernel, dim3(grid_for(dd.numel)), dim3(256), 0, s, dd, lo, gap, alpha, sf, wq, wd, codes, scales_in, nb, f);
            return rdo::check_launch("mx_round_fwd");
        },
        stream, "mx_round_fwd", 0.0, 16.0 * (double)dd.numel);
}

int rdo_mx_round_step(const rdo_ada_desc* d, const float* lo, const float* gap, const float* slabs, int32_t nsplit, float grad_scale,
                      float round_weight, const rdo_sched_row* sched, const int32_t* iter_ptr, float* alpha, float* adam_m, float* adam_v,
                      float* wq, float* wd, float* round_loss_out, void* stream) {
    if (int rc = check_desc(d, "rdo_mx_round_step", false)) return rc;
    RDO_REQUIRE(lo && gap && slabs && sched && iter_ptr && alpha && adam_m && adam_v && wq, "rdo_mx_round_step: null pointer");
    RDO_REQUIRE(nsplit >= 1, "rdo_mx_round_step: nsplit %d (at least one gradient slab)", nsplit);
    RDO_REQUIRE(aligned4(lo) && aligned4(gap) && aligned4(slabs) && aligned4(sched) && aligned4(iter_ptr) && aligned4(alpha) && aligned4(adam_m) &&
                aligned4(adam_v) && aligned4(wq) && aligned4(wd) && aligned4(round_loss_out), "rdo_mx_round_step: pointers must be 4-byte aligned");
    // the float4 form reads and writes 16 bytes at a time (slab s starts at slabs + s * numel: aligned with slabs when numel % 4 == 0);
    // streams that are only 4-byte aligned take the scalar form
    auto a16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const bool vec = d->numel % 4 == 0 && a16(lo) && a16(gap) && a16(slabs) && a16(alpha) && a16(adam_m) && a16(adam_v) && a16(wq);
    MxStepArgs a{};
    a.d = *d; a.lo = lo; a.gap = gap; a.slabs = slabs; a.nsplit = nsplit; a.grad_scale = grad_scale; a.round_weight = round_weight;
    a.sched = sched; a.iter_ptr = iter_ptr; a.alpha = alpha; a.m = adam_m; a.v = adam_v; a.wq = wq; a.round_loss_out = round_loss_out;
    return rdo::dispatch(
        [=](hipStream_t s) {
            if (vec)
                hipLaunchKernelGGL(mx_step_kernel<4>, dim3(grid_for(a.d.numel / 4)), dim3(256), 0, s, a);
            else
                hipLaunchKernelGGL(mx_step_kernel<1>, dim3(grid_for(a.d.numel)), dim3(256), 0, s, a);
            if (wd && a.d.Cin > 0) {
                const long blocks = tile_blocks(a.d);
                hipLaunchKernelGGL(mx_wd_transpose_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.d, (const float*)a.wq, wd);
            }
            return rdo::check_launch("mx_round_step");
        },
        stream, "mx_round_step", 0.0, 4.0 * a.d.numel * (nsplit + 9.0));
}

}  // extern "C"
