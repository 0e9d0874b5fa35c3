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
// rdo_mx_round_step restates the flat form of adaround.hip's fused step (ada_step_body: float4 streams where numel % 4 == 0, a scalar
// form otherwise, the slab loads 16 / 8 / 4 at a time, the same summation order, the same Adam constants, pow_u on the transcendental
// unit, the rounding loss by block_sum + one atomicAdd per workgroup) with `w, delta, zp` replaced by `lo, gap`; that file stays as it
// is (its step has bit-for-bit tests), hence the restated sigmoidf_, pow_u and constants.  The dgrad layout is a second launch.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxround.h"
#include "mx_device.h"

namespace {

constexpr float kGamma = -0.1f, kZeta = 1.1f;
constexpr float kBeta2 = 0.999f, kAdamEps = 1e-8f;
// 1 - beta as torch.optim.Adam forms it (in double, then one rounding), as in adaround.hip
constexpr float kOmBeta1 = (float)(1.0 - 0.9), kOmBeta2 = (float)(1.0 - 0.999);

__device__ __forceinline__ float sigmoidf_(float a) { return 1.0f / (1.0f + __expf(-a)); }

// u^p for u in [0, 1], p in [1, 19] on the transcendental unit: exp2(p * log2 u) (adaround.hip states its error)
__device__ __forceinline__ float pow_u(float u, float p) {
    return (u > 0.f) ? __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(u) * p) : 0.f;
}

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
        if (gp > 0.f) {
            const float rest = (w[e] - lo[e]) / gp;
            a = -logf((kZeta - kGamma) / (rest - kGamma) - 1.f);
        }
        alpha[e] = a;
    }
}

__device__ __forceinline__ long wd_index(const rdo_ada_desc& d, long e) {
    // e = ((co*KH + kh)*KW + kw)*Cin + ci  ->  ((ci*KH + KH-1-kh)*KW + KW-1-kw)*Cout + co
    const int Cin = d.Cin, KW = d.KW, KH = d.KH;
    long t = e / Cin;
    const int ci = (int)(e - t * Cin);
    const int kw = (int)(t % KW); t /= KW;
    const int kh = (int)(t % KH);
    const long co = t / KH;
    return (((long)ci * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)) * d.rows + co;
}

__device__ __forceinline__ float reparam_of(const rdo_ada_desc& d, float q) {
    if (!d.reparam) return q;
    const float lb = fmaxf(q, d.reparam_bound);
    return lb * lb - d.reparam_pedestal;
}

__global__ __launch_bounds__(256) void mx_fwd_kernel(rdo_ada_desc d, const float* __restrict__ lo, const float* __restrict__ gap,
                                                     const float* __restrict__ alpha, int soft, float* __restrict__ wq, float* __restrict__ wd,
                                                     uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, long nb, MxFormat f) {
    const long inner = d.numel / d.rows;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < d.numel; e += (long)gridDim.x * blockDim.x) {
        const float al = alpha[e];
        const float h = soft ? fminf(fmaxf(sigmoidf_(al) * (kZeta - kGamma) + kGamma, 0.f), 1.f) : (al >= 0.f ? 1.f : 0.f);
        const float q = lo[e] + gap[e] * h;                                     // hard: lo or lo + gap, exact
        if (codes) {
            const long row = e / inner;
            const unsigned sc = scales[row * nb + (e - row * inner) / kBlock];
            const unsigned qb = __builtin_bit_cast(unsigned, q);
            unsigned code = 0u;
            if (sc != 255u) code = mx_encode(qb & 0x7FFFFFFFu, (int)sc - 127, f) | ((qb & 0x80000000u) >> (32 - f.bits));
            codes[e] = (uint8_t)code;
        }
        const float o = reparam_of(d, q);
        wq[e] = o;
        if (wd && d.Cin > 0) wd[wd_index(d, e)] = o;
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
    const float b = sc.b, round_on = sc.round_on, step_size = sc.step_size, bc2 = sc.bc2_sqrt;
    float rl_local = 0.f;
    const long nq = d.numel / W;
    for (long qi = (long)blockIdx.x * blockDim.x + threadIdx.x; qi < nq; qi += (long)gridDim.x * blockDim.x) {
        const long e0 = qi * W;
        const vec_t lo4 = *reinterpret_cast<const vec_t*>(a.lo + e0);
        const vec_t gp4 = *reinterpret_cast<const vec_t*>(a.gap + e0);
        vec_t al4 = *reinterpret_cast<const vec_t*>(a.alpha + e0);
        vec_t g4 = lo4 * 0.f;
        {
            // the slab loads in flight as in ada_step_body: a serial chain of nsplit dependent loads was that kernel's whole time
            const float* sp = a.slabs + e0;
            int s = 0;
            for (; s + 16 <= a.nsplit; s += 16) {
                vec_t t[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) t[u] = *reinterpret_cast<const vec_t*>(sp + (long)(s + u) * d.numel);
                g4 += (((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))) +
                      (((t[8] + t[9]) + (t[10] + t[11])) + ((t[12] + t[13]) + (t[14] + t[15])));
            }
            for (; s + 8 <= a.nsplit; s += 8) {
                vec_t t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const vec_t*>(sp + (long)(s + u) * d.numel);
                g4 += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
            }
            if (s + 4 <= a.nsplit) {
                vec_t t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const vec_t*>(sp + (long)(s + u) * d.numel);
                g4 += (t[0] + t[1]) + (t[2] + t[3]);
                s += 4;
            }
            for (; s < a.nsplit; ++s) g4 += *reinterpret_cast<const vec_t*>(sp + (long)s * d.numel);
        }
        vec_t m4 = *reinterpret_cast<const vec_t*>(a.m + e0);
        vec_t v4 = *reinterpret_cast<const vec_t*>(a.v + e0);
        vec_t o4 = lo4;
        bool any_pinned = false;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float lo = lo4[k], gp = gp4[k];
            if (!(gp > 0.f)) {                                                  // pinned (or a non-finite block): the weight stays lo
                any_pinned = true;
                o4[k] = reparam_of(d, lo);
                continue;
            }
            float al = al4[k];
            const float sg = sigmoidf_(al);
            const float hraw = sg * (kZeta - kGamma) + kGamma;
            const float h = fminf(fmaxf(hraw, 0.f), 1.f);
            const float pass_h = (hraw >= 0.f && hraw <= 1.f) ? 1.f : 0.f;
            const float dh_da = pass_h * ((kZeta - kGamma) * (sg * (1.f - sg)));
            float g = g4[k];
            if (d.reparam) {
                const float q = lo + gp * h;
                const float lb = fmaxf(q, d.reparam_bound);
                const float go = g * (2.f * lb);                                // d(lb^2)/dlb
                g = (q >= d.reparam_bound || go < 0.f) ? go : 0.f;              // LowerBound backward
            }
            const float g_alpha = (g * gp) * dh_da;                             // hi is on the grid: no level clamp, no pass_q
            // rounding regulariser (value of the current alpha, gradient through h)
            float g_total = g_alpha * a.grad_scale;
            if (round_on != 0.f) {
                const float u = fabsf(h - 0.5f) * 2.f;
                const float ub1 = pow_u(u, b - 1.f);                            // u^(b-1); u^b = u * u^(b-1)
                rl_local += a.round_weight * (1.f - u * ub1);
                const float sgn = (h > 0.5f) ? 1.f : ((h < 0.5f) ? -1.f : 0.f);
                g_total += (-a.round_weight * (b * ub1) * 2.f * sgn) * dh_da;
            }
            // Adam (torch.optim.Adam defaults; alpha has no weight decay)
            float mm = m4[k], vv = v4[k];
            mm = fmaf(g_total - mm, kOmBeta1, mm);
            vv = fmaf(vv, kBeta2, kOmBeta2 * g_total * g_total);
            const float denom = sqrtf(vv) / bc2 + kAdamEps;
            al = al - step_size * (mm / denom);
            m4[k] = mm; v4[k] = vv; al4[k] = al;
            // next iteration's soft weight
            const float h2 = fminf(fmaxf(sigmoidf_(al) * (kZeta - kGamma) + kGamma, 0.f), 1.f);
            o4[k] = reparam_of(d, lo + gp * h2);
        }
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
    if (a.round_loss_out && round_on != 0.f) {
        const float t = rdo::block_sum(rl_local);           // the condition holds kernel arguments only: uniform over the workgroup
        if (threadIdx.x == 0) {
            if (t != 0.f) atomicAdd(a.round_loss_out + (long)it * RDO_LOG_SLOTS + (blockIdx.x & (RDO_LOG_SLOTS - 1)), t);
        }
    }
}

// wd[ci][KH-1-kh][KW-1-kw][co] = wq[co][kh][kw][ci]: 32x32 tiles through LDS, 128-byte segments on both sides (wd_transpose_kernel
// of adaround.hip without its plane outputs)
__global__ __launch_bounds__(256) void mx_wd_transpose_kernel(rdo_ada_desc d, const float* __restrict__ wq, float* __restrict__ wd) {
    const int taps = d.KH * d.KW, cdim = d.Cin;
    const int ctiles = (cdim + 31) / 32;
    int bid = blockIdx.x;
    const int ct = bid % ctiles; bid /= ctiles;
    const int tap = bid % taps;
    const int rt = bid / taps;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    __shared__ float tile[32][33];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = rt * 32 + ty + 8 * k, c = ct * 32 + tx;
        if (row < d.rows && c < cdim) tile[ty + 8 * k][tx] = wq[((long)row * taps + tap) * cdim + c];
    }
    __syncthreads();
    const int kh = tap / d.KW, kw = tap - kh * d.KW;
    const int tapf = (d.KH - 1 - kh) * d.KW + (d.KW - 1 - kw);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ci = ct * 32 + ty + 8 * k, co = rt * 32 + tx;
        if (ci < cdim && co < d.rows) wd[((long)ci * taps + tapf) * d.rows + co] = tile[tx][ty + 8 * k];
    }
}

using rdo::grid_for;

inline bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

int check_desc(const rdo_ada_desc* d, const char* who) {
    RDO_REQUIRE(d != nullptr, "%s: null descriptor", who);
    RDO_REQUIRE(d->numel > 0 && d->rows > 0 && d->numel % d->rows == 0, "%s: numel %ld not divisible by rows %d", who, (long)d->numel, d->rows);
    if (d->Cin > 0)
        RDO_REQUIRE(d->KH > 0 && d->KW > 0 && (long)d->rows * d->KH * d->KW * d->Cin == d->numel,
                    "%s: conv layout [%d][%d][%d][%d] does not match numel %ld", who, d->rows, d->KH, d->KW, d->Cin, (long)d->numel);
    return RDO_OK;
}

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
    if (int rc = check_desc(d, "rdo_mx_round_fwd")) return rc;
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
    if (int rc = check_desc(d, "rdo_mx_round_step")) return rc;
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
                const long blocks = rdo::ceil_div(a.d.rows, 32) * a.d.KH * a.d.KW * rdo::ceil_div(a.d.Cin, 32);
                hipLaunchKernelGGL(mx_wd_transpose_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a.d, (const float*)a.wq, wd);
            }
            return rdo::check_launch("mx_round_step");
        },
        stream, "mx_round_step", 0.0, 4.0 * a.d.numel * (nsplit + 9.0));
}

}  // extern "C"
