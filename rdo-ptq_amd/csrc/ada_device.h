// What the learned-rounding (AdaRound) step kernels share: adaround.hip (integer grids; the flat and the tile form) and mx_round.hip
// (the grids of the MX block formats).  The single statement of the per-element arithmetic -- h(alpha) and its slope, the LowerBound
// chain of a GDN gamma, the rounding regulariser, torch's Adam, the next soft weight -- and of what stands around it: the slab sum, the
// plane stores, the rounding-loss publish, the dgrad layout, the descriptor check.  A caller supplies its grid (q(h) and dq/dh, see
// ada_element) and its layouts.  Both callers are built with -ffp-contract=off so products and sums round separately, as the
// reference's op chain does.  Included once per translation unit, hence the unnamed namespace.
#pragma once
#include "rdo_common.h"

// ablation switch of a diagnostic build (make DIAG=1): adaround.hip defines it over its device word before it includes this file;
// everywhere else, and in the default library, no switch changes results
#ifndef ADA_ABL
#define ADA_ABL(bit) false
#endif

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float kGamma = -0.1f, kZeta = 1.1f;
constexpr float kBeta2 = 0.999f, kAdamEps = 1e-8f;
// 1 - beta as torch.optim.Adam forms it (in double, then one rounding): 1.f - 0.999f is 1.3e-5 below 0.001, and until
// tests/test_gpu_adaround_step.py read adam_v against float64 every second moment carried that factor.  beta1 = 0.9 enters as 1 - beta1 only.
constexpr float kOmBeta1 = (float)(1.0 - 0.9), kOmBeta2 = (float)(1.0 - 0.999);

__device__ __forceinline__ float sigmoidf_(float a) { return 1.0f / (1.0f + __expf(-a)); }

// u^p for u in [0, 1], p in [1, 19] (the rounding regulariser's (2|h - 1/2|)^(b-1)) on the transcendental unit: exp2(p * log2 u).
// HIP's __powf is the correctly rounded library pow -- ~190 instructions, more than the rest of an element's step together and
// ~150 us of every calibration step of the Cheng2020 schedule (tools/ada_step_ablate.py, profiles/r06a_ada_step_ablate.md).  v_log_f32 /
// v_exp_f32 are good to 1 ulp of their results: the power's relative error is <= 4e-8 * |p log2 u|, i.e. <= 3 ulp wherever the
// result is above 1e-3 and an absolute error below 1e-9 everywhere else (the term is a regulariser's value and slope next to a data
// gradient that carries the fp32 summation-order noise of 65 536-pixel reductions).
__device__ __forceinline__ float pow_u(float u, float p) {
    return (u > 0.f) ? __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(u) * p) : 0.f;
}

// ---- h(alpha) ----------------------------------------------------------------------------------------------------------------------------
// the rectified sigmoid h(alpha) = clamp(sigmoid(alpha) * (zeta - gamma) + gamma, 0, 1) and its slope (0 where the clamp holds)
struct AdaH {
    float h, dh_da;
};
__device__ __forceinline__ AdaH ada_h_slope(float al) {
    const float sg = sigmoidf_(al);
    const float hraw = sg * (kZeta - kGamma) + kGamma;
    const float h = fminf(fmaxf(hraw, 0.f), 1.f);
    const float pass_h = (hraw >= 0.f && hraw <= 1.f) ? 1.f : 0.f;
    return {h, pass_h * ((kZeta - kGamma) * (sg * (1.f - sg)))};
}
// forward only: the soft h, or the hard one (alpha >= 0)
__device__ __forceinline__ float ada_h(float al, bool soft) {
    return soft ? fminf(fmaxf(sigmoidf_(al) * (kZeta - kGamma) + kGamma, 0.f), 1.f) : (al >= 0.f ? 1.f : 0.f);
}
// the alpha at which h(alpha) is `rest`, the fraction of a grid step that the weight lies above the grid value below it
__device__ __forceinline__ float ada_alpha0(float rest) { return -logf((kZeta - kGamma) / (rest - kGamma) - 1.f); }

// ---- the slab sum ------------------------------------------------------------------------------------------------------------------------
// g + the nsplit gradient slabs at sp, sp + numel, ..., sixteen / eight / four / one at a time.  The order of the additions is part of
// the bit-for-bit contract between the forms; g arrives as the caller's `weight * 0.f`, which carries a non-finite weight into the sum.
// Eight and more slab loads in flight per thread: with ~5 waves per CU at these sizes a serial chain of nsplit dependent loads (one
// L2 / fabric round trip each) was the whole kernel time.
template <typename V>
__device__ __forceinline__ V slab_sum(V g, const float* sp, int nsplit, long numel) {
    int s = 0;
    for (; s + 16 <= nsplit; s += 16) {            // long chains (the 28-slab 3x3 convs, the 256-slab 1x1): sixteen in flight
        V t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = *reinterpret_cast<const V*>(sp + (long)(s + u) * numel);
        g += (((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))) +
             (((t[8] + t[9]) + (t[10] + t[11])) + ((t[12] + t[13]) + (t[14] + t[15])));
    }
    for (; s + 8 <= nsplit; s += 8) {
        V t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const V*>(sp + (long)(s + u) * numel);
        g += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    }
    if (s + 4 <= nsplit) {
        V t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const V*>(sp + (long)(s + u) * numel);
        g += (t[0] + t[1]) + (t[2] + t[3]);
        s += 4;
    }
    for (; s < nsplit; ++s) g += *reinterpret_cast<const V*>(sp + (long)s * numel);
    return g;
}

// ---- the LowerBound chain of a GDN gamma (quant_layer.py:142-146): gamma' = max(q, bound)^2 - pedestal ---------------------------------
__device__ __forceinline__ float lower_bound_fwd(const rdo_ada_desc& d, float q) {
    if (!d.reparam) return q;
    const float lb = fmaxf(q, d.reparam_bound);
    return lb * lb - d.reparam_pedestal;
}
// the gradient w.r.t. q from the one w.r.t. gamma' (CompressAI's rule: below the bound only a gradient that raises q passes)
__device__ __forceinline__ float lower_bound_bwd(const rdo_ada_desc& d, float q, float g) {
    if (!d.reparam) return g;
    const float lb = fmaxf(q, d.reparam_bound);
    const float go = g * (2.f * lb);                      // d(lb^2)/dlb
    return (q >= d.reparam_bound || go < 0.f) ? go : 0.f;
}

// ---- rounding regulariser + Adam ---------------------------------------------------------------------------------------------------------
// One Adam step of an element's alpha from its data gradient g_alpha: adds the regulariser's value AT THE CURRENT alpha (h, dh_da) to the
// thread's rounding-loss partial and its gradient to g_alpha * grad_scale.  b, round_on, step_size and bc2 are the schedule row's fields.
// al, m and v are the element's alpha and Adam moments, stepped in place.
__device__ __forceinline__ void ada_reg_adam(float g_alpha, AdaH hs, float& al, float& m, float& v, float grad_scale, float round_weight, float b,
                                             float round_on, float step_size, float bc2, float& rl_local) {
    // rounding regulariser (value of the current alpha, gradient through h)
    float g_total = g_alpha * grad_scale;
    if (round_on != 0.f && !ADA_ABL(4)) {
        const float u = fabsf(hs.h - 0.5f) * 2.f;
        const float ub1 = pow_u(u, b - 1.f);                       // u^(b-1); u^b = u * u^(b-1)
        rl_local += round_weight * (1.f - u * ub1);
        const float sgn = (hs.h > 0.5f) ? 1.f : ((hs.h < 0.5f) ? -1.f : 0.f);
        g_total += (-round_weight * (b * ub1) * 2.f * sgn) * hs.dh_da;
    }
    // Adam (torch.optim.Adam defaults; alpha has no weight decay)
    m = fmaf(g_total - m, kOmBeta1, m);                            // lerp as one fma: a single rounding behind the difference
    v = fmaf(v, kBeta2, kOmBeta2 * g_total * g_total);
    const float denom = sqrtf(v) / bc2 + kAdamEps;
    al = al - step_size * (m / denom);
}

// ---- the element step --------------------------------------------------------------------------------------------------------------------
// What a caller supplies is its grid, as the soft weight q(h) and the chain through it:
//   float q(float h)                the weight at rounding fraction h
//   float dq_dh(float g, float h)   g * dq/dh there
// (integer grid: q = (clamp(floor(w / delta) + h + zp, 0, L - 1) - zp) * delta, dq/dh = delta inside the clamp; MX grid: q = lo + gap * h,
// dq/dh = gap).  g is the summed data gradient w.r.t. the kernel-layout weight (mode 0, 1) or already the one w.r.t. alpha (mode 2).
// Works on element k of the thread's vectors (V: W floats; a reference cannot bind to one element of an ext_vector_type, and scalar
// in / out parameters would leave the compiler other merges to vectorise than the hand-written forms had).  mode 1 leaves the data gradient
// w.r.t. alpha in o[k] and al, m, v alone; modes 0 and 2 step al[k], m[k], v[k] and leave the next iteration's soft weight in o[k].
template <typename Grid, typename V>
__device__ __forceinline__ void ada_element(const Grid& grid, const rdo_ada_desc& d, int mode, int k, const V& g, V& al, V& m, V& v, V& o,
                                            float grad_scale, float round_weight, float b, float round_on, float step_size, float bc2,
                                            float& rl_local) {
    const AdaH hs = ada_h_slope(al[k]);
    float g_alpha = g[k];
    if (mode != 2) g_alpha = grid.dq_dh(lower_bound_bwd(d, grid.q(hs.h), g[k]), hs.h) * hs.dh_da;
    if (mode == 1) {
        o[k] = g_alpha;
        return;
    }
    float a1 = al[k], m1 = m[k], v1 = v[k];
    ada_reg_adam(g_alpha, hs, a1, m1, v1, grad_scale, round_weight, b, round_on, step_size, bc2, rl_local);
    m[k] = m1; v[k] = v1; al[k] = a1;
    o[k] = lower_bound_fwd(d, grid.q(ada_h(a1, true)));
}

// ---- stores ------------------------------------------------------------------------------------------------------------------------------
// exact three-way bf16 split (hardware RNE conversions), as rdo_split_bf16x3
__device__ __forceinline__ void split3(float v, unsigned short& h, unsigned short& m, unsigned short& l) {
    const __bf16 hb = (__bf16)v;
    const float r1 = v - (float)hb;
    const __bf16 mb = (__bf16)r1;
    const __bf16 lb = (__bf16)(r1 - (float)mb);
    h = __builtin_bit_cast(unsigned short, hb);
    m = __builtin_bit_cast(unsigned short, mb);
    l = __builtin_bit_cast(unsigned short, lb);
}
// element i of planes [3][n]
__device__ __forceinline__ void split3_store(float v, unsigned short* planes, long n, long i) {
    unsigned short h, m, l;
    split3(v, h, m, l);
    planes[i] = h;
    planes[n + i] = m;
    planes[2 * n + i] = l;
}
// four values -> planes [3][n] at f0 .. f0 + 3: one 8-byte store per plane
__device__ __forceinline__ void split3_store4(f32x4 o, unsigned short* planes, long n, long f0) {
    typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
    u16x4 ph, pm, pl;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned short h, m, l;
        split3(o[k], h, m, l);
        ph[k] = h; pm[k] = m; pl[k] = l;
    }
    *reinterpret_cast<u16x4*>(planes + f0) = ph;
    *reinterpret_cast<u16x4*>(planes + n + f0) = pm;
    *reinterpret_cast<u16x4*>(planes + 2 * n + f0) = pl;
}
// four values -> the fp16 two-way split of o * scale, planes [2][n] at f0 .. f0 + 3: one 8-byte store per plane
__device__ __forceinline__ void h2_store4(f32x4 o, float scale, unsigned short* planes, long n, long f0, int& bad) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x2 ph, pl;
    unsigned h, l;
    rdo::h2_split_pk(o[0], o[1], scale, h, l, bad); ph[0] = h; pl[0] = l;
    rdo::h2_split_pk(o[2], o[3], scale, h, l, bad); ph[1] = h; pl[1] = l;
    *reinterpret_cast<u32x2*>(planes + f0) = ph;
    *reinterpret_cast<u32x2*>(planes + n + f0) = pl;
}

// the workgroup's rounding loss into its slot of iteration `it`.  Every thread of the workgroup makes the call (block_sum holds a
// barrier): the condition holds kernel arguments and the schedule row only, uniform over the workgroup.
__device__ __forceinline__ void publish_round_loss(float* out, float round_on, int it, long bid, float rl_local) {
    if (out && round_on != 0.f) {
        const float t = rdo::block_sum(rl_local);
        if (threadIdx.x == 0) {
            if (t != 0.f) atomicAdd(out + (long)it * RDO_LOG_SLOTS + (bid & (RDO_LOG_SLOTS - 1)), t);
        }
    }
}

// ---- the dgrad layout --------------------------------------------------------------------------------------------------------------------
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

// emit kernel-layout weight(s) from the quantised value
__device__ __forceinline__ void emit(const rdo_ada_desc& d, long e, float q, float* wq, float* wd) {
    const float o = lower_bound_fwd(d, q);
    wq[e] = o;
    if (wd && d.Cin > 0) wd[wd_index(d, e)] = o;
}

// the workgroup's 32 x 32 transpose tile in LDS (rows padded to 33 words: a column read meets 32 different banks); one per kernel
__device__ __forceinline__ float (&lds_tile32())[32][33] {
    __shared__ float tile[32][33];
    return tile;
}

// wd[ci][KH-1-kh][KW-1-kw][co] = wq[co][kh][kw][ci]: 32x32 tiles through LDS, 128-byte segments on both sides.  wd_planes (nullable): the
// planes of wd -- the fp16 two-way split of wd * pscale, or with pscale == 0 the three-way bf16 split
__device__ __forceinline__ void wd_transpose_body(const rdo_ada_desc& d, const float* wq, float* wd, unsigned short* wd_planes, float pscale,
                                                  int* ovf, int bid) {
    const int taps = d.KH * d.KW, cdim = d.Cin;
    const int ctiles = (cdim + 31) / 32;
    const int ct = bid % ctiles; bid /= ctiles;
    const int tap = bid % taps;
    const int rt = bid / taps;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float(&tile)[32][33] = lds_tile32();
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
        if (ci < cdim && co < d.rows) {
            const long o = ((long)ci * taps + tapf) * d.rows + co;
            wd[o] = tile[tx][ty + 8 * k];
            // wd is the weight [Cin][KH][KW][Cout] of the dgrad conv: its planes go in that conv's fragment order
            if (wd_planes && pscale > 0.f) {
                int bad = 0;
                rdo::h2_split_store(tile[tx][ty + 8 * k], pscale, wd_planes, d.numel, rdo::frag_index(o, d.Cin, d.KH, d.KW, d.rows), bad);
                rdo::h2_report(bad, ovf);
            } else if (wd_planes) {
                split3_store(tile[tx][ty + 8 * k], wd_planes, d.numel, rdo::frag_index(o, d.Cin, d.KH, d.KW, d.rows));
            }
        }
    }
}
// its grid: the 32 x 32 tiles of a conv weight, one workgroup each (the tile form of adaround.hip's step walks the same tiles)
inline long tile_blocks(const rdo_ada_desc& d) { return rdo::ceil_div(d.rows, 32) * d.KH * d.KW * rdo::ceil_div(d.Cin, 32); }

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// levels: the descriptor is one of an integer grid and carries n_levels (an MX descriptor carries none)
inline int check_desc(const rdo_ada_desc* d, const char* who, bool levels = true) {
    RDO_REQUIRE(d != nullptr, "%s: null descriptor", who);
    RDO_REQUIRE(d->numel > 0 && d->rows > 0 && d->numel % d->rows == 0, "%s: numel %ld not divisible by rows %d", who,
                (long)d->numel, d->rows);
    RDO_REQUIRE(!levels || (d->n_levels >= 4 && d->n_levels <= 65536), "%s: n_levels %d unsupported", who, d->n_levels);
    if (d->Cin > 0)
        RDO_REQUIRE(d->KH > 0 && d->KW > 0 && (long)d->rows * d->KH * d->KW * d->Cin == d->numel,
                    "%s: conv layout [%d][%d][%d][%d] does not match numel %ld", who, d->rows, d->KH, d->KW, d->Cin,
                    (long)d->numel);
    return RDO_OK;
}

}  // namespace
