// K12 -- entropy-model likelihoods and the rate/distortion reductions, element-wise on NHWC tensors; the per-channel rate sums of the
// RD report (rate_channel_part_kernel below) take a likelihood tensor in either storage, [outer][C][inner].
//
// Restates (CompressAI 1.2.4 definitions, pinned only against the oracle's restatement -- SURVEY 8c "parity unpinned"):
//   EntropyBottleneck.forward (eval): z^ = round(z - median) + median ; p(z^) = |sigmoid(s*F(z^+.5)) - sigmoid(s*F(z^-.5))|,
//       F = per-channel 1-3-3-3-3-1 net with softplus(matrix) x + bias (+ tanh(factor) * tanh(.) between layers), floor 1e-9
//   GaussianConditional.forward (eval): y^ = round(y - mu) + mu ; p = Phi((.5-|y^-mu|)/s) - Phi((-.5-|y^-mu|)/s),
//       s = max(sigma, 0.11), Phi(x) = erfc(-x/sqrt2)/2, floor 1e-9
// Call sites in the reference: model forward inside save_inp_oup_data (quantization/utils.py:227,241) and Test_kodak
// (test_datasets.py:95); bpp / MSE sums of losses/losses.py:15-35 and test_datasets.py:21-33.
#include "rdo_common.h"

namespace {

constexpr int kParamsPerChannel = 58;   // 33 softplus(matrix) + 13 bias + 12 tanh(factor)

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// p: [33 matrices | 13 biases | 12 factors] of one channel (matrices already softplus'ed, factors already tanh'ed)
__device__ __forceinline__ float eb_logits(const float* p, float x) {
    const float* M = p;
    const float* Bv = p + 33;
    const float* Fv = p + 46;
    float h[3], g[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {              // layer 0: 1 -> 3
        float v = M[o] * x + Bv[o];
        h[o] = v + Fv[o] * tanhf(v);
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) {              // layers 1..3: 3 -> 3
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            float v = Bv[3 + 3 * l + o];
#pragma unroll
            for (int i = 0; i < 3; ++i) v += M[3 + 9 * l + 3 * o + i] * h[i];
            g[o] = v + Fv[3 + 3 * l + o] * tanhf(v);
        }
#pragma unroll
        for (int o = 0; o < 3; ++o) h[o] = g[o];
    }
    float v = Bv[12];                          // layer 4: 3 -> 1
#pragma unroll
    for (int i = 0; i < 3; ++i) v += M[30 + i] * h[i];
    return v;
}

__global__ __launch_bounds__(256) void eb_fwd_kernel(const float* z, const float* params, const float* medians, long n, int C,
                                                     float* zhat, float* lik) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float med = medians[c];
        const float q = rintf(z[i] - med) + med;
        const float* p = params + (long)c * kParamsPerChannel;
        const float lo = eb_logits(p, q - 0.5f), hi = eb_logits(p, q + 0.5f);
        const float t = lo + hi;
        const float sgn = t > 0.f ? -1.f : (t < 0.f ? 1.f : 0.f);
        zhat[i] = q;
        lik[i] = fmaxf(fabsf(sigm(sgn * hi) - sigm(sgn * lo)), 1e-9f);
    }
}

// value and derivative dF/dx of the cumulative-logits net (forward-mode through the five layers)
__device__ __forceinline__ float eb_logits_d(const float* p, float x, float& dFdx) {
    const float* M = p;
    const float* Bv = p + 33;
    const float* Fv = p + 46;
    float h[3], dh[3], g[3], dg[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        const float v = M[o] * x + Bv[o];
        const float th = tanhf(v);
        h[o] = v + Fv[o] * th;
        dh[o] = M[o] * (1.f + Fv[o] * (1.f - th * th));
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            float v = Bv[3 + 3 * l + o], dv = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                v += M[3 + 9 * l + 3 * o + i] * h[i];
                dv += M[3 + 9 * l + 3 * o + i] * dh[i];
            }
            const float th = tanhf(v);
            g[o] = v + Fv[3 + 3 * l + o] * th;
            dg[o] = dv * (1.f + Fv[3 + 3 * l + o] * (1.f - th * th));
        }
#pragma unroll
        for (int o = 0; o < 3; ++o) { h[o] = g[o]; dh[o] = dg[o]; }
    }
    float v = Bv[12], dv = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v += M[30 + i] * h[i];
        dv += M[30 + i] * dh[i];
    }
    dFdx = dv;
    return v;
}

// d(grad_scale * -log2 p)/dz^ of the factorised prior (z^ = the rounded value: the straight-through estimator hands it to z):
// p = |sigmoid(s hi) - sigmoid(s lo)|, hi = F(z^ + .5), lo = F(z^ - .5);  dp/dz^ = sign(.) * s * (sig'(s hi) F'(z^ + .5) - sig'(s lo) F'(z^ - .5));
// zero where the 1e-9 floor is active.
__global__ __launch_bounds__(256) void eb_bwd_kernel(const float* zhat, const float* params, long n, int C, float gscale, float* dz) {
    const float inv_ln2 = 1.4426950408889634f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float q = zhat[i];
        const float* p = params + (long)c * kParamsPerChannel;
        float dlo, dhi;
        const float lo = eb_logits_d(p, q - 0.5f, dlo), hi = eb_logits_d(p, q + 0.5f, dhi);
        const float t = lo + hi;
        const float sgn = t > 0.f ? -1.f : (t < 0.f ? 1.f : 0.f);
        const float sh = sigm(sgn * hi), sl = sigm(sgn * lo);
        const float diff = sh - sl;
        const float pr = fabsf(diff);
        float g = 0.f;
        if (pr > 1e-9f) {
            const float dp = (diff > 0.f ? 1.f : -1.f) * sgn * (sh * (1.f - sh) * dhi - sl * (1.f - sl) * dlo);
            g = -gscale * inv_ln2 / pr * dp;
        }
        dz[i] = g;
    }
}

__device__ __forceinline__ float std_cum(float x) { return 0.5f * erfcf(-0.70710678118654752440f * x); }

__global__ __launch_bounds__(256) void gc_fwd_kernel(const float* y, const float* scales, const float* means, long n,
                                                     float scale_bound, float* yhat, float* lik) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float mu = means ? means[i] : 0.f;
        const float q = rintf(y[i] - mu) + mu;
        const float v = fabsf(q - mu);
        const float s = fmaxf(scales[i], scale_bound);
        if (yhat) yhat[i] = q;
        lik[i] = fmaxf(std_cum((0.5f - v) / s) - std_cum((-0.5f - v) / s), 1e-9f);
    }
}

// d(-log2 p)/d(sigma), d(-log2 p)/d(mu) of the Gaussian conditional (y^ treated as constant, i.e. the STE of the rounding):
// p = Phi(a) - Phi(b), a = (.5 - v)/s, b = (-.5 - v)/s, v = |y^ - mu|; dp/ds = -(phi(a) a - phi(b) b)/s,
// dp/dv = -(phi(a) - phi(b))/s, dv/dmu = -sign(y^ - mu); gradients vanish where the floors (scale bound, 1e-9) are active.
__global__ __launch_bounds__(256) void gc_bwd_kernel(const float* yhat, const float* scales, const float* means, long n,
                                                     float scale_bound, float gscale, float* dscales, float* dmeans) {
    const float inv_sqrt2pi = 0.3989422804014327f, inv_ln2 = 1.4426950408889634f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float mu = means ? means[i] : 0.f;
        const float d = yhat[i] - mu;
        const float v = fabsf(d);
        const float sr = scales[i];
        const float s = fmaxf(sr, scale_bound);
        const float a = (0.5f - v) / s, b = (-0.5f - v) / s;
        const float p = std_cum(a) - std_cum(b);
        const float pa = inv_sqrt2pi * expf(-0.5f * a * a), pb = inv_sqrt2pi * expf(-0.5f * b * b);
        float ds = 0.f, dm = 0.f;
        if (p > 1e-9f) {
            const float coef = -gscale * inv_ln2 / p;             // d(-log2 p) = -dp / (p ln 2)
            if (sr >= scale_bound) ds = coef * (-(pa * a - pb * b) / s);
            const float dpdv = -(pa - pb) / s;
            const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            dm = coef * dpdv * (-sgn);
        }
        if (dscales) dscales[i] = ds;
        if (dmeans) dmeans[i] = dm;
    }
}

// out[0] += sum(-log2(lik)) * scale   (bpp numerator);  out[0] += sum((a-b)^2) * scale  (MSE numerator)
__global__ __launch_bounds__(256) void neg_log2_sum_kernel(const float* lik, long n, float scale, float* out) {
    float acc = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) acc -= log2f(lik[i]);
    acc = rdo::block_sum(acc);
    if (threadIdx.x == 0) atomicAdd(out, acc * scale);
}

__global__ __launch_bounds__(256) void sq_diff_sum_kernel(const float* a, const float* b, long n, float scale, int clamp01,
                                                          float* out) {
    float acc = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float x = a[i];
        if (clamp01) x = fminf(fmaxf(x, 0.f), 1.f);
        const float d = x - b[i];
        acc += d * d;
    }
    acc = rdo::block_sum(acc);
    if (threadIdx.x == 0) atomicAdd(out, acc * scale);
}

// The same two sums without atomics, for evaluation (PSNR / bpp of a saved model must be the same numbers on every run): every
// workgroup leaves its partial sum in part[blockIdx.x], one workgroup folds them in a fixed order and adds the total to out[0].
template <bool LOG2>
__global__ __launch_bounds__(256) void ordered_part_kernel(const float* a, const float* b, long n, float scale, int clamp01, float* part) {
    float acc = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (LOG2) {
            acc -= log2f(a[i]);
        } else {
            float x = a[i];
            if (clamp01) x = fminf(fmaxf(x, 0.f), 1.f);
            const float d = x - b[i];
            acc += d * d;
        }
    }
    acc = rdo::block_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc * scale;
}

__global__ __launch_bounds__(256) void ordered_fold_kernel(const float* part, int nblk, float* out) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += part[i];
    acc = rdo::block_sum(acc);
    if (threadIdx.x == 0) out[0] += acc;
}
using rdo::grid_for;
constexpr int kOrderedBlocks = rdo::kGridCap;      // one partial sum per workgroup of grid_for

// ---- per-channel rate sums (the RD report): out[c] = sum over (o, i) of -log2f(lik[((o C) + c) inner + i]), the expression of
// neg_log2_sum_kernel.  A channel holds n = outer * inner elements, numbered j = o * inner + i.  A thread is (element lane pl, channel):
// cpb channels side by side and PL = 256 / cpb element lanes of them in a workgroup, S workgroups (blockIdx.x) down a channel's elements,
// blockIdx.y over the groups of cpb channels; lane pl of workgroup s adds the elements j = s PL + pl, + S PL, .. serially.
//   inner > 1 (NCHW):          cpb = 1, PL = 256: the 256 threads read 256 consecutive j of ONE channel, i.e. runs of `inner` adjacent
//                              addresses (one run of 256 when inner >= 256, sixteen 64-byte runs when inner = 16)
//   inner = 1 (channels-last): cpb = min(C, 64), PL = 256 / cpb: thread t reads channel t % cpb of pixel t / cpb -- adjacent lanes,
//                              adjacent addresses (for C < 64 the whole workgroup reads one contiguous run of PL C floats)
// Then the PL lanes of a channel fold through LDS as a binary tree (lane pl += lane pl + h for h = 128, 64, .., 1 while pl + h < PL),
// part[c][s] = the workgroup's sum, and the fold kernel adds a channel's S partial sums: sixteen lanes, lane j the entries j, j + 16, ..
// serially, then the xor tree 8, 4, 2, 1.  No atomics, every word of `part` that is read was written by this call, and a thread, an
// LDS tree and a fold group only ever hold values of ONE channel: a NaN stays in its channel.
constexpr int kRcSlices = 256;         // most workgroups down one channel
struct RcGeom { int cpb, PL, S, cblocks; };
inline RcGeom rc_geom(int64_t outer, int32_t C, int64_t inner) {
    RcGeom g;
    g.cpb = inner == 1 ? (C < 64 ? C : 64) : 1;
    g.PL = 256 / g.cpb;
    const int64_t s = rdo::ceil_div(outer * inner, (int64_t)g.PL * 8);      // >= 8 elements a lane before a second workgroup pays
    g.S = (int)(s > kRcSlices ? kRcSlices : s);
    g.cblocks = (int)rdo::ceil_div(C, g.cpb);
    return g;
}
// the arguments the index arithmetic supports: j and j + S PL in 32 bits unsigned, blockIdx.y <= 65535, addresses in 64 bits
inline bool rc_supported(int64_t outer, int32_t C, int64_t inner) {
    return outer > 0 && C > 0 && inner > 0 && C <= 65535 && outer <= 0x7fffffffLL && inner <= 0x7fffffffLL && outer * inner <= 0x7fffffffLL;
}

template <bool NCHW>
__global__ __launch_bounds__(256) void rate_channel_part_kernel(const float* lik, unsigned n, int C, unsigned inner, int cpb, int PL,
                                                                float* part) {
    __shared__ float sm[256];
    const int pl = threadIdx.x / cpb, cl = threadIdx.x - pl * cpb;
    const int c = blockIdx.y * cpb + cl;
    const bool live = pl < PL && c < C;
    float acc = 0.f;
    if (live) {
        const unsigned step = gridDim.x * PL;
        for (unsigned j = blockIdx.x * PL + pl; j < n; j += step) {
            long a;
            if (NCHW) {
                const unsigned o = j / inner;
                a = ((long)o * C + c) * inner + (j - o * inner);
            } else {
                a = (long)j * C + c;
            }
            acc -= log2f(lik[a]);
        }
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (live && pl < h && pl + h < PL) sm[threadIdx.x] += sm[threadIdx.x + h * cpb];
        __syncthreads();
    }
    if (live && pl == 0) part[(long)c * gridDim.x + blockIdx.x] = sm[cl];
}

__global__ __launch_bounds__(256) void rate_channel_fold_kernel(const float* part, int S, int C, float* out) {
    const int c = blockIdx.x * 16 + (threadIdx.x >> 4), j = threadIdx.x & 15;
    float r = 0.f;
    if (c < C)
        for (int b = j; b < S; b += 16) r += part[(long)c * S + b];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) r += __shfl_xor(r, o, 16);
    if (c < C && j == 0) out[c] = r;
}

}  // namespace

extern "C" {

int rdo_factorized_likelihood_fwd(const float* z, const float* params, const float* medians, int64_t n, int32_t C, float* zhat,
                                  float* lik, void* stream) {
    RDO_REQUIRE(z && params && medians && zhat && lik && n > 0 && C > 0, "rdo_factorized_likelihood_fwd: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(eb_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, z, params, medians, (long)n, C, zhat, lik);
            return rdo::check_launch("factorized_likelihood_fwd");
        },
        stream, "entropy", 0.0, 12.0 * n);
}

int rdo_factorized_likelihood_bwd(const float* zhat, const float* params, int64_t n, int32_t C, float grad_scale, float* dz, void* stream) {
    RDO_REQUIRE(zhat && params && dz && n > 0 && C > 0, "rdo_factorized_likelihood_bwd: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(eb_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, zhat, params, (long)n, C, grad_scale, dz);
            return rdo::check_launch("factorized_likelihood_bwd");
        },
        stream, "entropy", 0.0, 8.0 * n);
}

int rdo_gaussian_likelihood_fwd(const float* y, const float* scales, const float* means, int64_t n, float scale_bound, float* yhat,
                                float* lik, void* stream) {
    RDO_REQUIRE(y && scales && lik && n > 0, "rdo_gaussian_likelihood_fwd: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(gc_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, y, scales, means, (long)n, scale_bound, yhat, lik);
            return rdo::check_launch("gaussian_likelihood_fwd");
        },
        stream, "entropy", 0.0, 20.0 * n);
}

int rdo_gaussian_likelihood_bwd(const float* yhat, const float* scales, const float* means, int64_t n, float scale_bound,
                                float grad_scale, float* dscales, float* dmeans, void* stream) {
    RDO_REQUIRE(yhat && scales && (dscales || dmeans) && n > 0, "rdo_gaussian_likelihood_bwd: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(gc_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, yhat, scales, means, (long)n, scale_bound,
                               grad_scale, dscales, dmeans);
            return rdo::check_launch("gaussian_likelihood_bwd");
        },
        stream, "entropy", 0.0, 20.0 * n);
}

int rdo_neg_log2_sum(const float* lik, int64_t n, float scale, float* out, void* stream) {
    RDO_REQUIRE(lik && out && n > 0, "rdo_neg_log2_sum: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(neg_log2_sum_kernel, dim3(grid_for(n)), dim3(256), 0, s, lik, (long)n, scale, out);
            return rdo::check_launch("neg_log2_sum");
        },
        stream, "entropy", 0.0, 4.0 * n);
}

int rdo_sq_diff_sum(const float* a, const float* b, int64_t n, float scale, int32_t clamp01, float* out, void* stream) {
    RDO_REQUIRE(a && b && out && n > 0, "rdo_sq_diff_sum: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(sq_diff_sum_kernel, dim3(grid_for(n)), dim3(256), 0, s, a, b, (long)n, scale, clamp01, out);
            return rdo::check_launch("sq_diff_sum");
        },
        stream, "entropy", 0.0, 8.0 * n);
}

int64_t rdo_ordered_sum_workspace(void) { return kOrderedBlocks; }

int rdo_neg_log2_sum_ordered(const float* lik, int64_t n, float scale, float* out, float* ws, void* stream) {
    RDO_REQUIRE(lik && out && ws && n > 0, "rdo_neg_log2_sum_ordered: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            const unsigned g = grid_for(n);
            hipLaunchKernelGGL(ordered_part_kernel<true>, dim3(g), dim3(256), 0, s, lik, (const float*)nullptr, (long)n, scale, 0, ws);
            hipLaunchKernelGGL(ordered_fold_kernel, dim3(1), dim3(256), 0, s, ws, (int)g, out);
            return rdo::check_launch("neg_log2_sum_ordered");
        },
        stream, "entropy", 0.0, 4.0 * n);
}

int rdo_sq_diff_sum_ordered(const float* a, const float* b, int64_t n, float scale, int32_t clamp01, float* out, float* ws, void* stream) {
    RDO_REQUIRE(a && b && out && ws && n > 0, "rdo_sq_diff_sum_ordered: bad argument");
    return rdo::dispatch(
        [=](hipStream_t s) {
            const unsigned g = grid_for(n);
            hipLaunchKernelGGL(ordered_part_kernel<false>, dim3(g), dim3(256), 0, s, a, b, (long)n, scale, clamp01, ws);
            hipLaunchKernelGGL(ordered_fold_kernel, dim3(1), dim3(256), 0, s, ws, (int)g, out);
            return rdo::check_launch("sq_diff_sum_ordered");
        },
        stream, "entropy", 0.0, 8.0 * n);
}

int64_t rdo_neg_log2_channel_sums_workspace(int64_t outer, int32_t C, int64_t inner) {
    return rc_supported(outer, C, inner) ? (int64_t)C * rc_geom(outer, C, inner).S : 0;
}

int rdo_neg_log2_channel_sums(const float* lik, int64_t outer, int32_t C, int64_t inner, float* out, float* ws, void* stream) {
    RDO_REQUIRE(lik && out && ws && outer > 0 && C > 0 && inner > 0, "rdo_neg_log2_channel_sums: bad argument");
    RDO_REQUIRE(rc_supported(outer, C, inner),
                "rdo_neg_log2_channel_sums: outer %lld x C %d x inner %lld is beyond the index arithmetic (C <= 65535, outer * inner < 2^31)",
                (long long)outer, C, (long long)inner);
    return rdo::dispatch(
        [=](hipStream_t s) {
            const RcGeom g = rc_geom(outer, C, inner);
            const unsigned n = (unsigned)(outer * inner);
            if (inner == 1)
                hipLaunchKernelGGL(rate_channel_part_kernel<false>, dim3(g.S, g.cblocks), dim3(256), 0, s, lik, n, C, 1u, g.cpb, g.PL, ws);
            else
                hipLaunchKernelGGL(rate_channel_part_kernel<true>, dim3(g.S, g.cblocks), dim3(256), 0, s, lik, n, C, (unsigned)inner, g.cpb,
                                   g.PL, ws);
            hipLaunchKernelGGL(rate_channel_fold_kernel, dim3((unsigned)rdo::ceil_div(C, 16)), dim3(256), 0, s, ws, g.S, C, out);
            return rdo::check_launch("neg_log2_channel_sums");
        },
        stream, "entropy", 0.0, 4.0 * outer * C * inner);
}

}  // extern "C"
