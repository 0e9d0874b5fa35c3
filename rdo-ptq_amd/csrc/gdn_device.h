// Device functions shared by the GDN / IGDN kernels: the element-wise formulas of the unit tail (fused_tail.hip), the per-token
// power-of-two scale and fp16 split of the token-matrix Linear (linear_h2.hip), and the loss hand-over of the tail launches.
// gdn_fused.hip runs all of them in one launch: one implementation, so the fused launch and the chain of separate launches produce
// the same bits.  The element-wise formulas need -ffp-contract=off (their callers are built with it); the token split rounds the
// same with and without: every product it feeds into an add or subtract is a product with a power of two, i.e. exact.
#pragma once
#include "rdo_common.h"

namespace rdo {
namespace gdn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float pow2f(int e) { return __builtin_bit_cast(float, (unsigned)(e + 127) << 23); }

__device__ __forceinline__ float amax_quad(const f32x4& v) { return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))); }

// ---- per-token scale of rdo_linear_h2: 2^(7 - floor(log2 amax)), the token's largest value lands in [2^7, 2^8).  Zero / denormal /
// non-finite rows: scale 1 (zeros stay zeros; inf / NaN propagate through fp16 as they would through fp32).  inv = 1 / sc, exact.
__device__ __forceinline__ void token_scale(float amax, float& sc, float& inv) {
    const int e = (int)((__builtin_bit_cast(unsigned, amax) >> 23) & 0xFF) - 127;
    const bool plain = e < -100 || e > 100;
    sc = plain ? 1.f : pow2f(7 - e);
    inv = plain ? 1.f : pow2f(e - 7);
}

// four scaled values -> the two fp16 planes (8 bytes each) at `dst` and `dst + plane`
__device__ __forceinline__ void split_quad_store(const f32x4& v, float sc, char* dst, int plane) {
    const f32x4 xs = v * sc;
    const f16x4 hi = __builtin_convertvector(xs, f16x4);
    const f16x4 lo = __builtin_convertvector(xs - __builtin_convertvector(hi, f32x4), f16x4);
    *reinterpret_cast<f16x4*>(dst) = hi;
    *reinterpret_cast<f16x4*>(dst + plane) = lo;
}

// ---- loss hand-over of the tail launches: every workgroup ends with one float atomic into one of the 32 log slots
// (pub: rdo_iter_bind_publish -- the launch's first thread leaves the iteration number there for the AdaRound step of the same iteration)
__device__ __forceinline__ void block_loss_add(float acc, float scale, float* loss_out, int it, int32_t* pub) {
    if (pub && blockIdx.x == 0 && threadIdx.x == 0) *pub = it;
    acc = rdo::block_sum(acc);
    if (threadIdx.x == 0 && loss_out)
        atomicAdd(loss_out + (long)it * RDO_LOG_SLOTS + (blockIdx.x & (RDO_LOG_SLOTS - 1)), acc * scale);
}

// the same for a 512-thread workgroup (block_sum is written for four waves): wave sums through `red` [8], added in wave order
__device__ __forceinline__ void block_loss_add8(float acc, float scale, float* loss_out, int it, int32_t* pub, float* red) {
    if (pub && blockIdx.x == 0 && threadIdx.x == 0) *pub = it;
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && loss_out) {
        float v = red[0];
#pragma unroll
        for (int w = 1; w < 8; ++w) v += red[w];
        atomicAdd(loss_out + (long)it * RDO_LOG_SLOTS + (blockIdx.x & (RDO_LOG_SLOTS - 1)), v * scale);
    }
}

// ---- GDN / IGDN epilogue + loss + gradient + dL/dnorm (quant_layer.py:142-154, layer_opt.py:133,150) ---------------------------------
__device__ __forceinline__ float loss_gdn_quad(const f32x4& xv, const f32x4& nv, const f32x4& y, const f32x4* r, int inverse, float gs,
                                               f32x4& o, f32x4& g, f32x4& tv) {
    f32x4 rs;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        rs[k] = __frsqrt_rn(nv[k]);
        o[k] = xv[k] * (inverse ? __fsqrt_rn(nv[k]) : rs[k]);       // the GDN / IGDN epilogue of the norm-pool conv
    }
    if (r) o += *r;
    const f32x4 dd = o - y;
    g = dd * gs;
#pragma unroll
    for (int k = 0; k < 4; ++k)       // GDN: y = x n^-1/2 -> dy/dn = -1/2 x n^-3/2 ; IGDN: y = x n^1/2 -> dy/dn = 1/2 x n^-1/2
        tv[k] = inverse ? (0.5f * g[k] * xv[k]) * rs[k] : (-0.5f * g[k] * xv[k]) * (rs[k] * rs[k] * rs[k]);
    return (dd[0] * dd[0] + dd[1] * dd[1]) + (dd[2] * dd[2] + dd[3] * dd[3]);
}

// ---- GDN backward: dx = g n^(-+1/2) + 2 x acc, in two halves: what is known before acc = t . gamma' (p = g n^(-+1/2), q = 2 x) and
// the rest.  The fused launch keeps p and q across its second GEMM; the separate kernels call gdn_dx_quad.
__device__ __forceinline__ void gdn_dx_pre(const f32x4& gv, const f32x4& xv, const f32x4& nv, int inverse, f32x4& p, f32x4& q) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float f = inverse ? __fsqrt_rn(nv[k]) : __frsqrt_rn(nv[k]);
        p[k] = gv[k] * f;
        q[k] = 2.f * xv[k];
    }
}
__device__ __forceinline__ f32x4 gdn_dx_fin(const f32x4& p, const f32x4& q, const f32x4& av) {
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = p[k] + q[k] * av[k];
    return o;
}
__device__ __forceinline__ f32x4 gdn_dx_quad(const f32x4& gv, const f32x4& xv, const f32x4& nv, const f32x4& av, int inverse) {
    f32x4 p, q;
    gdn_dx_pre(gv, xv, nv, inverse, p, q);
    return gdn_dx_fin(p, q, av);
}

}  // namespace gdn
}  // namespace rdo
