// Device functions of the uniform affine quantiser that more than one file evaluates (adaround.hip: rdo_uaq_fakequant and
// rdo_uaq_init_minmax; bit_alloc.hip: rdo_uaq_width_scan; weight_pack.hip: rdo_weight_pack and rdo_weight_unpack): ONE statement of each
// expression, so that the files cannot drift apart by a rounding.  All of them are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace rdo {

// the level (an integer-valued float in [0, Lm1]) of round-to-nearest on the grid (dl, z) of Lm1 + 1 levels
__device__ __forceinline__ float uaq_level_nearest(float wv, float dl, float z, float Lm1) {
    const float xint = rintf(wv / dl) + z;
    return fminf(fmaxf(xint, 0.f), Lm1);
}

// the level of the hard AdaRound rounding: down, plus one where the rounding logit av is >= 0 (the hard branch of ada_fwd_kernel)
__device__ __forceinline__ float uaq_level_hard(float wv, float av, float dl, float z, float Lm1) {
    const float xint = floorf(wv / dl) + (av >= 0.f ? 1.f : 0.f) + z;
    return fminf(fmaxf(xint, 0.f), Lm1);
}

// the value of a level: the tail expression of both fake-quantisation kernels
__device__ __forceinline__ float uaq_dequant(float level, float dl, float z) { return (level - z) * dl; }

// round-to-nearest fake quantisation of one value on the grid (dl, z) of Lm1 + 1 levels (quantizer.py:372-376 of the reference)
__device__ __forceinline__ float uaq_nearest(float wv, float dl, float z, float Lm1) {
    return uaq_dequant(uaq_level_nearest(wv, dl, z, Lm1), dl, z);
}

// the 'max' grid of a row whose min and max (clamped through 0) are mn, mx ('max' init, quantizer.py:281-298: python-double arithmetic
// for the range, rounded once; fp32 for the zero point)
__device__ __forceinline__ void uaq_minmax_grid(float mn, float mx, int n_levels, float& dl, float& zp) {
    const float d = fmaxf((float)(((double)mx - (double)mn) / (double)(n_levels - 1)), 1e-8f);
    dl = d;
    // the reference writes (-x_min / delta) with a Python float on the left: torch evaluates that as delta.reciprocal() * (-x_min)
    // in fp32 (Tensor.__rdiv__), one rounding more than a division -- it decides the ties at x.5 (symmetric weight ranges)
    zp = rintf(__fmul_rn(__frcp_rn(d), -mn));
}

// min and max over a 256-thread workgroup: the 64-lane __shfl_down steps 32 .. 1, the four wave values through LDS.  Valid on thread 0
// only; every thread of the workgroup makes the call (it holds a barrier), a second call needs a barrier of its own in between.
__device__ __forceinline__ void uaq_block_minmax(float& mn, float& mx) {
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_down(mn, o, 64));
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
    }
    __shared__ float smn[4], smx[4];
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
        mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    }
}

}  // namespace rdo
