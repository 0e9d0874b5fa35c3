// The row body of residual add + LayerNorm, stated once for swin.hip (add_ln_kernel) and mx_swin.hip (the LayerNorm producer of the MX
// Swin kernels): s = a (+ b), two-pass mean / variance, y = (s - mean) * rstd * w + bias.
// Layout: 16 lanes per row, VPL float4 per lane (C / 4 <= 16 * VPL), lane l16 holds float4 l16 + 16 k, k = 0 .. VPL - 1: every load
// instruction of a 16-lane group is 256 contiguous bytes; the two row statistics are four-step butterflies inside the group.
// The arithmetic is stated operation by operation (no contraction but the two written fmaf): the bits do not depend on the flags of
// the file that includes it or on what the compiler makes of the surrounding kernel, and they are rdo_add_layer_norm's.
#pragma once

typedef float ln4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float ln_sum4(ln4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float ln_red16(float v) {
    v += __shfl_xor(v, 8, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 1, 16);
    return v;
}

// the lane's VPL float4 of weight and bias (ones / zeros where the pointer is null or the float4 lies past C4)
template <int VPL>
__device__ __forceinline__ void ln_row_params(const ln4* __restrict__ w, const ln4* __restrict__ bias, int C4, int l16, ln4 (&wv)[VPL],
                                              ln4 (&bv)[VPL]) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
        const int c = l16 + 16 * k;
        wv[k] = (w && c < C4) ? w[c] : ln4{1.f, 1.f, 1.f, 1.f};
        bv[k] = (bias && c < C4) ? bias[c] : ln4{0.f, 0.f, 0.f, 0.f};
    }
}

// One row (its float4 start at `base`) by its 16 lanes: s -> s_out (if not null), LN(s) -> emit(k, float4) for the lane's float4
// below C4; wb(k, w, bias) gives the lane's k-th float4 of weight and bias (ln_row_params' registers, or a load where registers are
// short).  All 16 lanes of the row call it together.
template <int VPL, class Params, class Emit>
__device__ __forceinline__ void ln_row(const ln4* __restrict__ a, const ln4* __restrict__ b, long base, int C4, int l16, float invC, float eps,
                                       ln4* __restrict__ s_out, Params wb, Emit emit) {
#pragma clang fp contract(off)
    ln4 v[VPL];
    float s1 = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
        const int c = l16 + 16 * k;
        if (c < C4) {
            v[k] = a[base + c];
            if (b) v[k] += b[base + c];
            if (s_out) s_out[base + c] = v[k];
            s1 += ln_sum4(v[k]);
        } else {
            v[k] = ln4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float mean = ln_red16(s1) * invC;
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
        if (l16 + 16 * k < C4) {
            v[k] -= mean;
            const ln4 q = v[k] * v[k];
            s2 += ln_sum4(q);
        }
    }
    const float rstd = rsqrtf(__builtin_fmaf(ln_red16(s2), invC, eps));
#pragma unroll
    for (int k = 0; k < VPL; ++k)
        if (l16 + 16 * k < C4) {
            ln4 w, bias;
            wb(k, w, bias);
            emit(k, __builtin_elementwise_fma(v[k] * rstd, w, bias));
        }
}
