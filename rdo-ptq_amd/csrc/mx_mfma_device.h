// What mx_gemm.hip (the GEMM) and mx_conv.hip (the implicit-GEMM convolution) share of the block-scaled matrix instruction
// v_mfma_scale_f32_16x16x128_f8f6f4 on packed MX operands (include/rdo_ptq_mxgemm.h states the operand format and what a lane holds):
// the instruction's format numbers, a lane's operand registers from the packed blocks it owns in a K step, the FP8 one-of-eight mask,
// the K step itself and the store of a wave's 32 x 32 outputs.  Both kernels run one K step as mx_mfma_step on fragments made by
// load_blocks, in ascending K order: equal fragments and scales give equal bits, which is what makes the convolution the GEMM on the
// im2col matrix bit for bit.  Included once per translation unit, hence the unnamed namespace.
#pragma once
#include "mx_device.h"

namespace {

using i32x8 = __attribute__((ext_vector_type(8))) int;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// the instruction's format numbers {0 E4M3, 1 E5M2, 2 E2M3, 3 E3M2, 4 FP4} and the operand dwords of each
constexpr int hw_dwords(int hw) { return hw <= 1 ? 8 : (hw <= 3 ? 6 : 4); }

inline int hw_format(int format) {
    switch (format) {
        case RDO_MX_FP4: return 4;
        case RDO_MX_FP6_E2M3: return 2;
        case RDO_MX_FP6_E3M2: return 3;
        case RDO_MX_FP8_E4M3: return 0;
        case RDO_MX_FP8_E5M2: return 1;
    }
    return -1;
}

// The operand registers of lane (row, k group kg) for one K step from the packed blocks the lane owns in it.  FP4 / FP6 (4 / 6 dwords):
// the lane owns one block, block kg of the step, at `p0`; its dwords are the registers (p1 is not read).  FP8 (8 dwords): registers
// 0 .. 3 are elements 16 kg .. 16 kg + 15 of the step and registers 4 .. 7 elements 64 + 16 kg .. 64 + 16 kg + 15 -- the second (kg odd)
// or first half of block kg / 2 of the step, at `p0`, and the same half of block 2 + kg / 2, at `p1`.  A block that is not ok (a row
// past the matrix, a block past K / 32, a tap in the zero padding) is zero registers and its pointer is not read.
template <int DW>
__device__ __forceinline__ i32x8 load_blocks(const uint32_t* __restrict__ p0, bool ok0, const uint32_t* __restrict__ p1, bool ok1, int kg) {
    i32x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (DW == 8) {
        const int off = (kg & 1) * 4;
        if (ok0) {
#pragma unroll
            for (int d = 0; d < 4; ++d) v[d] = (int)p0[off + d];
        }
        if (ok1) {
#pragma unroll
            for (int d = 0; d < 4; ++d) v[4 + d] = (int)p1[off + d];
        }
    } else {
        if (ok0) {
#pragma unroll
            for (int d = 0; d < DW; ++d) v[d] = (int)p0[d];
        }
    }
    return v;
}

// load_blocks for a matrix row: the K step starts at block k0 of the row whose packed blocks start at `row`; the lane owns block
// k0 + kg (FP4 / FP6) or the halves of blocks k0 + kg / 2 and k0 + 2 + kg / 2 (FP8); the scale of lane kg is block k0 + kg's for every
// width.
template <int DW>
__device__ __forceinline__ i32x8 load_fragment(const uint32_t* __restrict__ row, long k0, int kg, long nb, bool row_ok) {
    if constexpr (DW == 8) {
        const long b0 = k0 + (kg >> 1), b1 = b0 + 2;
        return load_blocks<8>(row + b0 * 8, row_ok && b0 < nb, row + b1 * 8, row_ok && b1 < nb, kg);
    } else {
        const long kb = k0 + kg;
        return load_blocks<DW>(row + kb * DW, row_ok && kb < nb, row, false, kg);
    }
}

// An FP8 fragment with all but element t of every eight neighbouring elements cleared (t = 0 .. 7): the eight lie in a pair of VGPRs
// (2 p, 2 p + 1), element t in byte t & 3 of the VGPR of parity t >> 2.
__device__ __forceinline__ i32x8 keep_one_of_eight(const i32x8& v, int t) {
    const int m = (int)(0xFFu << (8 * (t & 3)));
    i32x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 4; ++p) o[2 * p + (t >> 2)] = v[2 * p + (t >> 2)] & m;
    return o;
}

// One K step of 128 of a wave's 2 x 2 tiles of 16 x 16: fa[i] / fb[j] the lane's operand registers for A tile i / B tile j, xa / xb
// their scale bytes.  FA / FB are the instruction's format numbers.
template <int FA, int FB>
__device__ __forceinline__ void mx_mfma_step(const i32x8 (&fa)[2], const i32x8 (&fb)[2], const int (&xa)[2], const int (&xb)[2],
                                             f32x4 (&acc)[2][2]) {
    constexpr int DA = hw_dwords(FA), DB = hw_dwords(FB);
    if constexpr (DA == 8 || DB == 8) {
        // With an FP8 operand the instruction adds the products of eight neighbouring k aligned to the largest of the eight and
        // drops what lies some 14 bits below it.  Eight passes, each with one element of every eight of ONE FP8 operand kept and
        // the rest cleared, leave a single product in every such sum: nothing is dropped, the sums between the groups are fp32's.
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            i32x8 ma[2], mb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ma[i] = DA == 8 ? keep_one_of_eight(fa[i], t) : fa[i];
                mb[i] = DA == 8 ? fb[i] : keep_one_of_eight(fb[i], t);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ma[i], mb[j], acc[i][j], FA, FB, 0, xa[i], 0, xb[j]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i], fb[j], acc[i][j], FA, FB, 0, xa[i], 0, xb[j]);
    }
}

// The wave's 32 x 32 outputs at (m0, n0) of y [M][N], bias added.  C/D: col = lane & 15 (r), row = 4 (lane >> 4) + reg.
__device__ __forceinline__ void mx_store_tiles(const f32x4 (&acc)[2][2], const float* __restrict__ bias, float* __restrict__ y, long m0,
                                               long n0, int M, int N, int r, int kg) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long col = n0 + 16 * j + r;
        if (col >= N) continue;
        const float bj = bias ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long row = m0 + 16 * i + 4 * kg + q;
                if (row < M) y[row * N + col] = acc[i][j][q] + bj;
            }
    }
}

inline bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace
