// What the MX Swin kernels share (mx_swin.hip: the LayerNorm producer and the MLP half; mx_swin_attn.hip: the attention half): the row
// phase that turns LN(a + b) into packed MX blocks without leaving the registers, the K loop of a 32 x 32 unit whose A rows lie in an
// LDS image, and the row stride of such an image.  The header comment of mx_swin.hip states the layouts.
#pragma once
#include "mx_pack_store_device.h"
#include "ln_row_device.h"

namespace {

// One row by its 16 lanes: LN(a + b) -> `ln` (if asked), its MX blocks -> dst_row (the row's packed dwords, global or LDS) and sc_row,
// block by block as ln_row hands the float4 out (weight and bias are loaded there: L1 lines, not 64 registers).  A row that is not live
// is not read; where keep_dead (the LDS image) its codes and scale bytes are zeros.  `live` is uniform over the row's 16 lanes.
template <int VPL>
__device__ __forceinline__ void ln_pack_row(const ln4* __restrict__ a, const ln4* __restrict__ b, const ln4* w, const ln4* bias, int C4, int l16,
                                            float invC, float eps, long row, bool live, bool keep_dead, ln4* __restrict__ sum_out, ln4* ln,
                                            const MxFormat& f, uint32_t* dst_row, uint8_t* sc_row) {
    if (live) {
        ln_row<VPL>(
            a, b, row * C4, C4, l16, invC, eps, sum_out,
            [&](int k, ln4& wk, ln4& bk) {
                wk = w ? w[l16 + 16 * k] : ln4{1.f, 1.f, 1.f, 1.f};
                bk = bias ? bias[l16 + 16 * k] : ln4{0.f, 0.f, 0.f, 0.f};
            },
            [&](int k, ln4 y) {                                                 // the eight lanes of block kb together: C4 % 8 == 0
                const int c = l16 + 16 * k, kb = c >> 3;
                if (ln) ln[row * C4 + c] = y;
                const float v[4] = {y.x, y.y, y.z, y.w};
                const unsigned sc = mx_quad_quant_store(v, f, dst_row + kb * f.bits, true);
                if ((l16 & 7) == 0) sc_row[kb] = (uint8_t)sc;
            });
    } else if (keep_dead) {
        const int s = l16 & 7;
        for (int c = l16; c < C4; c += 16) {
            if (s < f.bits) dst_row[(c >> 3) * f.bits + s] = 0u;
            if (s == 0) sc_row[c >> 3] = 0;
        }
    }
}

// mx_gemm_accumulate's loop for the wave's 32 x 32 outputs at (m0, n0) with the A rows in an LDS image (all 64 rows exist: no row test).
// A B row past `nlast` reads row nlast instead: its column's accumulators are the caller's to drop (a unit that overhangs the matrix);
// likewise an A row past `mlast` (an image of fewer rows than its units cover: mx_resunit.hip's 100-row halo).
template <int FA, int FB>
__device__ __forceinline__ void unit_accumulate(const uint32_t* image, int stride, const uint8_t* scales, int nb, const uint32_t* __restrict__ w,
                                                const uint8_t* __restrict__ sw, int m0, int n0, int r, int kg, f32x4 (&acc)[2][2],
                                                int nlast = 0x7fffffff, int mlast = 0x7fffffff) {
    constexpr int DA = hw_dwords(FA), DB = hw_dwords(FB);
    const uint32_t* arow[2];
    long brow[2];
    int srow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + 16 * i + r < mlast ? m0 + 16 * i + r : mlast;
        arow[i] = image + m * stride;
        srow[i] = m * nb;
        const int n = n0 + 16 * i + r;
        brow[i] = (long)(n < nlast ? n : nlast) * nb;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < nb; k0 += 4) {
        const int kb = k0 + kg;
        const bool kok = kb < nb;
        i32x8 fa[2], fb[2];
        int xa[2], xb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fa[i] = load_fragment<DA>(arow[i], k0, kg, nb, true);
            fb[i] = load_fragment<DB>(w + brow[i] * DB, k0, kg, nb, true);
            xa[i] = kok ? (int)scales[srow[i] + kb] : 127;
            xb[i] = kok ? (int)sw[brow[i] + kb] : 127;
        }
        mx_mfma_step<FA, FB>(fa, fb, xa, xb, acc);
    }
}

// dwords of an LDS operand row of nb blocks: a multiple of four, an odd number of 16-byte units (mx_gdn.hip's rule)
constexpr int lds_row_dwords(int nb, int bits) {
    int stride = (nb * bits + 3) & ~3;
    if (((stride >> 2) & 1) == 0) stride += 4;
    return stride;
}

}  // namespace
