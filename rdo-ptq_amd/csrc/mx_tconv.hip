// Transposed k x k convolutions on the block-scaled matrix instruction from packed MX operands (include/rdo_ptq_mxtconv.h): the implicit
// GEMM of mx_conv.hip -- the tiling, lane mapping and K step of mx_gemm_kernel, one wave 32 x 32 outputs, a workgroup of four waves
// 64 x 64, lane l = (row l & 15, k group l >> 4), a K step covers four blocks -- run once per PHASE of the output, all in one launch.
// Built with -ffp-contract=off like mx_conv.hip.  The output pixels of phase (ry, rx) = ((oy + pad) % s, (ox + pad) % s) are
// oy = oy0 + jy s, ox = ox0 + jx s and all use the taps kh = ry + a s < k, kw = rx + e s < k (a < ty, e < tx), whose input pixel is
// (qy0 + jy - a, qx0 + jx - e) with qy0 = (oy0 + pad - ry) / s: a stride-1 correlation with the taps walked backwards over the input.
// The gathered row of such a pixel lists the taps in ascending (a, e) order, cb = C / 32 blocks each, nb_p = ty tx cb blocks; block q of
// it is channel block q % cb of tap q / cb on both sides: block ((b H + iy) W + ix) cb + c of x (zero registers under the scale 127
// where the pixel lies outside the image, for a row past the phase's pixels and for a block past nb_p) and block
// ((kh k + kw) cb + c) of weight row n.  That is what rdo_mx_gemm reads from the gathered matrices of the phase, block for block, in the
// same K order: equal bits.  A phase without taps (k < s, or rows that output_padding adds) runs no K step and stores the bias.
// The grid is s s x tiles_m x tiles_n with tiles_m sized for the largest phase: the phase and the tile are decoded from the block index
// and a tile past its phase's pixels returns at once.  Both sides walk (channel block, e, a) with adds and compares (TapWalk), the FP8
// half blocks each on their own as in mx_conv.hip; the K loop holds no division.  The store maps a tile row back to its output pixel.
// The phase, the walk, the K loop and the argument checks are mx_tconv_device.h's, shared with the packed-output kernel of mx_chain.hip.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxtconv.h"
#include "mx_tconv_device.h"

namespace {

using namespace mxtconv;

template <int FX, int FW>
__global__ __launch_bounds__(256) void mx_tconv_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ sx,
                                                       const uint32_t* __restrict__ w, const uint8_t* __restrict__ sw, int B, int H, int W,
                                                       int cb, int k, int s, int pad, int Ho, int Wo, int N, int tiles_m, int tiles_n,
                                                       const float* __restrict__ bias, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kg = lane >> 4;
    PhaseTile t;
    if (!phase_tile(B, k, s, pad, Ho, Wo, N, tiles_m, tiles_n, t)) return;      // uniform over the wave; the kernel has no barrier
    f32x4 acc[2][2];
    accumulate<FX, FW>(x, sx, w, sw, H, W, cb, pad, N, t, r, kg, acc);
    // the wave's 32 x 32 outputs, bias added, each tile row at its output pixel.  C/D: col = lane & 15 (r), row = 4 (lane >> 4) + reg.
    long at[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) at[i][q] = out_pixel(t, t.m0 + 16 * i + 4 * kg + q, Ho, Wo);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long col = t.n0 + 16 * j + r;
        if (col >= N) continue;
        const float bj = bias ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (at[i][q] >= 0) y[at[i][q] * N + col] = acc[i][j][q] + bj;
    }
}

using TconvKernel = void (*)(const uint32_t*, const uint8_t*, const uint32_t*, const uint8_t*, int, int, int, int, int, int, int, int, int, int,
                             int, int, const float*, float*);

#define RDO_MXT_ROW(FX) {mx_tconv_kernel<FX, 0>, mx_tconv_kernel<FX, 1>, mx_tconv_kernel<FX, 2>, mx_tconv_kernel<FX, 3>, mx_tconv_kernel<FX, 4>}
const TconvKernel kTconv[5][5] = {RDO_MXT_ROW(0), RDO_MXT_ROW(1), RDO_MXT_ROW(2), RDO_MXT_ROW(3), RDO_MXT_ROW(4)};
#undef RDO_MXT_ROW

}  // namespace

extern "C" {

int64_t rdo_mx_conv_transpose2d_out_pixels(int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad, int32_t output_padding) {
    TconvPixels p;
    return tconv_pixels(B, H, W, k, stride, pad, output_padding, p) ? p.out : 0;
}

int rdo_mx_conv_transpose2d(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales, int32_t w_format,
                            int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad,
                            int32_t output_padding, const float* bias, float* y, void* stream) {
    RDO_REQUIRE(y, "rdo_mx_conv_transpose2d: null pointer");
    RDO_REQUIRE(aligned4(y), "rdo_mx_conv_transpose2d: x, w, bias and y must be 4-byte aligned");
    TconvPlan c;
    if (const int rc = check("rdo_mx_conv_transpose2d", x, x_scales, x_format, w, w_scales, w_format, B, H, W, C, N, k, stride, pad, output_padding,
                             bias, c))
        return rc;
    const TconvKernel kern = kTconv[hw_format(x_format)][hw_format(w_format)];
    const uint32_t* px = static_cast<const uint32_t*>(x);
    const uint32_t* pw = static_cast<const uint32_t*>(w);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(c.grid), dim3(256), 0, s, px, x_scales, pw, w_scales, B, H, W, c.cb, k, stride, pad, c.Ho, c.Wo, N,
                               c.tiles_m, c.tiles_n, bias, y);
            return rdo::check_launch("mx_conv_transpose2d");
        },
        stream, "mx_conv_transpose2d", 2.0 * (double)c.in * (double)N * (double)c.nbw * kBlock,
        (double)c.total_x * (4.0 * c.bits_x + 1.0) + (double)c.total_w * (4.0 * c.bits_w + 1.0) + (double)c.out * (double)N * 4.0);
}

}  // extern "C"
