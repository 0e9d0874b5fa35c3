// k x k convolutions on the block-scaled matrix instruction from packed MX operands (include/rdo_ptq_mxconv.h): an implicit GEMM with
// the tiling, lane mapping and K step of mx_gemm_kernel -- one wave owns 32 x 32 outputs, a workgroup of four waves 64 x 64, lane l =
// (row l & 15, k group l >> 4), a K step covers four blocks -- over M = B Ho Wo output pixels, N output channels and nb = k k C / 32
// blocks per row.  Built with -ffp-contract=off like mx_gemm.hip.  The fragments, the FP8 one-of-eight passes, the K step and the store
// are mx_mfma_device.h's, the B side (the weight rows) is the GEMM's load_fragment; the one difference is the A side: block kb of the
// im2col row of output pixel (b, oy, ox) is channel block kb % cb of tap kb / cb (cb = C / 32), that is block
// ((b H + oy stride - pad + kh) W + ox stride - pad + kw) cb + kb % cb of x with its scale byte, or, for a tap outside the image (and
// for a row past M or a block past nb), zero registers under the scale 127 -- what the GEMM reads from the im2col matrix, block for
// block, in the same K order: equal bits.  A tap is placed by its own (iy, ix) test, so it never reads across a row or an image of the
// batch.
// The pixel of a lane's rows is decomposed once, before the K loop; the (channel block, kh, kw) of the blocks a lane owns advance by
// four blocks a step with adds and compares (TapWalk): the loop holds no division.  The two FP8 half blocks of a lane (blocks kg / 2
// and 2 + kg / 2 of the step) are walked and placed each on its own, next to block kg, whose scale the lane holds.
// The walk, the K loop and the argument checks are mx_conv_device.h's, shared with the packed-output kernel of mx_chain.hip.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxconv.h"
#include "mx_conv_device.h"

namespace {

using namespace mxconv;

template <int FX, int FW>
__global__ __launch_bounds__(256) void mx_conv_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ sx,
                                                      const uint32_t* __restrict__ w, const uint8_t* __restrict__ sw, int H, int W, int cb,
                                                      int k, int stride, int pad, int Ho, int Wo, int M, int N, long nb, int tiles_n,
                                                      const float* __restrict__ bias, float* __restrict__ y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kg = lane >> 4;
    const long tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const long m0 = tm * 64 + (wave >> 1) * 32, n0 = tn * 64 + (wave & 1) * 32;
    if (m0 >= M || n0 >= N) return;                                             // uniform over the wave; the kernel has no barrier
    f32x4 acc[2][2];
    accumulate<FX, FW>(x, sx, w, sw, H, W, cb, k, stride, pad, Ho, Wo, M, N, nb, m0, n0, r, kg, acc);
    mx_store_tiles(acc, bias, y, m0, n0, M, N, r, kg);
}

using ConvKernel = void (*)(const uint32_t*, const uint8_t*, const uint32_t*, const uint8_t*, int, int, int, int, int, int, int, int, int, int,
                            long, int, const float*, float*);

#define RDO_MXC_ROW(FX) {mx_conv_kernel<FX, 0>, mx_conv_kernel<FX, 1>, mx_conv_kernel<FX, 2>, mx_conv_kernel<FX, 3>, mx_conv_kernel<FX, 4>}
const ConvKernel kConv[5][5] = {RDO_MXC_ROW(0), RDO_MXC_ROW(1), RDO_MXC_ROW(2), RDO_MXC_ROW(3), RDO_MXC_ROW(4)};
#undef RDO_MXC_ROW

}  // namespace

extern "C" {

int64_t rdo_mx_conv2d_out_pixels(int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad) {
    ConvPixels p;
    return conv_pixels(B, H, W, k, stride, pad, p) ? p.out : 0;
}

int rdo_mx_conv2d(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales, int32_t w_format,
                  int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad, const float* bias, float* y,
                  void* stream) {
    RDO_REQUIRE(y, "rdo_mx_conv2d: null pointer");
    RDO_REQUIRE(aligned4(y), "rdo_mx_conv2d: x, w, bias and y must be 4-byte aligned");
    ConvPlan c;
    if (const int rc = check("rdo_mx_conv2d", x, x_scales, x_format, w, w_scales, w_format, B, H, W, C, N, k, stride, pad, bias, c)) return rc;
    const ConvKernel kern = kConv[hw_format(x_format)][hw_format(w_format)];
    const uint32_t* px = static_cast<const uint32_t*>(x);
    const uint32_t* pw = static_cast<const uint32_t*>(w);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(c.grid), dim3(256), 0, s, px, x_scales, pw, w_scales, H, W, c.cb, k, stride, pad, c.Ho, c.Wo, c.M, N,
                               c.nb, c.tiles_n, bias, y);
            return rdo::check_launch("mx_conv2d");
        },
        stream, "mx_conv2d", 2.0 * (double)c.M * (double)N * (double)c.nb * kBlock,
        (double)c.total_x * (4.0 * c.bits_x + 1.0) + (double)c.total_w * (4.0 * c.bits_w + 1.0) + (double)c.M * (double)N * 4.0);
}

}  // extern "C"
