// The block-scaled GEMM, convolution and transposed convolution with a packed MX output (include/rdo_ptq_mxchain.h): the kernels of
// mx_gemm.hip, mx_conv.hip and mx_tconv.hip with another epilogue.  Tiling, lane mapping and the K loop are theirs -- the same
// mx_gemm_accumulate / mxconv::accumulate / mxtconv::accumulate, hence the same accumulators --; where they store 32 x 32 fp32 values,
// these run mx_pack_store (mx_pack_store_device.h): bias, activation, one MX block per output row of the wave (n0 % 32 == 0 and
// N % 32 == 0: the wave's 32 channels are one block of the next layer's K), packed through a wave-private LDS tile, stored as the dwords
// and the scale byte rdo_mx_quant_pack would have written from the fp32 result.  Built with -ffp-contract=off like the three.
// The input formats are template immediates of the instruction (25 pairs a kernel); the output format is an MxFormat passed by value and
// the activation an int, as in mx_quant_pack_kernel: no instantiation per output format.
// The kernels keep the per-wave early return of their fp32 twins and have no workgroup barrier: the exchange is inside the wave.
#include "rdo_common.h"
#include "mx_conv_device.h"
#include "mx_tconv_device.h"
#include "mx_pack_store_device.h"

namespace {

template <int FA, int FB>
__global__ __launch_bounds__(256) void mx_gemm_packed_kernel(const uint32_t* __restrict__ a, const uint8_t* __restrict__ sa,
                                                             const uint32_t* __restrict__ b, const uint8_t* __restrict__ sb, int M, int N,
                                                             long nb, int tiles_n, const float* __restrict__ bias, MxPackedOut out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const long m0 = tm * 64 + (wave >> 1) * 32, n0 = tn * 64 + (wave & 1) * 32;
    if (m0 >= M || n0 >= N) return;                                             // uniform over the wave; the kernel has no barrier
    f32x4 acc[2][2];
    mx_gemm_accumulate<FA, FB>(a, sa, b, sb, M, N, nb, m0, n0, lane & 15, lane >> 4, acc);
    mx_pack_store(acc, bias, out, n0, N, [=](int t) { return m0 + t < M ? m0 + t : -1L; });
}

template <int FX, int FW>
__global__ __launch_bounds__(256) void mx_conv_packed_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ sx,
                                                             const uint32_t* __restrict__ w, const uint8_t* __restrict__ sw, int H, int W, int cb,
                                                             int k, int stride, int pad, int Ho, int Wo, int M, int N, long nb, int tiles_n,
                                                             const float* __restrict__ bias, MxPackedOut out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const long m0 = tm * 64 + (wave >> 1) * 32, n0 = tn * 64 + (wave & 1) * 32;
    if (m0 >= M || n0 >= N) return;                                             // uniform over the wave; the kernel has no barrier
    f32x4 acc[2][2];
    mxconv::accumulate<FX, FW>(x, sx, w, sw, H, W, cb, k, stride, pad, Ho, Wo, M, N, nb, m0, n0, lane & 15, lane >> 4, acc);
    mx_pack_store(acc, bias, out, n0, N, [=](int t) { return m0 + t < M ? m0 + t : -1L; });      // NHWC: row m is output pixel m
}

template <int FX, int FW>
__global__ __launch_bounds__(256) void mx_tconv_packed_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ sx,
                                                              const uint32_t* __restrict__ w, const uint8_t* __restrict__ sw, int B, int H, int W,
                                                              int cb, int k, int s, int pad, int Ho, int Wo, int N, int tiles_m, int tiles_n,
                                                              const float* __restrict__ bias, MxPackedOut out) {
    const int lane = threadIdx.x & 63;
    mxtconv::PhaseTile t;
    if (!mxtconv::phase_tile(B, k, s, pad, Ho, Wo, N, tiles_m, tiles_n, t)) return;     // uniform over the wave; the kernel has no barrier
    f32x4 acc[2][2];
    mxtconv::accumulate<FX, FW>(x, sx, w, sw, H, W, cb, pad, N, t, lane & 15, lane >> 4, acc);      // a phase without taps: zeros -> act(bias)
    mx_pack_store(acc, bias, out, t.n0, N, [&](int row) { return mxtconv::out_pixel(t, t.m0 + row, Ho, Wo); });
}

using GemmPackedKernel = void (*)(const uint32_t*, const uint8_t*, const uint32_t*, const uint8_t*, int, int, long, int, const float*, MxPackedOut);
using ConvPackedKernel = void (*)(const uint32_t*, const uint8_t*, const uint32_t*, const uint8_t*, int, int, int, int, int, int, int, int, int, int,
                                  long, int, const float*, MxPackedOut);
using TconvPackedKernel = void (*)(const uint32_t*, const uint8_t*, const uint32_t*, const uint8_t*, int, int, int, int, int, int, int, int, int,
                                   int, int, int, const float*, MxPackedOut);

#define RDO_MXP_ROW(kernel, F) {kernel<F, 0>, kernel<F, 1>, kernel<F, 2>, kernel<F, 3>, kernel<F, 4>}
#define RDO_MXP_TABLE(kernel) {RDO_MXP_ROW(kernel, 0), RDO_MXP_ROW(kernel, 1), RDO_MXP_ROW(kernel, 2), RDO_MXP_ROW(kernel, 3), RDO_MXP_ROW(kernel, 4)}
const GemmPackedKernel kGemmPacked[5][5] = RDO_MXP_TABLE(mx_gemm_packed_kernel);
const ConvPackedKernel kConvPacked[5][5] = RDO_MXP_TABLE(mx_conv_packed_kernel);
const TconvPackedKernel kTconvPacked[5][5] = RDO_MXP_TABLE(mx_tconv_packed_kernel);
#undef RDO_MXP_TABLE
#undef RDO_MXP_ROW

// bytes of a packed [rows][N] output with its scale bytes
inline double packed_out_bytes(double rows, double N, const MxFormat& f) { return rows * N / kBlock * (4.0 * f.bits + 1.0); }

}  // namespace

extern "C" {

int rdo_mx_gemm_packed(const void* a, const uint8_t* a_scales, int32_t a_format, const void* b, const uint8_t* b_scales, int32_t b_format,
                       int32_t M, int32_t N, int64_t K, const float* bias, int32_t out_format, int32_t act, void* y_packed, uint8_t* y_scales,
                       void* stream) {
    const char* who = "rdo_mx_gemm_packed";
    GemmPlan p;
    MxPackedOut out;
    if (const int rc = mx_gemm_check(who, a, a_scales, a_format, b, b_scales, b_format, M, N, K, bias, p)) return rc;
    if (const int rc = mx_packed_out_check(who, out_format, act, N, y_packed, y_scales, out)) return rc;
    const GemmPackedKernel kern = kGemmPacked[hw_format(a_format)][hw_format(b_format)];
    const uint32_t* pa = static_cast<const uint32_t*>(a);
    const uint32_t* pb = static_cast<const uint32_t*>(b);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), 0, s, pa, a_scales, pb, b_scales, M, N, p.nb, p.tiles_n, bias, out);
            return rdo::check_launch("mx_gemm_packed");
        },
        stream, "mx_gemm_packed", 2.0 * (double)M * (double)N * (double)K,
        (double)p.total_a * (4.0 * p.bits_a + 1.0) + (double)p.total_b * (4.0 * p.bits_b + 1.0) + packed_out_bytes(M, N, out.f));
}

int rdo_mx_conv2d_packed(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales, int32_t w_format,
                         int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad, const float* bias,
                         int32_t out_format, int32_t act, void* y_packed, uint8_t* y_scales, void* stream) {
    const char* who = "rdo_mx_conv2d_packed";
    mxconv::ConvPlan c;
    MxPackedOut out;
    if (const int rc = mxconv::check(who, x, x_scales, x_format, w, w_scales, w_format, B, H, W, C, N, k, stride, pad, bias, c)) return rc;
    if (const int rc = mx_packed_out_check(who, out_format, act, N, y_packed, y_scales, out)) return rc;
    const ConvPackedKernel kern = kConvPacked[hw_format(x_format)][hw_format(w_format)];
    const uint32_t* px = static_cast<const uint32_t*>(x);
    const uint32_t* pw = static_cast<const uint32_t*>(w);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(c.grid), dim3(256), 0, s, px, x_scales, pw, w_scales, H, W, c.cb, k, stride, pad, c.Ho, c.Wo, c.M, N,
                               c.nb, c.tiles_n, bias, out);
            return rdo::check_launch("mx_conv2d_packed");
        },
        stream, "mx_conv2d_packed", 2.0 * (double)c.M * (double)N * (double)c.nb * kBlock,
        (double)c.total_x * (4.0 * c.bits_x + 1.0) + (double)c.total_w * (4.0 * c.bits_w + 1.0) + packed_out_bytes(c.M, N, out.f));
}

int rdo_mx_conv_transpose2d_packed(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales,
                                   int32_t w_format, int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride,
                                   int32_t pad, int32_t output_padding, const float* bias, int32_t out_format, int32_t act, void* y_packed,
                                   uint8_t* y_scales, void* stream) {
    const char* who = "rdo_mx_conv_transpose2d_packed";
    mxtconv::TconvPlan c;
    MxPackedOut out;
    if (const int rc = mxtconv::check(who, x, x_scales, x_format, w, w_scales, w_format, B, H, W, C, N, k, stride, pad, output_padding, bias, c))
        return rc;
    if (const int rc = mx_packed_out_check(who, out_format, act, N, y_packed, y_scales, out)) return rc;
    const TconvPackedKernel kern = kTconvPacked[hw_format(x_format)][hw_format(w_format)];
    const uint32_t* px = static_cast<const uint32_t*>(x);
    const uint32_t* pw = static_cast<const uint32_t*>(w);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(c.grid), dim3(256), 0, s, px, x_scales, pw, w_scales, B, H, W, c.cb, k, stride, pad, c.Ho, c.Wo, N,
                               c.tiles_m, c.tiles_n, bias, out);
            return rdo::check_launch("mx_conv_transpose2d_packed");
        },
        stream, "mx_conv_transpose2d_packed", 2.0 * (double)c.in * (double)N * (double)c.nbw * kBlock,
        (double)c.total_x * (4.0 * c.bits_x + 1.0) + (double)c.total_w * (4.0 * c.bits_w + 1.0) + packed_out_bytes((double)c.out, N, out.f));
}

}  // extern "C"
