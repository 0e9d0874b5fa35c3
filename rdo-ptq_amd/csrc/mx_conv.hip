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
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxconv.h"
#include "mx_mfma_device.h"

namespace {

// (channel block, kh, kw) of one block index of the im2col row, advanced by the four blocks of a K step
struct TapWalk {
    int c, ky, kx;
};

__device__ __forceinline__ TapWalk tap_start(int q, int cb, int k) {            // q < 6: once per lane
    const int t = q / cb;
    return TapWalk{q - t * cb, t / k, t % k};
}

__device__ __forceinline__ void tap_advance(TapWalk& w, int cb, int k) {
    w.c += 4;
    while (w.c >= cb) {                                                         // at most four times: cb >= 1
        w.c -= cb;
        if (++w.kx == k) {
            w.kx = 0;
            ++w.ky;
        }
    }
}

// what the K loop keeps of an output pixel: the input position of tap (0, 0) and the index of that (possibly virtual) input pixel
struct Pixel {
    long iy0, ix0, at0;
    bool ok;
};

// the block of x a walk points at for a pixel: its index and whether it lies in the image (q: the walk's block index in the row)
__device__ __forceinline__ bool tap_block(const Pixel& p, const TapWalk& w, long q, long nb, int H, int W, int cb, long& blk) {
    const long iy = p.iy0 + w.ky, ix = p.ix0 + w.kx;
    blk = (p.at0 + (long)w.ky * W + w.kx) * cb + w.c;
    return p.ok && q < nb && iy >= 0 && iy < H && ix >= 0 && ix < W;
}

template <int FX, int FW>
__global__ __launch_bounds__(256) void mx_conv_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ sx,
                                                      const uint32_t* __restrict__ w, const uint8_t* __restrict__ sw, int H, int W, int cb,
                                                      int k, int stride, int pad, int Ho, int Wo, int M, int N, long nb, int tiles_n,
                                                      const float* __restrict__ bias, float* __restrict__ y) {
    constexpr int DX = hw_dwords(FX), DW = hw_dwords(FW);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kg = lane >> 4;
    const long tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const long m0 = tm * 64 + (wave >> 1) * 32, n0 = tn * 64 + (wave & 1) * 32;
    if (m0 >= M || n0 >= N) return;                                             // uniform over the wave; the kernel has no barrier
    Pixel px[2];
    long brow[2];
    bool bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long m = m0 + 16 * i + r;
        px[i].ok = m < M;
        const unsigned mm = px[i].ok ? (unsigned)m : 0u;                        // M <= 2^31 - 1: 32-bit divisions, once per lane
        const unsigned b = mm / ((unsigned)Ho * (unsigned)Wo), rem = mm - b * ((unsigned)Ho * (unsigned)Wo);
        const unsigned oy = rem / (unsigned)Wo, ox = rem - oy * (unsigned)Wo;
        px[i].iy0 = (long)oy * stride - pad;
        px[i].ix0 = (long)ox * stride - pad;
        px[i].at0 = ((long)b * H + px[i].iy0) * W + px[i].ix0;
        bok[i] = n0 + 16 * i + r < N;
        brow[i] = (n0 + 16 * i + r) * nb;
    }
    // the blocks the lane owns in a step: kg (its scale; FP4 / FP6: its operand) and, FP8, the half blocks of kg / 2 and 2 + kg / 2
    TapWalk ws = tap_start(kg, cb, k), w0 = tap_start(kg >> 1, cb, k), w1 = tap_start(2 + (kg >> 1), cb, k);
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long k0 = 0; k0 < nb; k0 += 4) {
        const long kb = k0 + kg;
        const bool kok = kb < nb;
        i32x8 fa[2], fb[2];
        int xa[2], xb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            long bs;
            const bool oks = tap_block(px[i], ws, kb, nb, H, W, cb, bs);
            if constexpr (DX == 8) {
                long b0, b1;
                const bool ok0 = tap_block(px[i], w0, k0 + (kg >> 1), nb, H, W, cb, b0);
                const bool ok1 = tap_block(px[i], w1, k0 + 2 + (kg >> 1), nb, H, W, cb, b1);
                fa[i] = load_blocks<8>(x + b0 * 8, ok0, x + b1 * 8, ok1, kg);
            } else {
                fa[i] = load_blocks<DX>(x + bs * DX, oks, x, false, kg);
            }
            xa[i] = oks ? (int)sx[bs] : 127;
            fb[i] = load_fragment<DW>(w + brow[i] * DW, k0, kg, nb, bok[i]);
            xb[i] = bok[i] && kok ? (int)sw[brow[i] + kb] : 127;
        }
        mx_mfma_step<FX, FW>(fa, fb, xa, xb, acc);
        tap_advance(ws, cb, k);
        if constexpr (DX == 8) {
            tap_advance(w0, cb, k);
            tap_advance(w1, cb, k);
        }
    }
    mx_store_tiles(acc, bias, y, m0, n0, M, N, r, kg);
}

using ConvKernel = void (*)(const uint32_t*, const uint8_t*, const uint32_t*, const uint8_t*, int, int, int, int, int, int, int, int, int, int,
                            long, int, const float*, float*);

#define RDO_MXC_ROW(FX) {mx_conv_kernel<FX, 0>, mx_conv_kernel<FX, 1>, mx_conv_kernel<FX, 2>, mx_conv_kernel<FX, 3>, mx_conv_kernel<FX, 4>}
const ConvKernel kConv[5][5] = {RDO_MXC_ROW(0), RDO_MXC_ROW(1), RDO_MXC_ROW(2), RDO_MXC_ROW(3), RDO_MXC_ROW(4)};
#undef RDO_MXC_ROW

constexpr int64_t kMaxRows = 0x7fffffffLL;

// (input pixels, Ho, Wo, output pixels) of a geometry; false for a refused one.  Every product is formed where it cannot overflow.
struct ConvPixels {
    int64_t in, Ho, Wo, out;
};

inline bool conv_pixels(int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad, ConvPixels& p) {
    if (B <= 0 || H <= 0 || W <= 0 || k <= 0 || stride <= 0 || pad < 0) return false;
    const int64_t eh = (int64_t)H + 2 * (int64_t)pad - k, ew = (int64_t)W + 2 * (int64_t)pad - k;
    if (eh < 0 || ew < 0) return false;
    p.Ho = eh / stride + 1;
    p.Wo = ew / stride + 1;
    const int64_t hw = (int64_t)H * W;                                          // < 2^62
    if (hw > kMaxRows / B) return false;
    p.in = hw * B;
    if (p.Ho > kMaxRows / p.Wo) return false;                                   // Ho, Wo < 2^33
    if (p.Ho * p.Wo > kMaxRows / B) return false;
    p.out = p.Ho * p.Wo * B;
    return true;
}

}  // namespace

extern "C" {

int64_t rdo_mx_conv2d_out_pixels(int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad) {
    ConvPixels p;
    return conv_pixels(B, H, W, k, stride, pad, p) ? p.out : 0;
}

int rdo_mx_conv2d(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales, int32_t w_format,
                  int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad, const float* bias, float* y,
                  void* stream) {
    RDO_REQUIRE(x && x_scales && w && w_scales && y, "rdo_mx_conv2d: null pointer");
    RDO_REQUIRE(aligned4(x) && aligned4(w) && aligned4(bias) && aligned4(y), "rdo_mx_conv2d: x, w, bias and y must be 4-byte aligned");
    MxFormat fx, fw;
    RDO_REQUIRE(mx_format(x_format, fx), "rdo_mx_conv2d: unknown x_format %d (0 .. %d)", (int)x_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(mx_format(w_format, fw), "rdo_mx_conv2d: unknown w_format %d (0 .. %d)", (int)w_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && N > 0 && k > 0 && stride > 0 && pad >= 0,
                "rdo_mx_conv2d: non-positive size B %d H %d W %d C %d N %d k %d stride %d, or pad %d < 0", B, H, W, C, N, k, stride, pad);
    RDO_REQUIRE(C % kBlock == 0, "rdo_mx_conv2d: C %d is no multiple of the block size %d", C, kBlock);
    RDO_REQUIRE((int64_t)H + 2 * (int64_t)pad >= k && (int64_t)W + 2 * (int64_t)pad >= k,
                "rdo_mx_conv2d: kernel %d does not fit the padded input %d x %d (pad %d)", k, H, W, pad);
    ConvPixels p;
    RDO_REQUIRE(conv_pixels(B, H, W, k, stride, pad, p), "rdo_mx_conv2d: B %d x H %d x W %d input or the output pixels exceed 2^31 - 1", B, H, W);
    const long cb = C / kBlock;                                                 // < 2^26
    const long total_x = p.in * cb;                                             // < 2^57
    // blocks of a weight row k k cb and of the weight, each product formed below 2^63
    const bool row_fits = k <= (1 << 20) && cb <= kMaxBlocks / ((long)k * k);
    const long nb = row_fits ? (long)k * k * cb : 0;
    RDO_REQUIRE(total_x <= kMaxBlocks && row_fits && nb <= kMaxBlocks / N,
                "rdo_mx_conv2d: B %d H %d W %d C %d N %d k %d make more than 2^40 blocks in an operand", B, H, W, C, N, k);
    const long total_w = nb * N;
    const long tiles_m = rdo::ceil_div(p.out, 64), tiles_n = rdo::ceil_div(N, 64);
    RDO_REQUIRE(tiles_m * tiles_n <= 0x7fffffffL, "rdo_mx_conv2d: %lld output pixels x N %d make more than 2^31 - 1 output tiles",
                (long long)p.out, N);
    const ConvKernel kern = kConv[hw_format(x_format)][hw_format(w_format)];
    const uint32_t* px = static_cast<const uint32_t*>(x);
    const uint32_t* pw = static_cast<const uint32_t*>(w);
    const int icb = (int)cb, Ho = (int)p.Ho, Wo = (int)p.Wo, M = (int)p.out, tn = (int)tiles_n;
    const unsigned grid = (unsigned)(tiles_m * tiles_n);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, px, x_scales, pw, w_scales, H, W, icb, k, stride, pad, Ho, Wo, M, N, nb, tn,
                               bias, y);
            return rdo::check_launch("mx_conv2d");
        },
        stream, "mx_conv2d", 2.0 * (double)M * (double)N * (double)nb * kBlock,
        (double)total_x * (4.0 * fx.bits + 1.0) + (double)total_w * (4.0 * fw.bits + 1.0) + (double)M * (double)N * 4.0);
}

}  // extern "C"
