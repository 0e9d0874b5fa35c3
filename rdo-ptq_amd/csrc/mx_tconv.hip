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
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxtconv.h"
#include "mx_mfma_device.h"

namespace {

// (channel block, tap row a, tap column e) of one block index of the gathered row, advanced by the four blocks of a K step
struct TapWalk {
    int c, a, e;
};

__device__ __forceinline__ TapWalk tap_start(int q, int cb, int tx) {           // q < 6: once per lane; tx >= 1
    const int t = q / cb;
    return TapWalk{q - t * cb, t / tx, t % tx};
}

__device__ __forceinline__ void tap_advance(TapWalk& w, int cb, int tx) {
    w.c += 4;
    while (w.c >= cb) {                                                         // at most four times: cb >= 1
        w.c -= cb;
        if (++w.e == tx) {
            w.e = 0;
            ++w.a;
        }
    }
}

// what the K loop keeps of an output pixel: the input position of tap (a, e) = (0, 0) and the index of that (possibly virtual) pixel
struct Pixel {
    long iy0, ix0, at0;
    bool ok;
};

// the geometry of the phase, uniform over the workgroup
struct Phase {
    int ry, rx, s, k;
    long wtap0;                                                                 // weight block of tap (0, 0) of the phase, before cb
};

// the blocks a walk points at for a pixel: x's (with whether it lies in the image) and the offset into a weight row
__device__ __forceinline__ bool tap_block(const Pixel& p, const TapWalk& w, long q, long nb, int H, int W, int cb, long& blk) {
    const long iy = p.iy0 - w.a, ix = p.ix0 - w.e;
    blk = (p.at0 - (long)w.a * W - w.e) * cb + w.c;
    return p.ok && q < nb && iy >= 0 && iy < H && ix >= 0 && ix < W;
}

__device__ __forceinline__ long weight_block(const Phase& ph, const TapWalk& w, int cb) {
    return (ph.wtap0 + ((long)w.a * ph.k + w.e) * ph.s) * cb + w.c;             // ((ry + a s) k + rx + e s) cb + c
}

// first output coordinate of a phase r and how many there are below `n`: o = o0 + j s
__device__ __forceinline__ void phase_range(int r, int s, int pad, int n, long& o0, long& count) {
    o0 = (((long)r - pad) % s + s) % s;
    count = o0 < n ? (n - o0 + s - 1) / s : 0;
}

template <int FX, int FW>
__global__ __launch_bounds__(256) void mx_tconv_kernel(const uint32_t* __restrict__ x, const uint8_t* __restrict__ sx,
                                                       const uint32_t* __restrict__ w, const uint8_t* __restrict__ sw, int B, int H, int W,
                                                       int cb, int k, int s, int pad, int Ho, int Wo, int N, int tiles_m, int tiles_n,
                                                       const float* __restrict__ bias, float* __restrict__ y) {
    constexpr int DX = hw_dwords(FX), DW = hw_dwords(FW);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kg = lane >> 4;
    // phase and tile from the block index (uniform)
    const unsigned per_phase = (unsigned)tiles_m * (unsigned)tiles_n;
    const unsigned p = blockIdx.x / per_phase, t = blockIdx.x - p * per_phase;
    const unsigned tm = t / (unsigned)tiles_n, tn = t - tm * (unsigned)tiles_n;
    Phase ph;
    ph.ry = (int)(p / (unsigned)s);
    ph.rx = (int)(p - (unsigned)ph.ry * (unsigned)s);
    ph.s = s;
    ph.k = k;
    ph.wtap0 = (long)ph.ry * k + ph.rx;
    long oy0, ox0, ny, nx;
    phase_range(ph.ry, s, pad, Ho, oy0, ny);
    phase_range(ph.rx, s, pad, Wo, ox0, nx);
    const long M = (long)B * ny * nx;                                           // <= B Ho Wo <= 2^31 - 1
    const long m0 = (long)tm * 64 + (wave >> 1) * 32, n0 = (long)tn * 64 + (wave & 1) * 32;
    if (m0 >= M || n0 >= N) return;                                             // uniform over the wave; the kernel has no barrier
    const int ty = ph.ry < k ? (int)(((long)k - ph.ry + s - 1) / s) : 0, tx = ph.rx < k ? (int)(((long)k - ph.rx + s - 1) / s) : 0;
    const long nb = (long)ty * tx * cb;                                         // blocks of the phase's gathered row
    const long nbw = (long)k * k * cb;                                          // blocks of a weight row
    const long qy0 = (oy0 + pad - ph.ry) / s, qx0 = (ox0 + pad - ph.rx) / s;    // exact and >= 0
    const unsigned unx = (unsigned)nx, uplane = (unsigned)(ny * nx);
    Pixel px[2];
    long brow[2];
    bool bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long m = m0 + 16 * i + r;
        px[i].ok = m < M;
        const unsigned mm = px[i].ok ? (unsigned)m : 0u;                        // M <= 2^31 - 1: 32-bit divisions, once per lane
        const unsigned b = mm / uplane, rem = mm - b * uplane;
        const unsigned jy = rem / unx, jx = rem - jy * unx;
        px[i].iy0 = qy0 + jy;
        px[i].ix0 = qx0 + jx;
        px[i].at0 = ((long)b * H + px[i].iy0) * W + px[i].ix0;
        bok[i] = n0 + 16 * i + r < N;
        brow[i] = (n0 + 16 * i + r) * nbw;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nb > 0) {
        // the blocks the lane owns in a step: kg (its scale; FP4 / FP6: its operand) and, FP8, the half blocks of kg / 2 and 2 + kg / 2
        TapWalk ws = tap_start(kg, cb, tx), w0 = tap_start(kg >> 1, cb, tx), w1 = tap_start(2 + (kg >> 1), cb, tx);
        for (long k0 = 0; k0 < nb; k0 += 4) {
            const long kb = k0 + kg, h0 = k0 + (kg >> 1), h1 = h0 + 2;
            const bool kok = kb < nb;
            const long wbs = weight_block(ph, ws, cb), wb0 = weight_block(ph, w0, cb), wb1 = weight_block(ph, w1, cb);
            i32x8 fa[2], fb[2];
            int xa[2], xb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                long bs;
                const bool oks = tap_block(px[i], ws, kb, nb, H, W, cb, bs);
                if constexpr (DX == 8) {
                    long b0, b1;
                    const bool ok0 = tap_block(px[i], w0, h0, nb, H, W, cb, b0);
                    const bool ok1 = tap_block(px[i], w1, h1, nb, H, W, cb, b1);
                    fa[i] = load_blocks<8>(x + b0 * 8, ok0, x + b1 * 8, ok1, kg);
                } else {
                    fa[i] = load_blocks<DX>(x + bs * DX, oks, x, false, kg);
                }
                xa[i] = oks ? (int)sx[bs] : 127;
                if constexpr (DW == 8) {
                    fb[i] = load_blocks<8>(w + (brow[i] + wb0) * 8, bok[i] && h0 < nb, w + (brow[i] + wb1) * 8, bok[i] && h1 < nb, kg);
                } else {
                    fb[i] = load_blocks<DW>(w + (brow[i] + wbs) * DW, bok[i] && kok, w, false, kg);
                }
                xb[i] = bok[i] && kok ? (int)sw[brow[i] + wbs] : 127;
            }
            mx_mfma_step<FX, FW>(fa, fb, xa, xb, acc);
            tap_advance(ws, cb, tx);
            if constexpr (DX == 8 || DW == 8) {
                tap_advance(w0, cb, tx);
                tap_advance(w1, cb, tx);
            }
        }
    }
    // the wave's 32 x 32 outputs, bias added, each tile row at its output pixel.  C/D: col = lane & 15 (r), row = 4 (lane >> 4) + reg.
    long at[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long m = m0 + 16 * i + 4 * kg + q;
            const unsigned mm = m < M ? (unsigned)m : 0u;
            const unsigned b = mm / uplane, rem = mm - b * uplane;
            const unsigned jy = rem / unx, jx = rem - jy * unx;
            at[i][q] = m < M ? (((long)b * Ho + oy0 + (long)jy * s) * Wo + ox0 + (long)jx * s) * N : -1;
        }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long col = n0 + 16 * j + r;
        if (col >= N) continue;
        const float bj = bias ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (at[i][q] >= 0) y[at[i][q] + col] = acc[i][j][q] + bj;
    }
}

using TconvKernel = void (*)(const uint32_t*, const uint8_t*, const uint32_t*, const uint8_t*, int, int, int, int, int, int, int, int, int, int,
                             int, int, const float*, float*);

#define RDO_MXT_ROW(FX) {mx_tconv_kernel<FX, 0>, mx_tconv_kernel<FX, 1>, mx_tconv_kernel<FX, 2>, mx_tconv_kernel<FX, 3>, mx_tconv_kernel<FX, 4>}
const TconvKernel kTconv[5][5] = {RDO_MXT_ROW(0), RDO_MXT_ROW(1), RDO_MXT_ROW(2), RDO_MXT_ROW(3), RDO_MXT_ROW(4)};
#undef RDO_MXT_ROW

constexpr int64_t kMaxRows = 0x7fffffffLL;

// (input pixels, Ho, Wo, output pixels) of a geometry; false for a refused one.  Every product is formed where it cannot overflow.
struct TconvPixels {
    int64_t in, Ho, Wo, out;
};

inline bool tconv_pixels(int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad, int32_t opad, TconvPixels& p) {
    if (B <= 0 || H <= 0 || W <= 0 || k <= 0 || stride <= 0 || pad < 0 || opad < 0 || opad >= stride) return false;
    p.Ho = ((int64_t)H - 1) * stride - 2 * (int64_t)pad + k + opad;             // |.| < 2^63
    p.Wo = ((int64_t)W - 1) * stride - 2 * (int64_t)pad + k + opad;
    if (p.Ho <= 0 || p.Wo <= 0) return false;
    const int64_t hw = (int64_t)H * W;                                          // < 2^62
    if (hw > kMaxRows / B) return false;
    p.in = hw * B;
    if (p.Ho > kMaxRows / p.Wo) return false;
    if (p.Ho * p.Wo > kMaxRows / B) return false;
    p.out = p.Ho * p.Wo * B;
    return true;
}

}  // namespace

extern "C" {

int64_t rdo_mx_conv_transpose2d_out_pixels(int32_t B, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad, int32_t output_padding) {
    TconvPixels p;
    return tconv_pixels(B, H, W, k, stride, pad, output_padding, p) ? p.out : 0;
}

int rdo_mx_conv_transpose2d(const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales, int32_t w_format,
                            int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad,
                            int32_t output_padding, const float* bias, float* y, void* stream) {
    RDO_REQUIRE(x && x_scales && w && w_scales && y, "rdo_mx_conv_transpose2d: null pointer");
    RDO_REQUIRE(aligned4(x) && aligned4(w) && aligned4(bias) && aligned4(y),
                "rdo_mx_conv_transpose2d: x, w, bias and y must be 4-byte aligned");
    MxFormat fx, fw;
    RDO_REQUIRE(mx_format(x_format, fx), "rdo_mx_conv_transpose2d: unknown x_format %d (0 .. %d)", (int)x_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(mx_format(w_format, fw), "rdo_mx_conv_transpose2d: unknown w_format %d (0 .. %d)", (int)w_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && N > 0 && k > 0 && stride > 0 && pad >= 0,
                "rdo_mx_conv_transpose2d: non-positive size B %d H %d W %d C %d N %d k %d stride %d, or pad %d < 0", B, H, W, C, N, k, stride,
                pad);
    RDO_REQUIRE(output_padding >= 0 && output_padding < stride, "rdo_mx_conv_transpose2d: output_padding %d is not in 0 .. stride - 1 = %d",
                output_padding, stride - 1);
    RDO_REQUIRE(C % kBlock == 0, "rdo_mx_conv_transpose2d: C %d is no multiple of the block size %d", C, kBlock);
    RDO_REQUIRE(((int64_t)H - 1) * stride - 2 * (int64_t)pad + k + output_padding > 0 &&
                    ((int64_t)W - 1) * stride - 2 * (int64_t)pad + k + output_padding > 0,
                "rdo_mx_conv_transpose2d: input %d x %d, kernel %d, stride %d, pad %d, output_padding %d leave no output", H, W, k, stride, pad,
                output_padding);
    TconvPixels p;
    RDO_REQUIRE(tconv_pixels(B, H, W, k, stride, pad, output_padding, p),
                "rdo_mx_conv_transpose2d: B %d x H %d x W %d input or the output pixels exceed 2^31 - 1", B, H, W);
    const long cb = C / kBlock;                                                 // < 2^26
    const long total_x = p.in * cb;                                             // < 2^57
    // blocks of a weight row k k cb and of the weight, each product formed below 2^63
    const bool row_fits = k <= (1 << 20) && cb <= kMaxBlocks / ((long)k * k);
    const long nbw = row_fits ? (long)k * k * cb : 0;
    RDO_REQUIRE(total_x <= kMaxBlocks && row_fits && nbw <= kMaxBlocks / N,
                "rdo_mx_conv_transpose2d: B %d H %d W %d C %d N %d k %d make more than 2^40 blocks in an operand", B, H, W, C, N, k);
    const long total_w = nbw * N;
    // tiles of the largest phase, ceil(Ho / s) x ceil(Wo / s) pixels an image (<= Ho Wo), times the s s phases
    const long pix = rdo::ceil_div(p.Ho, (int64_t)stride) * rdo::ceil_div(p.Wo, (int64_t)stride) * B;
    const long tiles_m = rdo::ceil_div(pix, 64), tiles_n = rdo::ceil_div(N, 64);
    const long per_phase = tiles_m * tiles_n;                                   // < 2^50
    RDO_REQUIRE(per_phase <= 0x7fffffffL && (long)stride * stride <= 0x7fffffffL / per_phase,
                "rdo_mx_conv_transpose2d: %lld output pixels x N %d in %d x %d phases make more than 2^31 - 1 output tiles", (long long)p.out, N,
                stride, stride);
    const TconvKernel kern = kTconv[hw_format(x_format)][hw_format(w_format)];
    const uint32_t* px = static_cast<const uint32_t*>(x);
    const uint32_t* pw = static_cast<const uint32_t*>(w);
    const int icb = (int)cb, Ho = (int)p.Ho, Wo = (int)p.Wo, tm = (int)tiles_m, tn = (int)tiles_n;
    const unsigned grid = (unsigned)(per_phase * stride * stride);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, px, x_scales, pw, w_scales, B, H, W, icb, k, stride, pad, Ho, Wo, N, tm, tn, bias,
                               y);
            return rdo::check_launch("mx_conv_transpose2d");
        },
        stream, "mx_conv_transpose2d", 2.0 * (double)p.in * (double)N * (double)nbw * kBlock,
        (double)total_x * (4.0 * fx.bits + 1.0) + (double)total_w * (4.0 * fw.bits + 1.0) + (double)p.out * (double)N * 4.0);
}

}  // extern "C"
