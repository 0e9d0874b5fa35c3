// What mx_tconv.hip (fp32 output) and mx_chain.hip (packed MX output) share of the phase-wise transposed convolution on packed MX
// operands (include/rdo_ptq_mxtconv.h): the phase and tile of a workgroup, the walk over a phase's taps, the K loop for a wave's 32 x 32
// outputs, the output pixel of a tile row, and the argument checks with the launch geometry.  mx_tconv.hip's head comment states the
// mapping.  Included once per translation unit; the names live in `mxtconv` because mx_conv_device.h has a TapWalk and a Pixel of its own.
#pragma once
#include "mx_mfma_device.h"

namespace {
namespace mxtconv {

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

// the phase of a workgroup, its pixels and the wave's 32 x 32 tile of them
struct PhaseTile {
    Phase ph;
    long oy0, ox0, ny, nx, M, m0, n0;
};

// phase and tile from the block index (uniform over the wave); false for a tile past its phase's pixels or past N: the wave returns
__device__ __forceinline__ bool phase_tile(int B, int k, int s, int pad, int Ho, int Wo, int N, int tiles_m, int tiles_n, PhaseTile& t) {
    const int wave = threadIdx.x >> 6;
    const unsigned per_phase = (unsigned)tiles_m * (unsigned)tiles_n;
    const unsigned p = blockIdx.x / per_phase, tt = blockIdx.x - p * per_phase;
    const unsigned tm = tt / (unsigned)tiles_n, tn = tt - tm * (unsigned)tiles_n;
    t.ph.ry = (int)(p / (unsigned)s);
    t.ph.rx = (int)(p - (unsigned)t.ph.ry * (unsigned)s);
    t.ph.s = s;
    t.ph.k = k;
    t.ph.wtap0 = (long)t.ph.ry * k + t.ph.rx;
    phase_range(t.ph.ry, s, pad, Ho, t.oy0, t.ny);
    phase_range(t.ph.rx, s, pad, Wo, t.ox0, t.nx);
    t.M = (long)B * t.ny * t.nx;                                                // <= B Ho Wo <= 2^31 - 1
    t.m0 = (long)tm * 64 + (wave >> 1) * 32;
    t.n0 = (long)tn * 64 + (wave & 1) * 32;
    return t.m0 < t.M && t.n0 < N;
}

// the output pixel (b Ho + oy) Wo + ox of row m of the phase's pixels, -1 past them
__device__ __forceinline__ long out_pixel(const PhaseTile& t, long m, int Ho, int Wo) {
    const unsigned unx = (unsigned)t.nx, uplane = (unsigned)(t.ny * t.nx);
    const unsigned mm = m < t.M ? (unsigned)m : 0u;
    const unsigned b = mm / uplane, rem = mm - b * uplane;
    const unsigned jy = rem / unx, jx = rem - jy * unx;
    return m < t.M ? ((long)b * Ho + t.oy0 + (long)jy * t.ph.s) * Wo + t.ox0 + (long)jx * t.ph.s : -1;
}

// The K loop of the phase for the wave's 32 x 32 outputs: what mx_tconv_kernel stores and mx_tconv_packed_kernel quantises -- one
// statement, equal accumulators.  A phase without taps leaves them zero.
template <int FX, int FW>
__device__ __forceinline__ void accumulate(const uint32_t* __restrict__ x, const uint8_t* __restrict__ sx, const uint32_t* __restrict__ w,
                                           const uint8_t* __restrict__ sw, int H, int W, int cb, int pad, int N, const PhaseTile& t, int r,
                                           int kg, f32x4 (&acc)[2][2]) {
    constexpr int DX = hw_dwords(FX), DW = hw_dwords(FW);
    const Phase& ph = t.ph;
    const int k = ph.k, s = ph.s;
    const int ty = ph.ry < k ? (int)(((long)k - ph.ry + s - 1) / s) : 0, tx = ph.rx < k ? (int)(((long)k - ph.rx + s - 1) / s) : 0;
    const long nb = (long)ty * tx * cb;                                         // blocks of the phase's gathered row
    const long nbw = (long)k * k * cb;                                          // blocks of a weight row
    const long qy0 = (t.oy0 + pad - ph.ry) / s, qx0 = (t.ox0 + pad - ph.rx) / s;    // exact and >= 0
    const unsigned unx = (unsigned)t.nx, uplane = (unsigned)(t.ny * t.nx);
    Pixel px[2];
    long brow[2];
    bool bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long m = t.m0 + 16 * i + r;
        px[i].ok = m < t.M;
        const unsigned mm = px[i].ok ? (unsigned)m : 0u;                        // M <= 2^31 - 1: 32-bit divisions, once per lane
        const unsigned b = mm / uplane, rem = mm - b * uplane;
        const unsigned jy = rem / unx, jx = rem - jy * unx;
        px[i].iy0 = qy0 + jy;
        px[i].ix0 = qx0 + jx;
        px[i].at0 = ((long)b * H + px[i].iy0) * W + px[i].ix0;
        bok[i] = t.n0 + 16 * i + r < N;
        brow[i] = (t.n0 + 16 * i + r) * nbw;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nb <= 0) return;
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

// what rdo_mx_conv_transpose2d and rdo_mx_conv_transpose2d_packed check of their operands (`who`: the entry's name), and the launch
// they share
struct TconvPlan {
    long total_x, total_w, nbw, in, out;
    int bits_x, bits_w, cb, Ho, Wo, tiles_m, tiles_n;
    unsigned grid;
};

inline int check(const char* who, const void* x, const uint8_t* x_scales, int32_t x_format, const void* w, const uint8_t* w_scales,
                 int32_t w_format, int32_t B, int32_t H, int32_t W, int32_t C, int32_t N, int32_t k, int32_t stride, int32_t pad,
                 int32_t output_padding, const float* bias, TconvPlan& c) {
    RDO_REQUIRE(x && x_scales && w && w_scales, "%s: null pointer", who);
    RDO_REQUIRE(aligned4(x) && aligned4(w) && aligned4(bias), "%s: x, w, bias and y must be 4-byte aligned", who);
    MxFormat fx, fw;
    RDO_REQUIRE(mx_format(x_format, fx), "%s: unknown x_format %d (0 .. %d)", who, (int)x_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(mx_format(w_format, fw), "%s: unknown w_format %d (0 .. %d)", who, (int)w_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && N > 0 && k > 0 && stride > 0 && pad >= 0,
                "%s: non-positive size B %d H %d W %d C %d N %d k %d stride %d, or pad %d < 0", who, B, H, W, C, N, k, stride, pad);
    RDO_REQUIRE(output_padding >= 0 && output_padding < stride, "%s: output_padding %d is not in 0 .. stride - 1 = %d", who, output_padding,
                stride - 1);
    RDO_REQUIRE(C % kBlock == 0, "%s: C %d is no multiple of the block size %d", who, C, kBlock);
    RDO_REQUIRE(((int64_t)H - 1) * stride - 2 * (int64_t)pad + k + output_padding > 0 &&
                    ((int64_t)W - 1) * stride - 2 * (int64_t)pad + k + output_padding > 0,
                "%s: input %d x %d, kernel %d, stride %d, pad %d, output_padding %d leave no output", who, H, W, k, stride, pad, output_padding);
    TconvPixels p;
    RDO_REQUIRE(tconv_pixels(B, H, W, k, stride, pad, output_padding, p), "%s: B %d x H %d x W %d input or the output pixels exceed 2^31 - 1",
                who, B, H, W);
    const long cb = C / kBlock;                                                 // < 2^26
    const long total_x = p.in * cb;                                             // < 2^57
    // blocks of a weight row k k cb and of the weight, each product formed below 2^63
    const bool row_fits = k <= (1 << 20) && cb <= kMaxBlocks / ((long)k * k);
    const long nbw = row_fits ? (long)k * k * cb : 0;
    RDO_REQUIRE(total_x <= kMaxBlocks && row_fits && nbw <= kMaxBlocks / N, "%s: B %d H %d W %d C %d N %d k %d make more than 2^40 blocks in an operand",
                who, B, H, W, C, N, k);
    // tiles of the largest phase, ceil(Ho / s) x ceil(Wo / s) pixels an image (<= Ho Wo), times the s s phases
    const long pix = rdo::ceil_div(p.Ho, (int64_t)stride) * rdo::ceil_div(p.Wo, (int64_t)stride) * B;
    const long tiles_m = rdo::ceil_div(pix, 64), tiles_n = rdo::ceil_div(N, 64);
    const long per_phase = tiles_m * tiles_n;                                   // < 2^50
    RDO_REQUIRE(per_phase <= 0x7fffffffL && (long)stride * stride <= 0x7fffffffL / per_phase,
                "%s: %lld output pixels x N %d in %d x %d phases make more than 2^31 - 1 output tiles", who, (long long)p.out, N, stride, stride);
    c = TconvPlan{total_x, nbw * N, nbw, p.in, p.out, fx.bits, fw.bits, (int)cb, (int)p.Ho, (int)p.Wo, (int)tiles_m, (int)tiles_n,
                  (unsigned)(per_phase * stride * stride)};
    return RDO_OK;
}

}  // namespace mxtconv
}  // namespace
