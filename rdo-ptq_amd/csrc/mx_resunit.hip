// The residual unit of the Cheng2020 attention block on the block-scaled matrix instruction, one launch (include/rdo_ptq_mxresunit.h):
//   rdo_mx_residual_unit:  out = relu(x + conv1x1(relu(conv3x3(relu(conv1x1(x))))))  with x, h1 and h2 each quantised to the activation format
// Built with -ffp-contract=off and without packed fp32 instructions like mx_chain.hip: acc + bias, the ReLUs and x + branch are separate
// fp32 operations, one rounding each.
//
// mx_resunit_kernel<FA, FB>: a workgroup of 256 threads owns an 8 x 8 tile of output pixels of one image; the grid is B ceil(H / 8)
// ceil(W / 8).  The 3 x 3 needs h1 on the tile's 10 x 10 halo, so the first 1 x 1 is computed on 100 pixels (1.56 x the tile's) and
// nothing but x is read from memory twice.  Dynamic LDS, two packed images of 100 rows with their scale bytes:
//   image X   [100][strideX] dwords   the halo of x, K = N         scales X  [100][N / 32] bytes
//   image H1  [100][strideH] dwords   the halo of h1, K = N / 2    scales H1 [100][N / 64] bytes
//   image H2  [64][strideH] dwords and scales H2 [64][N / 64]: the tile of h2, in the place of image X / scales X, which are dead by then
//   (row strides by lds_row_dwords, mx_swin_device.h), beside the 4 608 B of mx_pack_tile's static wave-private byte tiles.  Dynamic +
//   static bytes in FP8: N = 128: 23 000 + 4 608 = 27 608 (5 workgroups a CU by LDS: gfx950 has 163 840 B a CU); N = 192: 32 900 + 4 608
//   = 37 508 (4 a CU); N = 320: 52 700 + 4 608 = 57 308 (2 a CU).  FP4 at N = 192: 16 900 + 4 608 = 21 508 (7 a CU).  Never above
//   65 536: no dynamic-LDS attribute is raised (RDO_MXRESUNIT_MAX_N).
// Halo row hr = 10 hy + hx is the pixel (ty0 - 1 + hy, tx0 - 1 + hx) of image b; the tile's pixel (py, px) is halo row 10 (py + 1) +
// px + 1 and row 8 py + px of image H2.  A halo pixel outside ITS OWN image -- past any of the four borders; the test is on (gy, gx), so
// a halo never reaches into the neighbouring image of the batch -- is the 3 x 3's zero padding: zero codes under the scale byte 127, in
// image X and, whatever relu(b1) is, in image H1 -- the registers and the scale rdo_mx_conv2d gives a tap outside the image.
// Phase 0.  Seven passes of 16 rows, 16 lanes a row, lane l16 holds float4 l16 + 16 k: the eight neighbouring lanes of one k hold one
//   block, which mx_quad_quant_store quantises and places (rdo_mx_quant_pack's bits).                        __syncthreads.
// Phase 1.  4 N / 64 units of 32 halo rows x 32 channels of h1 (unit u = channel block u >> 2, rows 32 (u & 3)) to wave u % 4: A
//   fragments from image X (rows past 99 read row 99 and are dropped), B from w1 in global memory (L2 resident); relu(acc + b1),
//   mx_pack_tile, the dwords to image H1.                                                                     __syncthreads.
// Phase 2.  2 N / 64 units of 32 tile pixels x 32 channels of h2: the implicit GEMM of mxconv::accumulate with the A side in image H1
//   -- block kb of a pixel's im2col row is channel block kb % cb of tap kb / cb, halo row 10 (py + kh) + px + kw; the K steps of four
//   blocks straddle taps where cb = N / 64 is no multiple of four and the last one is short (nb = 9 cb), exactly as there --; relu(acc +
//   b2), mx_pack_tile, the dwords to image H2.                                                                __syncthreads.
// Phase 3.  2 N / 32 units of 32 tile pixels x 32 channels: unit_accumulate from image H2 against w3; branch = acc + b3, s = x + branch
//   (x read again: the lines phase 0 read), out = relu(s) as relu_fwd's element.
// The optional outputs are stored where their values are made: xp copied from image X after phase 0, h1 / h2 from the pack epilogues
// (interior pixels only), branch in phase 3.  The two pack epilogues are one closure, so mx_pack_tile is instantiated once and its
// static byte tiles exist once: the compiler reports 4 608 B of static LDS for every instantiation of the kernel.
// Ragged tiles: no thread returns or skips a barrier.  A unit of phases 2 and 3 whose 32 pixels (tile rows 4 .. 7) lie below the image is
// skipped by its wave between the barriers; pixels outside the image inside a unit store nothing.
// Why 32-row units and not the 16-row ones 100 rows suggest (112 instead of 128 rows in phase 1): mx_pack_tile, unit_accumulate and the
// accumulator layout they share are statements the suite pins bit for bit; phase 1 is the smallest of the three products (K = N against
// 9 N / 2 for half as many rows in phase 2).
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxresunit.h"
#include "mx_conv_device.h"
#include "mx_swin_device.h"

namespace {

constexpr int kTile = 8, kHalo = kTile + 2, kHaloRows = kHalo * kHalo, kTileRows = kTile * kTile;

struct ResUnitArgs {
    const float* x;
    int H, W, N, nbN, cb, strideX, strideH, tiles_x, tiles_y;                   // cb: blocks of N / 2; strides: dwords of an LDS row
    MxFormat fa;                                                                // the activation format
    const uint32_t *w1, *w2, *w3;
    const uint8_t *s1, *s2, *s3;
    const float *b1, *b2, *b3;                                                  // nullable
    float *out, *branch;                                                        // branch nullable
    uint32_t *xp, *h1, *h2;                                                     // nullable, each with its scale bytes
    uint8_t *xs, *h1s, *h2s;
};

// dynamic LDS bytes of a workgroup: the two halo images and their scale bytes
constexpr size_t resunit_lds(int N, int bits) {
    return (size_t)kHaloRows * 4 * (lds_row_dwords(N / 32, bits) + lds_row_dwords(N / 64, bits)) + (size_t)kHaloRows * (N / 32 + N / 64);
}
// LDS of a workgroup beside the dynamic part: mx_pack_tile's four wave-private byte tiles
constexpr size_t kStaticLds = 4 * 32 * kPackRowDwords * sizeof(uint32_t);
static_assert(RDO_MXRESUNIT_MAX_N % 64 == 0 && resunit_lds(RDO_MXRESUNIT_MAX_N, 8) + kStaticLds <= 64 * 1024 &&
                  resunit_lds(RDO_MXRESUNIT_MAX_N + 64, 8) + kStaticLds > 64 * 1024,
              "RDO_MXRESUNIT_MAX_N is the most channels whose FP8 images fit 64 KiB of LDS");

// mxconv::accumulate for the wave's 32 tile pixels x 32 channels at (m0, n0) with the A side in the halo image of h1: 3 x 3, stride 1,
// the padding already in the image as zero codes under the scale 127.  The walk over the taps, the K order, the trailing blocks' scale
// and the B side are that function's: a change there has to be made here too; tests/test_gpu_mx_resunit.py holds the two to equal bits.
template <int FA, int FB>
__device__ __forceinline__ void halo_conv_accumulate(const uint32_t* image, int stride, const uint8_t* scales, int cb,
                                                     const uint32_t* __restrict__ w, const uint8_t* __restrict__ sw, int m0, int n0, int r, int kg,
                                                     f32x4 (&acc)[2][2]) {
    using namespace mxconv;
    constexpr int DA = hw_dwords(FA), DB = hw_dwords(FB);
    const int nb = 9 * cb;
    int hrow[2];                                                                // the halo row of tap (0, 0) of the lane's pixel
    long brow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + 16 * i + r;
        hrow[i] = (m >> 3) * kHalo + (m & 7);
        brow[i] = (long)(n0 + 16 * i + r) * nb;
    }
    TapWalk ws = tap_start(kg, cb, 3), w0 = tap_start(kg >> 1, cb, 3), w1 = tap_start(2 + (kg >> 1), cb, 3);
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
            const int rs = hrow[i] + kHalo * ws.ky + ws.kx;
            if constexpr (DA == 8) {
                const int r0 = hrow[i] + kHalo * w0.ky + w0.kx, r1 = hrow[i] + kHalo * w1.ky + w1.kx;
                fa[i] = load_blocks<8>(image + r0 * stride + w0.c * 8, k0 + (kg >> 1) < nb, image + r1 * stride + w1.c * 8,
                                       k0 + 2 + (kg >> 1) < nb, kg);
            } else {
                fa[i] = load_blocks<DA>(image + rs * stride + ws.c * DA, kok, image, false, kg);
            }
            xa[i] = kok ? (int)scales[rs * cb + ws.c] : 127;
            fb[i] = load_fragment<DB>(w + brow[i] * DB, k0, kg, nb, true);
            xb[i] = kok ? (int)sw[brow[i] + kb] : 127;
        }
        mx_mfma_step<FA, FB>(fa, fb, xa, xb, acc);
        tap_advance(ws, cb, 3);
        if constexpr (DA == 8) {
            tap_advance(w0, cb, 3);
            tap_advance(w1, cb, 3);
        }
    }
}

// v = relu(acc + bias[n0 ..]) of a unit, in the accumulator layout (mx_pack_store's step 1)
__device__ __forceinline__ void bias_relu(const f32x4 (&acc)[2][2], const float* __restrict__ bias, int n0, int r, f32x4 (&v)[2][2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float bj = bias ? bias[n0 + 16 * j + r] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[i][j][q] = mx_act(acc[i][j][q] + bj, RDO_MX_ACT_RELU);
    }
}

template <int FA, int FB>
__global__ __launch_bounds__(256) void mx_resunit_kernel(ResUnitArgs p) {
    extern __shared__ uint32_t lds[];
    uint32_t* imageX = lds;
    uint32_t* imageH1 = imageX + kHaloRows * p.strideX;
    uint8_t* scalesX = reinterpret_cast<uint8_t*>(imageH1 + kHaloRows * p.strideH);
    uint8_t* scalesH1 = scalesX + kHaloRows * p.nbN;
    uint32_t* imageH2 = imageX;                                                 // 64 strideH <= 100 strideX, 64 cb <= 100 nbN
    uint8_t* scalesH2 = scalesX;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int H = p.H, W = p.W, N = p.N, nbN = p.nbN, cb = p.cb, bits = p.fa.bits;
    const int tx = blockIdx.x % p.tiles_x, tyb = blockIdx.x / p.tiles_x;
    const int ty = tyb % p.tiles_y, b = tyb / p.tiles_y;
    const int ty0 = ty * kTile, tx0 = tx * kTile;
    const long image0 = (long)b * H * W;                                        // the first pixel of image b
    // the pixel of halo row hr and whether it lies in the image
    auto halo_pixel = [&](int hr, int& gy, int& gx) {
        const int hy = hr / kHalo;
        gy = ty0 - 1 + hy;
        gx = tx0 - 1 + hr - kHalo * hy;
        return hr < kHaloRows && gy >= 0 && gy < H && gx >= 0 && gx < W;
    };

    // ---- phase 0: the halo of x -> packed blocks and scale bytes of image X ------------------------------------------------------------
    {
        const int l16 = threadIdx.x & 15, grp = threadIdx.x >> 4, N4 = N >> 2;
        for (int pass = 0; pass < (kHaloRows + 15) / 16; ++pass) {
            const int hr = 16 * pass + grp;
            int gy, gx;
            const bool in = halo_pixel(hr, gy, gx);
            const ln4* src = reinterpret_cast<const ln4*>(p.x) + (in ? (image0 + (long)gy * W + gx) * N4 : 0L);
            for (int c0 = 0; c0 < N4; c0 += 16) {                               // the same trips for every lane: the quantiser shuffles
                const int c = c0 + l16, kb = c >> 3;
                const bool live = hr < kHaloRows && c < N4;                     // uniform over a block's eight lanes: N4 % 8 == 0
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (in && live) {
                    const ln4 t = src[c];
                    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
                }
                const unsigned sc = mx_quad_quant_store(v, p.fa, imageX + (live ? hr * p.strideX + kb * bits : 0), live);
                if (live && (l16 & 7) == 0) scalesX[hr * nbN + kb] = (uint8_t)(in ? sc : 127u);
            }
        }
    }
    __syncthreads();
    if (p.xp) {                                                                 // the interior rows of image X are xp's rows
        const int rowdw = nbN * bits;
        for (int e = threadIdx.x; e < kTileRows * rowdw; e += 256) {
            const int m = e / rowdw, d = e - m * rowdw, hr = ((m >> 3) + 1) * kHalo + (m & 7) + 1;
            const int gy = ty0 + (m >> 3), gx = tx0 + (m & 7);
            if (gy >= H || gx >= W) continue;
            const long pix = image0 + (long)gy * W + gx;
            p.xp[pix * rowdw + d] = imageX[hr * p.strideX + d];
            if (d < nbN) p.xs[pix * nbN + d] = scalesX[hr * nbN + d];
        }
    }

    // ---- the pack epilogue of phases 1 and 2 ------------------------------------------------------------------------------------------------
    // One closure for both: mx_pack_tile's static byte tiles belong to its instantiation, so two closure types would be two sets of
    // tiles (9 216 B a workgroup); `halo` says which phase calls, m0 / hb are the calling unit's.
    const int r = lane & 15, kg = lane >> 4;
    bool halo = true;
    int m0 = 0, hb = 0;
    auto put = [&](int t, int h, const unsigned (&d)[4], unsigned scale) {
        if (halo) {                                                             // phase 1: halo row m0 + t of image H1
            const int hr = m0 + t;
            if (hr >= kHaloRows) return;
            int gy, gx;
            const bool in = halo_pixel(hr, gy, gx);
            const unsigned zero[4] = {0u, 0u, 0u, 0u};
            mx_put_dwords(imageH1 + hr * p.strideH + hb * bits + h * (bits >> 1), in ? d : zero, bits);
            if (h == 0) scalesH1[hr * cb + hb] = (uint8_t)(in ? scale : 127u);
            if (p.h1 && in && gy >= ty0 && gy < ty0 + kTile && gx >= tx0 && gx < tx0 + kTile) {
                const long blk = (image0 + (long)gy * W + gx) * cb + hb;
                mx_put_dwords(p.h1 + blk * bits + h * (bits >> 1), d, bits);
                if (h == 0) p.h1s[blk] = (uint8_t)scale;
            }
        } else {                                                                // phase 2: tile pixel m0 + t of image H2
            const int m = m0 + t, gy = ty0 + (m >> 3), gx = tx0 + (m & 7);
            mx_put_dwords(imageH2 + m * p.strideH + hb * bits + h * (bits >> 1), d, bits);
            if (h == 0) scalesH2[m * cb + hb] = (uint8_t)scale;
            if (p.h2 && gy < H && gx < W) {
                const long blk = (image0 + (long)gy * W + gx) * cb + hb;
                mx_put_dwords(p.h2 + blk * bits + h * (bits >> 1), d, bits);
                if (h == 0) p.h2s[blk] = (uint8_t)scale;
            }
        }
    };
    // the unit's accumulators -> relu(acc + bias) -> one MX block a row -> `put`
    auto pack_unit = [&](const f32x4 (&acc)[2][2], const float* bias) {
        f32x4 v[2][2];
        bias_relu(acc, bias, 32 * hb, r, v);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                  // the previous unit's byte-tile reads precede these writes
        __builtin_amdgcn_wave_barrier();
        mx_pack_tile(v, p.fa, put);
    };

    // ---- phase 1: h1 = pack(relu(x W1^T + b1)) on the halo -> image H1 ------------------------------------------------------------------
    for (int u = wave; u < 4 * cb; u += 4) {
        m0 = 32 * (u & 3), hb = u >> 2;
        f32x4 acc[2][2];
        unit_accumulate<FA, FB>(imageX, p.strideX, scalesX, nbN, p.w1, p.s1, m0, 32 * hb, r, kg, acc, 0x7fffffff, kHaloRows - 1);
        pack_unit(acc, p.b1);
    }
    __syncthreads();

    // ---- phase 2: h2 = pack(relu(conv3x3(h1, W2) + b2)) on the tile -> image H2 (over image X) ----------------------------------------------
    halo = false;
    for (int u = wave; u < 2 * cb; u += 4) {
        m0 = 32 * (u & 1), hb = u >> 1;
        if (ty0 + (m0 >> 3) >= H) continue;                                     // uniform over the wave; no barrier inside the loop
        f32x4 acc[2][2];
        halo_conv_accumulate<FA, FB>(imageH1, p.strideH, scalesH1, cb, p.w2, p.s2, m0, 32 * hb, r, kg, acc);
        pack_unit(acc, p.b2);
    }
    __syncthreads();

    // ---- phase 3: out = relu(x + (h2 W3^T + b3)) -----------------------------------------------------------------------------------------
    for (int u = wave; u < 2 * nbN; u += 4) {
        const int m0 = 32 * (u & 1), n0 = 32 * (u >> 1);
        if (ty0 + (m0 >> 3) >= H) continue;
        f32x4 acc[2][2];
        unit_accumulate<FA, FB>(imageH2, p.strideH, scalesH2, cb, p.w3, p.s3, m0, n0, r, kg, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + 16 * j + r;
            const float bj = p.b3 ? p.b3[col] : 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int m = m0 + 16 * i + 4 * kg + q, gy = ty0 + (m >> 3), gx = tx0 + (m & 7);
                    if (gy >= H || gx >= W) continue;
                    const long at = (image0 + (long)gy * W + gx) * N + col;
                    const float y = acc[i][j][q] + bj;
                    if (p.branch) p.branch[at] = y;
                    const float s = p.x[at] + y;
                    p.out[at] = s > 0.f ? s : 0.f * s;                          // relu_fwd_kernel's element (elementwise.hip)
                }
        }
    }
}

using ResUnitKernel = void (*)(ResUnitArgs);

// [activation format][weight format]
#define RDO_MXRU_ROW(FA) \
    {mx_resunit_kernel<FA, 0>, mx_resunit_kernel<FA, 1>, mx_resunit_kernel<FA, 2>, mx_resunit_kernel<FA, 3>, mx_resunit_kernel<FA, 4>}
const ResUnitKernel kResUnit[5][5] = {RDO_MXRU_ROW(0), RDO_MXRU_ROW(1), RDO_MXRU_ROW(2), RDO_MXRU_ROW(3), RDO_MXRU_ROW(4)};
#undef RDO_MXRU_ROW

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

int rdo_mx_residual_unit(const float* x, int32_t B, int32_t H, int32_t W, int32_t N, int32_t act_format, const void* w1,
                         const uint8_t* w1_scales, const float* b1, const void* w2, const uint8_t* w2_scales, const float* b2,
                         const void* w3, const uint8_t* w3_scales, const float* b3, int32_t w_format, float* out, void* xp,
                         uint8_t* xp_scales, void* h1, uint8_t* h1_scales, void* h2, uint8_t* h2_scales, float* branch, void* stream) {
    const char* who = "rdo_mx_residual_unit";
    RDO_REQUIRE(x && w1 && w1_scales && w2 && w2_scales && w3 && w3_scales && out, "%s: null pointer", who);
    RDO_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0, "%s: non-positive size B %d H %d W %d N %d", who, (int)B, (int)H, (int)W, (int)N);
    RDO_REQUIRE((int64_t)H * W <= 0x7fffffffLL / B, "%s: B %d x H %d x W %d pixels exceed 2^31 - 1", who, (int)B, (int)H, (int)W);
    RDO_REQUIRE(N % 64 == 0, "%s: N %d is no multiple of 64: N / 2 must be whole MX blocks of %d", who, (int)N, kBlock);
    RDO_REQUIRE(N <= RDO_MXRESUNIT_MAX_N, "%s: N %d is above %d, the most whose halo images fit the kernel's LDS", who, (int)N,
                RDO_MXRESUNIT_MAX_N);
    ResUnitArgs p;
    MxFormat fw;
    RDO_REQUIRE(mx_format(act_format, p.fa), "%s: unknown act_format %d (0 .. %d)", who, (int)act_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(mx_format(w_format, fw), "%s: unknown w_format %d (0 .. %d)", who, (int)w_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE((xp == nullptr) == (xp_scales == nullptr) && (h1 == nullptr) == (h1_scales == nullptr) && (h2 == nullptr) == (h2_scales == nullptr),
                "%s: xp, h1 and h2 each go together with their scale bytes", who);
    RDO_REQUIRE(aligned16(x) && aligned16(out) && aligned16(branch), "%s: x, out and branch must be 16-byte aligned", who);
    RDO_REQUIRE(aligned4(w1) && aligned4(w2) && aligned4(w3) && aligned4(b1) && aligned4(b2) && aligned4(b3) && aligned4(xp) && aligned4(h1) &&
                    aligned4(h2),
                "%s: w1, w2, w3, b1, b2, b3, xp, h1 and h2 must be 4-byte aligned", who);
    const int tiles_y = rdo::ceil_div(H, kTile), tiles_x = rdo::ceil_div(W, kTile);
    const int64_t grid = (int64_t)B * tiles_y * tiles_x;                        // <= B H W
    p.x = x;
    p.H = H;
    p.W = W;
    p.N = N;
    p.nbN = N / kBlock;
    p.cb = N / (2 * kBlock);
    p.strideX = lds_row_dwords(p.nbN, p.fa.bits);
    p.strideH = lds_row_dwords(p.cb, p.fa.bits);
    p.tiles_x = tiles_x;
    p.tiles_y = tiles_y;
    p.w1 = static_cast<const uint32_t*>(w1);
    p.w2 = static_cast<const uint32_t*>(w2);
    p.w3 = static_cast<const uint32_t*>(w3);
    p.s1 = w1_scales;
    p.s2 = w2_scales;
    p.s3 = w3_scales;
    p.b1 = b1;
    p.b2 = b2;
    p.b3 = b3;
    p.out = out;
    p.branch = branch;
    p.xp = static_cast<uint32_t*>(xp);
    p.h1 = static_cast<uint32_t*>(h1);
    p.h2 = static_cast<uint32_t*>(h2);
    p.xs = xp_scales;
    p.h1s = h1_scales;
    p.h2s = h2_scales;
    const ResUnitKernel kern = kResUnit[hw_format(act_format)][hw_format(w_format)];
    const size_t lds = resunit_lds(N, p.fa.bits);                               // + kStaticLds <= 65 536 for every N served
    const double pixels = (double)B * H * W, half = N / 2.0;
    const double abytes = 4.0 * p.fa.bits + 1.0;                                // of one packed block with its scale byte
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, s, p);
            return rdo::check_launch("mx_residual_unit");
        },
        stream, "mx_residual_unit", 2.0 * pixels * half * (2.0 * N + 9.0 * half),
        pixels * N * 4.0 * (3.0 + (branch ? 1.0 : 0.0)) + (2.0 * p.nbN * half + 9.0 * p.cb * half) * (4.0 * fw.bits + 1.0) +
            pixels * ((xp ? p.nbN : 0) + (h1 ? p.cb : 0) + (h2 ? p.cb : 0)) * abytes);
}

}  // extern "C"
