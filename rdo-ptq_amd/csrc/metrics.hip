// MS-SSIM building blocks for the evaluation path (reference: `ms_ssim` of pytorch_msssim, test_datasets.py:25-27,
// losses/losses.py:27,54): one scale of SSIM / contrast-structure statistics with an 11-tap separable Gaussian window (valid
// padding) and the 2x2 average pooling between scales.  Planes are [planes][H][W] fp32 (NCHW images: planes = B*C).
// A 16 x 16 output tile per workgroup: the 26 x 26 input halo of both images goes to LDS, rows are filtered into five 26 x 16
// LDS planes (mu1, mu2, E[xx], E[yy], E[xy]), then columns; per-plane sums accumulate with one atomic per workgroup.
// Backward (the differentiable `ms-ssim` distortion of losses.RateDistortionLoss): rdo_ssim_level_bwd gives d/dx of
// sum_p g_ssim[p] ssim_mean[p] + g_cs[p] cs_mean[p] -- a 16 x 16 tile of dx per workgroup, statistics recomputed over the tile plus
// a 10-pixel margin, the three adjoint maps a1..a3 in LDS, then the transposed ("full") separable filter; each dx pixel is written
// by exactly one workgroup (no atomics: bit-reproducible).  rdo_avg_pool2_bwd is the gather adjoint of rdo_avg_pool2.
#include "rdo_common.h"

namespace {

constexpr int WIN = 11, TILE = 16, HALO = TILE + WIN - 1;

struct SsimArgs {
    const float* x;
    const float* y;
    int planes, H, W;
    float c1, c2;
    float win[WIN];
    float* ssim_sum;   // [planes]
    float* cs_sum;     // [planes]
};

__global__ __launch_bounds__(256) void ssim_level_kernel(SsimArgs a) {
    __shared__ float sx[HALO][HALO + 1], sy[HALO][HALO + 1];
    __shared__ float r[5][HALO][TILE + 1];
    const int Ho = a.H - WIN + 1, Wo = a.W - WIN + 1;
    const int plane = blockIdx.z, h0 = blockIdx.y * TILE, w0 = blockIdx.x * TILE;
    const float* px = a.x + (long)plane * a.H * a.W;
    const float* py = a.y + (long)plane * a.H * a.W;
    for (int e = threadIdx.x; e < HALO * HALO; e += 256) {
        const int i = e / HALO, j = e - i * HALO;
        const int h = h0 + i, w = w0 + j;
        const bool ok = h < a.H && w < a.W;
        sx[i][j] = ok ? px[(long)h * a.W + w] : 0.f;
        sy[i][j] = ok ? py[(long)h * a.W + w] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < HALO * TILE; e += 256) {
        const int i = e / TILE, j = e - i * TILE;
        float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = a.win[k], u = sx[i][j + k], v = sy[i][j + k];
            m1 += g * u; m2 += g * v; xx += g * u * u; yy += g * v * v; xy += g * u * v;
        }
        r[0][i][j] = m1; r[1][i][j] = m2; r[2][i][j] = xx; r[3][i][j] = yy; r[4][i][j] = xy;
    }
    __syncthreads();
    const int i = threadIdx.x / TILE, j = threadIdx.x % TILE;
    float ssim = 0.f, cs = 0.f;
    if (h0 + i < Ho && w0 + j < Wo) {
        float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = a.win[k];
            m1 += g * r[0][i + k][j]; m2 += g * r[1][i + k][j]; xx += g * r[2][i + k][j]; yy += g * r[3][i + k][j];
            xy += g * r[4][i + k][j];
        }
        const float s11 = xx - m1 * m1, s22 = yy - m2 * m2, s12 = xy - m1 * m2;
        cs = (2.f * s12 + a.c2) / (s11 + s22 + a.c2);
        ssim = ((2.f * m1 * m2 + a.c1) / (m1 * m1 + m2 * m2 + a.c1)) * cs;
    }
    float sum[2] = {ssim, cs};
    rdo::block_sum(sum);
    if (threadIdx.x == 0) {
        const float inv = 1.0f / ((float)Ho * (float)Wo);
        atomicAdd(a.ssim_sum + plane, sum[0] * inv);
        atomicAdd(a.cs_sum + plane, sum[1] * inv);
    }
}

// F.avg_pool2d(x, 2, padding=(H%2, W%2)) with count_include_pad=True: out[h][w] = sum of the 2x2 window (zeros outside) / 4
__global__ __launch_bounds__(256) void avg_pool2_kernel(const float* x, int planes, int H, int W, int ph, int pw, int Ho, int Wo, float* out) {
    const long total = (long)planes * Ho * Wo;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int w = (int)(t % Wo);
        const int h = (int)((t / Wo) % Ho);
        const long p = t / ((long)Wo * Ho);
        float acc = 0.f;
#pragma unroll
        for (int dh = 0; dh < 2; ++dh)
#pragma unroll
            for (int dw = 0; dw < 2; ++dw) {
                const int hi = 2 * h - ph + dh, wi = 2 * w - pw + dw;
                if ((unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W) acc += x[(p * H + hi) * W + wi];
            }
        out[t] = 0.25f * acc;
    }
}

// dx of L = sum_p g_ssim[p] mean_q ssim_q + g_cs[p] mean_q cs_q.  Per valid q (N = Ho Wo), A = 2 mx my + C1, B = mx^2 + my^2 + C1,
// Cn = 2 sxy + C2, D = sxx + syy + C2, cs = Cn / D, ssim = (A / B) cs:
//   dL/dcs = (g_cs + g_ssim A/B) / N,  dL/dsxy = 2 dL/dcs / D,  dL/dsxx = -dL/dcs Cn / D^2,  dL/dmx|direct = g_ssim cs 2 (my - mx A/B) / B / N
// and, with sxx = G*(xx) - mx^2, sxy = G*(xy) - mx my, mx = G*x:
//   a1 = dL/dmx|direct - 2 mx a2 - my a3,  a2 = dL/dsxx,  a3 = dL/dsxy,   dx = G'*a1 + 2 x G'*a2 + y G'*a3
// (G' = the transposed, full-padding filter; the window is symmetric, so G'*a at p = sum_k g[k] a[p - 10 + k]).  The tile's
// statistics are taken about one value c of x in the tile (x - c, y - c: the variances do not change, the means are shifted
// back), which keeps E[xx] - mx^2 out of catastrophic cancellation on the smooth coarse scales; a1 and the final combination use
// the shifted values consistently (x - c, y - c, mx - c, my - c): the same gradient for a window that sums to 1 (the fp32 window
// does up to its rounding, a ~1e-7 relative effect).
constexpr int MARGIN = WIN - 1, IN = TILE + 2 * MARGIN;   // input rows / cols a 16 x 16 tile of dx depends on: 36

struct SsimBwdArgs {
    const float* x;
    const float* y;
    int planes, H, W;
    float c1, c2;
    float win[WIN];
    const float* g_ssim;   // [planes]
    const float* g_cs;     // [planes]
    float* dx;             // [planes][H][W]
};

__global__ __launch_bounds__(256) void ssim_level_bwd_kernel(SsimBwdArgs a) {
    __shared__ float sx[IN][IN + 1], sy[IN][IN + 1];
    __shared__ float r[5][IN][HALO + 1];          // row-filtered statistics; reused for the row-filtered adjoints
    __shared__ float am[3][HALO][HALO + 1];       // a1, a2, a3 at the statistics positions (0 outside the valid region)
    float (*t)[HALO][TILE + 1] = reinterpret_cast<float (*)[HALO][TILE + 1]>(&r[0][0][0]);   // [3][HALO][TILE + 1] <= r
    static_assert(3 * HALO * (TILE + 1) <= 5 * IN * (HALO + 1), "adjoint row buffer must fit in the statistics buffer");
    const int Ho = a.H - WIN + 1, Wo = a.W - WIN + 1;
    const int plane = blockIdx.z, h0 = blockIdx.y * TILE, w0 = blockIdx.x * TILE;
    const long off = (long)plane * a.H * a.W;
    const float* px = a.x + off;
    const float* py = a.y + off;
    const float c = px[(long)h0 * a.W + w0];        // h0 < H, w0 < W by the grid
    for (int e = threadIdx.x; e < IN * IN; e += 256) {
        const int i = e / IN, j = e - i * IN;
        const int h = h0 - MARGIN + i, w = w0 - MARGIN + j;
        const bool ok = (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W;
        sx[i][j] = ok ? px[(long)h * a.W + w] - c : 0.f;
        sy[i][j] = ok ? py[(long)h * a.W + w] - c : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < IN * HALO; e += 256) {
        const int i = e / HALO, j = e - i * HALO;
        float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = a.win[k], u = sx[i][j + k], v = sy[i][j + k];
            m1 += g * u; m2 += g * v; xx += g * u * u; yy += g * v * v; xy += g * u * v;
        }
        r[0][i][j] = m1; r[1][i][j] = m2; r[2][i][j] = xx; r[3][i][j] = yy; r[4][i][j] = xy;
    }
    __syncthreads();
    const float inv = 1.0f / ((float)Ho * (float)Wo);
    const float gs = a.g_ssim[plane] * inv, gc = a.g_cs[plane] * inv;
    for (int e = threadIdx.x; e < HALO * HALO; e += 256) {
        const int i = e / HALO, j = e - i * HALO;
        const int qh = h0 - MARGIN + i, qw = w0 - MARGIN + j;
        float a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (qh >= 0 && qw >= 0 && qh < Ho && qw < Wo) {
            float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float g = a.win[k];
                m1 += g * r[0][i + k][j]; m2 += g * r[1][i + k][j]; xx += g * r[2][i + k][j]; yy += g * r[3][i + k][j];
                xy += g * r[4][i + k][j];
            }
            const float s11 = xx - m1 * m1, s22 = yy - m2 * m2, s12 = xy - m1 * m2;
            const float mx = m1 + c, my = m2 + c;
            const float A = 2.f * mx * my + a.c1, B = mx * mx + my * my + a.c1;
            const float Cn = 2.f * s12 + a.c2, D = s11 + s22 + a.c2;
            const float cs = Cn / D, l = A / B;
            const float dcs = gc + gs * l;
            a2 = -dcs * cs / D;
            a3 = 2.f * dcs / D;
            const float dmx = gs * cs * 2.f * (my - mx * l) / B;
            a1 = dmx - 2.f * m1 * a2 - m2 * a3;
        }
        am[0][i][j] = a1; am[1][i][j] = a2; am[2][i][j] = a3;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < HALO * TILE; e += 256) {
        const int i = e / TILE, j = e - i * TILE;
        float u1 = 0.f, u2 = 0.f, u3 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = a.win[k];
            u1 += g * am[0][i][j + k]; u2 += g * am[1][i][j + k]; u3 += g * am[2][i][j + k];
        }
        t[0][i][j] = u1; t[1][i][j] = u2; t[2][i][j] = u3;
    }
    __syncthreads();
    const int i = threadIdx.x / TILE, j = threadIdx.x % TILE;
    const int h = h0 + i, w = w0 + j;
    if (h < a.H && w < a.W) {
        float u1 = 0.f, u2 = 0.f, u3 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = a.win[k];
            u1 += g * t[0][i + k][j]; u2 += g * t[1][i + k][j]; u3 += g * t[2][i + k][j];
        }
        a.dx[off + (long)h * a.W + w] = u1 + 2.f * sx[i + MARGIN][j + MARGIN] * u2 + sy[i + MARGIN][j + MARGIN] * u3;
    }
}

// adjoint of avg_pool2_kernel: every input pixel lies in exactly one 2 x 2 window (stride 2): dx = g_out[window] / 4
__global__ __launch_bounds__(256) void avg_pool2_bwd_kernel(const float* g, int planes, int H, int W, int ph, int pw, int Ho, int Wo, float* dx) {
    const long total = (long)planes * H * W;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int w = (int)(t % W);
        const int h = (int)((t / W) % H);
        const long p = t / ((long)W * H);
        dx[t] = 0.25f * g[(p * Ho + (h + ph) / 2) * Wo + (w + pw) / 2];
    }
}

}  // namespace

extern "C" {

int rdo_ssim_level(const float* x, const float* y, int32_t planes, int32_t H, int32_t W, const float* window11, float c1, float c2,
                   float* ssim_sum, float* cs_sum, void* stream) {
    RDO_REQUIRE(x && y && window11 && ssim_sum && cs_sum && planes > 0, "rdo_ssim_level: bad argument");
    RDO_REQUIRE(H >= WIN && W >= WIN, "rdo_ssim_level: the %dx%d plane is smaller than the 11-tap window", H, W);
    SsimArgs a;
    a.x = x; a.y = y; a.planes = planes; a.H = H; a.W = W; a.c1 = c1; a.c2 = c2; a.ssim_sum = ssim_sum; a.cs_sum = cs_sum;
    for (int k = 0; k < WIN; ++k) a.win[k] = window11[k];       // host pointer: 11 floats copied into the launch arguments
    const int Ho = H - WIN + 1, Wo = W - WIN + 1;
    return rdo::dispatch(
        [=](hipStream_t s) {
            if (hipMemsetAsync(a.ssim_sum, 0, sizeof(float) * a.planes, s) != hipSuccess ||
                hipMemsetAsync(a.cs_sum, 0, sizeof(float) * a.planes, s) != hipSuccess)
                return rdo::set_error(RDO_EHIP, "rdo_ssim_level: memset failed");
            dim3 grid((unsigned)rdo::ceil_div(Wo, TILE), (unsigned)rdo::ceil_div(Ho, TILE), (unsigned)a.planes);
            hipLaunchKernelGGL(ssim_level_kernel, grid, dim3(256), 0, s, a);
            return rdo::check_launch("ssim_level");
        },
        stream, "ssim_level", 0.0, 8.0 * planes * H * W);
}

int rdo_avg_pool2(const float* x, int32_t planes, int32_t H, int32_t W, float* out, void* stream) {
    RDO_REQUIRE(x && out && planes > 0 && H > 0 && W > 0, "rdo_avg_pool2: bad argument");
    const int ph = H % 2, pw = W % 2;
    const int Ho = (H + 2 * ph - 2) / 2 + 1, Wo = (W + 2 * pw - 2) / 2 + 1;
    return rdo::dispatch(
        [=](hipStream_t s) {
            long g = rdo::ceil_div((long)planes * Ho * Wo, 256);
            hipLaunchKernelGGL(avg_pool2_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, x, planes, H, W, ph, pw, Ho, Wo, out);
            return rdo::check_launch("avg_pool2");
        },
        stream, "avg_pool2", 0.0, 5.0 * planes * H * W);
}

int rdo_ssim_level_bwd(const float* x, const float* y, int32_t planes, int32_t H, int32_t W, const float* window11, float c1, float c2,
                       const float* g_ssim, const float* g_cs, float* dx, void* stream) {
    RDO_REQUIRE(x && y && window11 && g_ssim && g_cs && dx && planes > 0, "rdo_ssim_level_bwd: bad argument");
    RDO_REQUIRE(H >= WIN && W >= WIN, "rdo_ssim_level_bwd: the %dx%d plane is smaller than the 11-tap window", H, W);
    SsimBwdArgs a;
    a.x = x; a.y = y; a.planes = planes; a.H = H; a.W = W; a.c1 = c1; a.c2 = c2; a.g_ssim = g_ssim; a.g_cs = g_cs; a.dx = dx;
    for (int k = 0; k < WIN; ++k) a.win[k] = window11[k];       // host pointer, as in rdo_ssim_level
    return rdo::dispatch(
        [=](hipStream_t s) {
            dim3 grid((unsigned)rdo::ceil_div(W, TILE), (unsigned)rdo::ceil_div(H, TILE), (unsigned)a.planes);
            hipLaunchKernelGGL(ssim_level_bwd_kernel, grid, dim3(256), 0, s, a);
            return rdo::check_launch("ssim_level_bwd");
        },
        stream, "ssim_level_bwd", 0.0, 12.0 * planes * H * W);
}

int rdo_avg_pool2_bwd(const float* g_out, int32_t planes, int32_t H, int32_t W, float* dx, void* stream) {
    RDO_REQUIRE(g_out && dx && planes > 0 && H > 0 && W > 0, "rdo_avg_pool2_bwd: bad argument");
    const int ph = H % 2, pw = W % 2;
    const int Ho = (H + 2 * ph - 2) / 2 + 1, Wo = (W + 2 * pw - 2) / 2 + 1;
    return rdo::dispatch(
        [=](hipStream_t s) {
            long g = rdo::ceil_div((long)planes * H * W, 256);
            hipLaunchKernelGGL(avg_pool2_bwd_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, g_out, planes, H, W, ph, pw, Ho, Wo, dx);
            return rdo::check_launch("avg_pool2_bwd");
        },
        stream, "avg_pool2_bwd", 0.0, 5.0 * planes * H * W);
}

}  // extern "C"
