// What the window attention kernels of swin.hip and attn_tape.hip share: the geometry of a launch and its host-side check, the token ->
// pixel map (the header comment of swin.hip states the token order) and the 32 x 32 fp32 MFMA tile product on LDS images.
#pragma once
#include "rdo_common.h"

namespace {

constexpr int NMAX = 64;

struct AttnGeom {
    int B, H, W, C, heads, ws, shift, N, hd, hs;   // hs: LDS row stride (odd)
    float scale;
#ifdef RDO_DIAG
    int diag;                                      // ablation bits (diagnostic build, RDO_ATTN_DIAG): 1 no stores, 2 no products, 4 no loads, 8 no softmax
#endif
};
#ifdef RDO_DIAG
#define ATTN_ABL(bit) (g.diag & (bit))
#else
#define ATTN_ABL(bit) false
#endif

__device__ __forceinline__ int token_pixel(const AttnGeom& g, int win, int tok) {
    const int nww = g.W / g.ws, nwh = g.H / g.ws;
    const int b = win / (nwh * nww);
    const int r = win - b * (nwh * nww);
    const int wh = r / nww, ww = r - wh * nww;
    const int ih = tok / g.ws, iw = tok - ih * g.ws;
    int h = wh * g.ws + ih + g.shift, w = ww * g.ws + iw + g.shift;
    if (h >= g.H) h -= g.H;
    if (w >= g.W) w -= g.W;
    return (b * g.H + h) * g.W + w;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int SS = 65;                             // row stride of a [64][64] score-shaped LDS image

// C[i][j] += sum_k A(i,k) * B(k,j) for the wave's tile; TA: A stored [k][i]; TB: B stored [j][k] (else [k][j]).
// bcols: valid columns of B when B is [k][j] (reads past it are replaced by 0 so the tile may overhang the matrix)
template <bool TA, bool TB>
__device__ __forceinline__ f32x16 tile_gemm(const float* A, int lda, const float* B, int ldb, int ti, int tj, int K, int bcols) {
    const int l = threadIdx.x & 63, lr = l & 31, lk = l >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int ai = 32 * ti + lr, bj = 32 * tj + lr;
    for (int s = 0; s < K; s += 2) {
        const int k = s + lk;
        const float a = TA ? A[k * lda + ai] : A[ai * lda + k];
        float b;
        if (TB) b = B[bj * ldb + k];
        else b = bj < bcols ? B[k * ldb + bj] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    return acc;
}

__device__ __forceinline__ void tile_to_lds(const f32x16& acc, float* D, int ldd, int ti, int tj) {
    const int l = threadIdx.x & 63, lr = l & 31, lk = l >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) D[(32 * ti + (r & 3) + 8 * (r >> 2) + 4 * lk) * ldd + 32 * tj + lr] = acc[r];
}

int make_geom(const rdo_attn_desc* d, AttnGeom* g, const char* who) {
    RDO_REQUIRE(d != nullptr, "%s: null descriptor", who);
    RDO_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->heads > 0 && d->window > 0, "%s: bad geometry", who);
    RDO_REQUIRE(d->C % d->heads == 0, "%s: C=%d not divisible by heads=%d", who, d->C, d->heads);
    RDO_REQUIRE(d->H % d->window == 0 && d->W % d->window == 0, "%s: %dx%d not divisible by window %d", who, d->H, d->W, d->window);
    RDO_REQUIRE(d->window * d->window <= NMAX, "%s: windows of more than %d tokens are not supported", who, NMAX);
    RDO_REQUIRE(d->shift >= 0 && d->shift < d->window, "%s: shift must be in [0, window)", who);
    g->B = d->B; g->H = d->H; g->W = d->W; g->C = d->C; g->heads = d->heads; g->ws = d->window; g->shift = d->shift;
    g->N = d->window * d->window;
    g->hd = d->C / d->heads;
    g->hs = (g->hd + 1) | 1;                 // odd row stride; an odd head dim gets the zero column its last k pair reads (hd + 2)
    RDO_REQUIRE(g->hd <= 64, "%s: head dims above 64 are not supported", who);
    g->scale = d->scale;
#ifdef RDO_DIAG
    { const char* e = getenv("RDO_ATTN_DIAG"); g->diag = e ? atoi(e) : 0; }
#endif
    return RDO_OK;
}

}  // namespace
