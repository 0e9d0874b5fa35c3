// The backward of the two products of the activation-quantised window attention (include/rdo_ptq_attnq.h).  That attention runs in
// pieces -- probabilities (swin.hip, forward without the P V product), quantiser, P V (win_attn_pv_kernel), quantiser -- so that the
// quantiser object alone decides how a site is quantised; the quantisers differentiate themselves (actquant.hip), and the two kernels
// here are what lies between them.  Both take the probabilities as GIVEN float32 data: no softmax is recomputed, no mask is applied.
//
// One 4-wave workgroup per (window, head), plain grid windows x heads with the head fastest: the workgroups that share the heads-last
// cache lines of a probs row run together.  Operands are zero-padded to 64 rows in LDS with the odd row strides of swin.hip; the
// products run on v_mfma_f32_32x32x2_f32 (exact fp32 products) through swin.hip's `tile_gemm`, wave w owning the 32 x 32 tile
// (w >> 1, w & 1) of a product; a wave whose tile lies wholly outside the matrix skips it.  One code path for every (N, hd): all global
// accesses are 4 bytes wide (no alignment beyond that is asked of a pointer), no persistent loop, no prefetch -- the launches are
// bound by reading and writing the [windows][N][N][heads] tensors.  No atomics; every sum has a fixed order.
//   pv_bwd:     dP = dO V^T (every pair written, also those the shift mask separates);  dV = Pq^T dO;  zeros for dQ, dK
//   probs_bwd:  D_i = sum_j p_ij g_ij (a row's four threads: 16 terms each, then two xor-shuffles);  dS = p (g - D);
//               dQ = scale * (dS K);  dK = dS^T (scale Q);  zeros for dV
#include "attn_device.h"
#include "../../include/rdo_ptq_attnq.h"

namespace {

__device__ __forceinline__ void zero_lds(float* p, int n) {
    for (int e = threadIdx.x; e < n; e += 256) p[e] = 0.f;
}

// rows [N][hd] of this (window, head) out of a pixel-ordered tensor into an LDS image of row stride hs
__device__ __forceinline__ void load_rows(const AttnGeom& g, const float* src, int row_stride, int ch0, const int* pix, float* dst, float mul) {
    for (int e = threadIdx.x; e < g.N * g.hd; e += 256) {
        const int tok = e / g.hd, d = e - tok * g.hd;
        dst[tok * g.hs + d] = mul * src[(long)pix[tok] * row_stride + ch0 + d];
    }
}

// zeros for the channels [ch0, ch0 + hd) of the window's tokens: the thirds of dqkv a kernel does not own
__device__ __forceinline__ void zero_rows(const AttnGeom& g, float* dst, int ch0, const int* pix) {
    for (int e = threadIdx.x; e < g.N * g.hd; e += 256) {
        const int tok = e / g.hd, d = e - tok * g.hd;
        dst[(long)pix[tok] * (3 * g.C) + ch0 + d] = 0.f;
    }
}

// the wave's tile of a [N][hd] result into the channels [ch0, ch0 + hd) of dqkv (accumulator layout of `tile_to_lds`)
__device__ __forceinline__ void tile_to_rows(const AttnGeom& g, const f32x16& acc, float* dqkv, int ch0, const int* pix, int ti, int tj, float mul) {
    const int l = threadIdx.x & 63, lr = l & 31, lk = l >> 5;
    const int d = 32 * tj + lr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int tok = 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (tok < g.N && d < g.hd) dqkv[(long)pix[tok] * (3 * g.C) + ch0 + d] = mul * acc[r];
    }
}

__global__ __launch_bounds__(256) void attn_pv_bwd_kernel(const float* qkv, const float* probs_q, const float* dout, AttnGeom g,
                                                          float* dprobs, float* dqkv) {
    extern __shared__ float lds[];
    float* V = lds;                           // [64][hs]
    float* dO = V + 64 * g.hs;                // [64][hs]
    float* P = dO + 64 * g.hs;                // [64][65]
    __shared__ int pix[NMAX];
    const int win = blockIdx.x / g.heads, head = blockIdx.x - win * g.heads;
    const int w = threadIdx.x >> 6, ti = w >> 1, tj = w & 1;
    const int lr = threadIdx.x & 31, lk = (threadIdx.x & 63) >> 5;
    zero_lds(lds, 2 * 64 * g.hs + 64 * SS);
    if (threadIdx.x < g.N) pix[threadIdx.x] = token_pixel(g, win, threadIdx.x);
    __syncthreads();
    load_rows(g, qkv, 3 * g.C, 2 * g.C + head * g.hd, pix, V, 1.f);
    load_rows(g, dout, g.C, head * g.hd, pix, dO, 1.f);
    const long pbase = (long)win * g.N * g.N;
    for (int e = threadIdx.x; e < g.N * g.N; e += 256) {
        const int i = e / g.N, j = e - i * g.N;
        P[i * SS + j] = probs_q[(pbase + e) * g.heads + head];
    }
    zero_rows(g, dqkv, head * g.hd, pix);
    zero_rows(g, dqkv, g.C + head * g.hd, pix);
    __syncthreads();
    const int hk = (g.hd + 1) & ~1, nk = (g.N + 1) & ~1;           // reduction lengths, whole k pairs (the odd one out reads a zero)
    if (32 * ti < g.N && 32 * tj < g.N) {                          // dP = dO V^T
        const f32x16 acc = tile_gemm<false, true>(dO, g.hs, V, g.hs, ti, tj, hk, 0);
        const int j = 32 * tj + lr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * ti + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (i < g.N && j < g.N) dprobs[(pbase + (long)i * g.N + j) * g.heads + head] = acc[r];
        }
    }
    if (32 * ti < g.N && 32 * tj < g.hd) {                         // dV = Pq^T dO
        const f32x16 acc = tile_gemm<true, false>(P, SS, dO, g.hs, ti, tj, nk, g.hd);
        tile_to_rows(g, acc, dqkv, 2 * g.C + head * g.hd, pix, ti, tj, 1.f);
    }
}

__global__ __launch_bounds__(256) void attn_probs_bwd_kernel(const float* qkv, const float* probs, const float* dprobs, AttnGeom g,
                                                             float* dqkv) {
    extern __shared__ float lds[];
    float* Q = lds;                           // [64][hs], pre-scaled
    float* K = Q + 64 * g.hs;                 // [64][hs]
    float* dS = K + 64 * g.hs;                // [64][65]
    __shared__ int pix[NMAX];
    const int win = blockIdx.x / g.heads, head = blockIdx.x - win * g.heads;
    const int w = threadIdx.x >> 6, ti = w >> 1, tj = w & 1;
    zero_lds(lds, 2 * 64 * g.hs + 64 * SS);
    if (threadIdx.x < g.N) pix[threadIdx.x] = token_pixel(g, win, threadIdx.x);
    __syncthreads();
    load_rows(g, qkv, 3 * g.C, head * g.hd, pix, Q, g.scale);
    load_rows(g, qkv, 3 * g.C, g.C + head * g.hd, pix, K, 1.f);
    zero_rows(g, dqkv, 2 * g.C + head * g.hd, pix);
    {
        // row i = thread / 4, columns j = (thread & 3) + 4 k, k < 16 (the layout of swin.hip's softmax rows): the probabilities and their
        // gradients go from global memory to registers, dS to LDS
        const int i = threadIdx.x >> 2, part = threadIdx.x & 3;
        const long rbase = ((long)win * g.N + i) * g.N;
        float p[16], gg[16];
        float D = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int j = part + 4 * k;
            const bool ok = i < g.N && j < g.N;
            p[k] = ok ? probs[(rbase + j) * g.heads + head] : 0.f;
            gg[k] = ok ? dprobs[(rbase + j) * g.heads + head] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) D += p[k] * gg[k];
        D += __shfl_xor(D, 1, 64);
        D += __shfl_xor(D, 2, 64);
        if (i < g.N) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int j = part + 4 * k;
                if (j < g.N) dS[i * SS + j] = p[k] * (gg[k] - D);
            }
        }
    }
    __syncthreads();
    const int nk = (g.N + 1) & ~1;
    if (32 * ti < g.N && 32 * tj < g.hd) {
        const f32x16 dq = tile_gemm<false, false>(dS, SS, K, g.hs, ti, tj, nk, g.hd);      // dQ = scale * (dS K)
        tile_to_rows(g, dq, dqkv, head * g.hd, pix, ti, tj, g.scale);
        const f32x16 dk = tile_gemm<true, false>(dS, SS, Q, g.hs, ti, tj, nk, g.hd);       // dK = dS^T (scale Q)
        tile_to_rows(g, dk, dqkv, g.C + head * g.hd, pix, ti, tj, 1.f);
    }
}

struct Span {
    const float* p;
    size_t n;
};
inline bool overlap(const Span& a, const Span& b) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a0 < b0 + b.n * sizeof(float) && b0 < a0 + a.n * sizeof(float);
}

// what both entries check and derive: geometry, the operand sizes in floats, the grid
struct Launch {
    AttnGeom g;
    size_t qkv, out, probs, lds;
    unsigned grid;
};
int make_launch(const rdo_attn_desc* d, Launch* L, const char* who) {
    if (int rc = make_geom(d, &L->g, who)) return rc;
    const AttnGeom& g = L->g;
    const size_t pixels = (size_t)g.B * g.H * g.W;
    const size_t items = pixels / g.N * g.heads;
    RDO_REQUIRE(items <= 0x7fffffffu, "%s: %zu (window, head) pairs are more than a grid holds", who, items);
    L->qkv = pixels * 3 * g.C;
    L->out = pixels * g.C;
    L->probs = pixels * g.N * g.heads;
    L->lds = ((size_t)2 * 64 * g.hs + (size_t)64 * SS) * sizeof(float);      // <= 49 920 bytes at hd = 64
    L->grid = (unsigned)items;
    return RDO_OK;
}

}  // namespace

extern "C" {

int rdo_window_attention_pv_bwd(const rdo_attn_desc* d, const float* qkv, const float* probs_q, const float* dout, float* dprobs,
                                float* dqkv, void* stream) {
    const char* who = "rdo_window_attention_pv_bwd";
    Launch L;
    if (int rc = make_launch(d, &L, who)) return rc;
    RDO_REQUIRE(qkv && probs_q && dout && dprobs && dqkv, "%s: null pointer", who);
    const Span in[3] = {{qkv, L.qkv}, {probs_q, L.probs}, {dout, L.out}}, o1 = {dprobs, L.probs}, o2 = {dqkv, L.qkv};
    for (const Span& s : in) RDO_REQUIRE(!overlap(o1, s) && !overlap(o2, s), "%s: an output overlaps an input (dqkv over qkv, dprobs over probs_q, ...)", who);
    RDO_REQUIRE(!overlap(o1, o2), "%s: dprobs and dqkv overlap", who);
    const AttnGeom g = L.g;
    const size_t lds = L.lds;
    const unsigned grid = L.grid;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(attn_pv_bwd_kernel, dim3(grid), dim3(256), lds, s, qkv, probs_q, dout, g, dprobs, dqkv);
            return rdo::check_launch("window_attention_pv_bwd");
        },
        stream, "window_attention_pv_bwd", 4.0 * grid * (double)g.N * g.N * g.hd, 4.0 * (2.0 * L.probs + 2.0 * L.qkv / 3.0 + L.qkv));
}

int rdo_window_attention_probs_bwd(const rdo_attn_desc* d, const float* qkv, const float* probs, const float* dprobs, float* dqkv,
                                   void* stream) {
    const char* who = "rdo_window_attention_probs_bwd";
    Launch L;
    if (int rc = make_launch(d, &L, who)) return rc;
    RDO_REQUIRE(qkv && probs && dprobs && dqkv, "%s: null pointer", who);
    const Span in[3] = {{qkv, L.qkv}, {probs, L.probs}, {dprobs, L.probs}}, o = {dqkv, L.qkv};
    for (const Span& s : in) RDO_REQUIRE(!overlap(o, s), "%s: dqkv overlaps an input (qkv, probs or dprobs)", who);
    const AttnGeom g = L.g;
    const size_t lds = L.lds;
    const unsigned grid = L.grid;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(attn_probs_bwd_kernel, dim3(grid), dim3(256), lds, s, qkv, probs, dprobs, g, dqkv);
            return rdo::check_launch("window_attention_probs_bwd");
        },
        stream, "window_attention_probs_bwd", 4.0 * grid * (double)g.N * g.N * g.hd, 4.0 * (2.0 * L.probs + 2.0 * L.qkv / 3.0 + L.qkv));
}

}  // extern "C"
