// GDN / IGDN block of a reconstruction unit, forward and backward, in ONE launch (quant_layer.py:142-154, layer_opt.py:133,150):
//
//   norm = beta' + gamma' . c^2                     rdo_linear_h2(square_input)            c [M][192] fp32, NHWC
//   out  = c * norm^(-+1/2) (+ residual)            rdo_loss_gdn_bwd
//   g    = dL/dout, loss, t = dL/dnorm
//   acc  = t . gamma'                               rdo_linear_h2 on the planes of gamma'^T
//   dx   = g * norm^(-+1/2) + 2 c acc               rdo_gdn_bwd_dx_h2 (fp32 and / or H2 planes)
//
// The four launches pass `norm` and `acc` through HBM and re-read c, g and t: 13 passes over an [M][192] fp32 tensor.  Here a workgroup
// keeps the 64-token x 192-channel panel on chip between the steps: reads c, residual, target; writes g, t, dx (6 passes; c is read
// again from L2 in accumulator order).
//
// Arithmetic: the device functions of the chain, called in the chain's order (gdn_device.h) -- the per-token power-of-two scale and
// fp16 split of rdo_linear_h2, its K-step and product order (w_lo x_hi, w_hi x_lo, w_hi x_hi per 32-wide K step), the element-wise
// formulas of fused_tail.hip under -ffp-contract=off: every output equals the chain's bit for bit; the loss partial sums are added in
// another order (float atomics, as before).
//
// Structure: one 512-thread workgroup per CU, 8 waves = 4 channel groups x 2 token halves (the wave grid of linear_h2w_kernel): a wave
// owns channels [48 cg, 48 cg + 48) of 32 tokens (3 x 2 accumulator tiles of 16 x 16; a lane holds four consecutive channels of one
// token per tile).  The panel -- c^2, then t -- lives in LDS as fp16 planes; BOTH weights stream from L2 in fragment order, one K step
// ahead, as in linear_h2_kernel (two stationary weights are 288 registers: they do not fit beside the rest at two waves per SIMD).
// Between the GEMMs a lane keeps, per element, p = g norm^(-+1/2) and q = 2 c (gdn_dx_pre): 48 registers beside 24 accumulators and
// the 64 of the K loop -- no scratch.  A workgroup walks tiles blockIdx.x, + gridDim.x, ...
#include "rdo_common.h"
#include "gather_body.h"
#include "gdn_device.h"
#include "../../include/rdo_ptq_gdn.h"
#include "../../include/rdo_ptq_subpel.h"

namespace {

using namespace rdo::gdn;
using rdo::gq::H2Out;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16;

constexpr int BM = 64;                     // tokens per tile
constexpr int CH = 192;                    // channels
constexpr int KS = CH / 32;                // K steps of a GEMM
constexpr int NBLK = CH / 16;              // 16-channel blocks of the outputs
constexpr int PLANE = (CH / 16) * BM * 32; // bytes per plane of the panel: 24 KiB
constexpr int LDS_BYTES = 2 * PLANE + BM * 4 + 4 * BM * 4 + 8 * 4;   // + 1 / scale of c^2 per token, the channel groups' partial maxima of t, the waves' loss sums

struct GdnArgs {
    const float* c;                // [M][192]
    const u16* wf;                 // planes of gamma' (rdo_split_h2_linear)
    const u16* wb;                 // planes of gamma'^T
    const float* beta;             // [192]
    const float* res;              // [M][192] or null
    const float* tgt;              // target cache [rows][per_image]
    const int32_t* idx;            // [iters][B]
    const int32_t* iter;
    int32_t* pub;                  // rdo_iter_bind_publish
    int B, ntiles, inverse;
    long per_image, M;
    float inv_wscale, inv_npix, coef;
    float* out;                    // nullable
    float* gout;                   // nullable
    float* t;
    float* dx;                     // nullable
    H2Out dxp;                     // p nullable
    float* loss_out;
    H2Out gp;                      // rdo_gdn_fwd_bwd_px: dL/dout as planes of [B][H/2][W/2][4 * 192] in unshuffle order (p nullable)
    int W, HW, Mq;                 // ... of tokens that are the pixels of [B][H][W]; Mq = M / 4 pixels of the half-size grid
};

__device__ __forceinline__ const f32x4& ldq(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void stq(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }

// INV: IGDN; RES: a residual is added to the output; PX: dL/dout leaves as planes in unshuffle order (gp) -- an instantiation of its own
template <bool INV, bool RES, bool PX = false>
__global__ __launch_bounds__(512, 2) void gdn_fwd_bwd_kernel(GdnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* scl = reinterpret_cast<float*>(smem + 2 * PLANE);          // [BM]: 1 / scale of the token's c^2
    float* wmax = scl + BM;                                           // [4][BM]: largest |t| of the token over a channel group's 48 channels
    float* wsum = wmax + 4 * BM;                                      // [8]: the waves' loss sums
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = wave & 3, th = wave >> 2;
    const int l16 = lane & 15, kg = lane >> 4;
    const int it = *a.iter;
    const float gs = a.coef * 2.f * a.inv_npix;
    const long ppi = a.per_image / CH;
    const int ch0 = 48 * cg + 4 * kg;                                 // the lane's channels: ch0 + 16 i .. + 3
    // Addresses are a UNIFORM base (tile, token tile j, weight fragment: scalar registers) plus one 32-bit lane offset: written with the
    // whole offset per lane, the tile loop's invariant parts -- a 64-bit address per fragment and per (j, tensor) -- are hoisted out of
    // the loop and spilled
    const unsigned lane_e = (unsigned)((32 * th + l16) * CH + ch0);   // element of (token 32 th + l16, channel ch0) inside the tile
    float lsum = 0.f;
    int bad = 0;

    // weight fragments: plane p, K step ks, 16-channel block b -> 1 KiB at ((p * KS + ks) * NBLK + b) * 512 halfs; lane -> 16 bytes
    // (buffer loads: the fragment's offset rides in a scalar register, the lane's 16 bytes in ONE vector register for all 72 fragments.
    //  As global loads each fragment gets a 64-bit vector address, invariant in the tile loop: hoisted out of it, and spilled)
    const auto rs_f = __builtin_amdgcn_make_buffer_rsrc(const_cast<u16*>(a.wf), 0, 2 * CH * CH * 2, 0x00020000);
    const auto rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<u16*>(a.wb), 0, 2 * CH * CH * 2, 0x00020000);
    auto load_w = [&](f16x8 (&fw)[2][3], const decltype(rs_f)& planes, int ks) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int i = 0; i < 3; ++i)
                fw[p][i] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(planes, (unsigned)lane * 16u,
                                                                                           ((p * KS + ks) * NBLK + cg * 3 + i) * 1024, 0));
    };
    const int fx_lane = (kg >> 1) * (BM * 32) + (32 * th + l16) * 32 + (kg & 1) * 16;
    // acc = W . panel: the K loop of linear_h2_kernel.  The barrier in front publishes the panel (the first fragments are in flight across it)
    auto gemm = [&](const decltype(rs_f)& planes, f32x4 (&acc)[3][2]) {
        f16x8 fw[2][2][3];
        load_w(fw[0], planes, 0);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + 1 < KS) load_w(fw[(ks + 1) & 1], planes, ks + 1);      // a whole step ahead of their first use
            __builtin_amdgcn_sched_barrier(0);
            f16x8 fx[2][2];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    fx[p][j] = *reinterpret_cast<const f16x8*>(smem + p * PLANE + (2 * ks) * (BM * 32) + j * (16 * 32) + fx_lane);
            const int c = ks & 1;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[c][1][i], fx[0][j], acc[i][j], 0, 0, 0);    // w_lo x_hi
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[c][0][i], fx[1][j], acc[i][j], 0, 0, 0);    // w_hi x_lo
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[c][0][i], fx[0][j], acc[i][j], 0, 0, 0);    // w_hi x_hi
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    f32x4 bq[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) bq[i] = ldq(a.beta + ch0 + 16 * i);

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long m0 = (long)tile * BM;
        // ---- c^2 as planes: 16 lanes per token, three float4 per lane, 32 tokens per pass; all six loads before the first use
        {
            const int row_in_pass = tid >> 4;
            f32x4 v[2][3];
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const float* src = a.c + (m0 + pass * 32) * CH;
#pragma unroll
                for (int k = 0; k < 3; ++k) v[pass][k] = ldq(src + (unsigned)(row_in_pass * CH + 4 * l16) + 64 * k);
            }
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int r = pass * 32 + row_in_pass;
                float amax = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    v[pass][k] *= v[pass][k];
                    amax = fmaxf(amax, amax_quad(v[pass][k]));
                }
                amax = fmaxf(amax, __shfl_xor(amax, 8, 16));
                amax = fmaxf(amax, __shfl_xor(amax, 4, 16));
                amax = fmaxf(amax, __shfl_xor(amax, 2, 16));
                amax = fmaxf(amax, __shfl_xor(amax, 1, 16));
                float sc, inv;
                token_scale(amax, sc, inv);
                if (l16 == 0) scl[r] = inv;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int c4 = l16 + 16 * k;
                    split_quad_store(v[pass][k], sc, smem + (c4 >> 2) * (BM * 32) + r * 32 + (c4 & 3) * 8, PLANE);
                }
            }
        }
        f32x4 acc[3][2];
        gemm(rs_f, acc);                                              // gamma' . c^2
        // ---- norm, the unit's output, loss, g = dL/dout, t = dL/dnorm; p and q for dx
        f32x4 p[3][2], q[3][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int tok = 32 * th + 16 * j + l16;
            const long m = m0 + tok;
            const int b = (int)(m / ppi);
            const long g0 = (m0 + 16 * j) * CH;                       // + lane_e = the lane's first element of token tile j
            const float* yrow = a.tgt + ((long)a.idx[(long)it * a.B + b] - b) * a.per_image + m * CH + ch0;   // the target of that element
            const float f = scl[tok] * a.inv_wscale;
            f32x4 xv[3], yv[3], rv[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {                             // all loads before any store (the stores may alias them as far as the compiler knows)
                xv[i] = ldq(a.c + g0 + lane_e + 16 * i);
                yv[i] = ldq(yrow + 16 * i);
                if (RES) rv[i] = ldq(a.res + g0 + lane_e + 16 * i);
            }
            // PX: token (b, y, x) -> pixel (b, y >> 1, x >> 1) of the half-size grid, its 192 channels behind those of the group's
            // (2 (y & 1) + (x & 1)) predecessors: the lane's quad of block 3 cg + i is a quarter of record 12 group + 3 cg + i
            // (32-bit element offsets: M * 192 < 2^31; the overflow mark is handed over per token tile, so that it does not live
            //  across the GEMMs)
            unsigned ge = 0;
            int bad_g = 0;
            if constexpr (PX) {
                const int rem = (int)m - b * a.HW, y = rem / a.W, x = rem - y * a.W;
                const int m2 = b * (a.HW >> 2) + (y >> 1) * (a.W >> 1) + (x >> 1), grp = ((y & 1) << 1) + (x & 1);
                ge = (unsigned)(((12 * grp + 3 * cg) * a.Mq + m2) * 16 + 4 * kg);
            }
            float tmax = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                f32x4 n = acc[i][j] * f;
                n += bq[i];
                f32x4 o, g, tv;
                lsum += loss_gdn_quad(xv[i], n, yv[i], RES ? &rv[i] : nullptr, INV ? 1 : 0, gs, o, g, tv);
                if (a.out) stq(a.out + g0 + lane_e + 16 * i, o);
                if (a.gout) stq(a.gout + g0 + lane_e + 16 * i, g);
                if constexpr (PX) {
                    unsigned h0, l0, h1, l1;
                    rdo::h2_split_pk(g[0], g[1], a.gp.s, h0, l0, bad_g);
                    rdo::h2_split_pk(g[2], g[3], a.gp.s, h1, l1, bad_g);
                    u16* gd = a.gp.p + (ge + (unsigned)(i * 16 * a.Mq));
                    *reinterpret_cast<u32x2*>(gd) = u32x2{h0, h1};
                    *reinterpret_cast<u32x2*>(gd + a.M * CH) = u32x2{l0, l1};
                }
                stq(a.t + g0 + lane_e + 16 * i, tv);
                // IGDN: the chain takes sqrt(norm) in two launches, and they round differently: in the tail the call merges with the
                // sqrt inside the reciprocal square root and inherits its relaxed accuracy, in rdo_gdn_bwd_dx_h2 it stands alone and
                // is correctly rounded.  An opaque copy of norm keeps the two apart here as well (tests/test_gpu_gdn_fused.py)
                f32x4 nd = n;
                if (INV) asm volatile("" : "+v"(nd));
                gdn_dx_pre(g, xv[i], nd, INV ? 1 : 0, p[i][j], q[i][j]);
                acc[i][j] = tv;
                tmax = fmaxf(tmax, amax_quad(tv));
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            if (kg == 0) wmax[cg * BM + tok] = tmax;
            if constexpr (PX) rdo::h2_report(bad_g, a.gp.ovf);
        }
        __syncthreads();                                              // every wave has left GEMM 1: the panel is free; the partial maxima are in
        // ---- t as planes, with the per-token scale over all 192 channels
        float inv_t[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int tok = 32 * th + 16 * j + l16;
            const float amax = fmaxf(fmaxf(wmax[tok], wmax[BM + tok]), fmaxf(wmax[2 * BM + tok], wmax[3 * BM + tok]));
            float sc;
            token_scale(amax, sc, inv_t[j]);
#pragma unroll
            for (int i = 0; i < 3; ++i) split_quad_store(acc[i][j], sc, smem + (3 * cg + i) * (BM * 32) + tok * 32 + kg * 8, PLANE);
        }
        gemm(rs_b, acc);                                              // t . gamma'
        // ---- dx
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long g0 = (m0 + 16 * j) * CH;
            const float f = inv_t[j] * a.inv_wscale;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const f32x4 av = acc[i][j] * f;
                const f32x4 d = gdn_dx_fin(p[i][j], q[i][j], av);
                if (a.dx) stq(a.dx + g0 + lane_e + 16 * i, d);
                if (a.dxp.p) {                                        // slice-major planes [2][12][M][16]: 8 bytes per plane, 32-byte records by four lanes
                    const long e = ((long)(3 * cg + i) * a.M + m0 + 16 * j) * 16 + (unsigned)((32 * th + l16) * 16 + 4 * kg);
                    unsigned h0, l0, h1, l1;
                    rdo::h2_split_pk(d[0], d[1], a.dxp.s, h0, l0, bad);
                    rdo::h2_split_pk(d[2], d[3], a.dxp.s, h1, l1, bad);
                    *reinterpret_cast<u32x2*>(a.dxp.p + e) = u32x2{h0, h1};
                    *reinterpret_cast<u32x2*>(a.dxp.p + a.M * CH + e) = u32x2{l0, l1};
                }
            }
        }
        __syncthreads();                                              // every wave has left GEMM 2 before the next panel goes in
    }
    if (a.dxp.p) rdo::h2_report(bad, a.dxp.ovf);
    block_loss_add8(lsum, a.inv_npix * a.coef, a.loss_out, it, a.pub, wsum);
}

bool pow2(float s) {
    if (!(s > 0.f) || s != s || s > 3.0e38f) return false;
    int e;
    return frexpf(s, &e) == 0.5f;
}

int cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    return n;
}

}  // namespace

extern "C" int rdo_gdn_fwd_bwd_supported(int64_t M, int32_t C) {
    return C == CH && M > 0 && M % BM == 0 && rdo_linear_h2_supported(M, C, C);
}

static int gdn_fwd_bwd_impl(const float* c, const void* fwd_planes, const void* bwd_planes, float wscale, const float* beta,
                            const float* residual, const float* tgt_cache, const int32_t* idx_table, const int32_t* iter_ptr, int32_t B,
                            int64_t per_image, int32_t C, float coef, int32_t inverse, float* out, float* grad_out, float* t, float* dx,
                            void* dx_planes, float dx_scale, float* loss_out, void* stream, void* dup_planes, float dup_scale, int32_t W,
                            void* dup_flag) {
    RDO_REQUIRE(c && fwd_planes && bwd_planes && beta && tgt_cache && idx_table && iter_ptr && t, "rdo_gdn_fwd_bwd: null pointer");
    RDO_REQUIRE(B > 0 && C > 0 && per_image > 0 && per_image % C == 0, "rdo_gdn_fwd_bwd: bad shape");
    const int64_t M = (int64_t)B * (per_image / C);
    RDO_REQUIRE(rdo_gdn_fwd_bwd_supported(M, C), "rdo_gdn_fwd_bwd: %ld tokens x %d channels is not supported (C = 192, tokens %% 64)", (long)M, C);
    RDO_REQUIRE(pow2(wscale), "rdo_gdn_fwd_bwd: weight scale %g is not a power of two", (double)wscale);
    RDO_REQUIRE(!dx_planes || dx_scale > 0.f, "rdo_gdn_fwd_bwd: dx_scale must be a positive power of two");
    RDO_REQUIRE(((reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(fwd_planes) | reinterpret_cast<uintptr_t>(bwd_planes) |
                  reinterpret_cast<uintptr_t>(beta) | reinterpret_cast<uintptr_t>(residual) | reinterpret_cast<uintptr_t>(tgt_cache) |
                  reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(t) |
                  reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dx_planes)) & 15) == 0,
                "rdo_gdn_fwd_bwd: pointers must be 16-byte aligned");
    GdnArgs a;
    a.c = c; a.wf = reinterpret_cast<const u16*>(fwd_planes); a.wb = reinterpret_cast<const u16*>(bwd_planes); a.beta = beta; a.res = residual;
    a.tgt = tgt_cache; a.idx = idx_table; a.iter = iter_ptr; a.pub = rdo::take_iter_publish();
    a.B = B; a.ntiles = (int)(M / BM); a.inverse = inverse ? 1 : 0; a.per_image = (long)per_image; a.M = (long)M;
    a.inv_wscale = 1.0f / wscale; a.inv_npix = (float)(1.0 / (double)M); a.coef = coef;
    a.out = out; a.gout = grad_out; a.t = t; a.dx = dx;
    a.dxp = H2Out{reinterpret_cast<u16*>(dx_planes), dx_scale, rdo::h2_overflow_flag()};
    a.loss_out = loss_out;
    a.gp = H2Out{reinterpret_cast<u16*>(dup_planes), dup_scale, dup_flag ? reinterpret_cast<int*>(dup_flag) : rdo::h2_overflow_flag()};
    a.W = W; a.HW = (int)(per_image / C); a.Mq = (int)(M / 4);
    const double n = (double)M * C;
    // passes it really makes: c, target (+ residual) in; t (+ out, g, dx, dx planes) out; both weights
    const double bytes = n * (12.0 + 4.0 * ((residual != nullptr) + (out != nullptr) + (grad_out != nullptr) + (dx != nullptr)) + (dx_planes ? 4.0 : 0.0) + (dup_planes ? 4.0 : 0.0)) +
                         2.0 * 4.0 * C * C;
    return rdo::dispatch(
        [a](hipStream_t s) {
            const int wgs = cu_count();                               // one resident workgroup per CU walks the tiles
            const dim3 grid((unsigned)(a.ntiles < wgs ? a.ntiles : wgs));
            if (a.gp.p) {
                if (a.inverse && a.res) hipLaunchKernelGGL((gdn_fwd_bwd_kernel<true, true, true>), grid, dim3(512), LDS_BYTES, s, a);
                else if (a.inverse) hipLaunchKernelGGL((gdn_fwd_bwd_kernel<true, false, true>), grid, dim3(512), LDS_BYTES, s, a);
                else if (a.res) hipLaunchKernelGGL((gdn_fwd_bwd_kernel<false, true, true>), grid, dim3(512), LDS_BYTES, s, a);
                else hipLaunchKernelGGL((gdn_fwd_bwd_kernel<false, false, true>), grid, dim3(512), LDS_BYTES, s, a);
                return rdo::check_launch("gdn_fwd_bwd_px");
            }
            if (a.inverse && a.res) hipLaunchKernelGGL((gdn_fwd_bwd_kernel<true, true>), grid, dim3(512), LDS_BYTES, s, a);
            else if (a.inverse) hipLaunchKernelGGL((gdn_fwd_bwd_kernel<true, false>), grid, dim3(512), LDS_BYTES, s, a);
            else if (a.res) hipLaunchKernelGGL((gdn_fwd_bwd_kernel<false, true>), grid, dim3(512), LDS_BYTES, s, a);
            else hipLaunchKernelGGL((gdn_fwd_bwd_kernel<false, false>), grid, dim3(512), LDS_BYTES, s, a);
            return rdo::check_launch("gdn_fwd_bwd");
        },
        stream, "linear_h2_gdn", 2.0 * 2.0 * (double)M * C * C, bytes);
}

extern "C" int rdo_gdn_fwd_bwd(const float* c, const void* fwd_planes, const void* bwd_planes, float wscale, const float* beta,
                               const float* residual, const float* tgt_cache, const int32_t* idx_table, const int32_t* iter_ptr, int32_t B,
                               int64_t per_image, int32_t C, float coef, int32_t inverse, float* out, float* grad_out, float* t, float* dx,
                               void* dx_planes, float dx_scale, float* loss_out, void* stream) {
    return gdn_fwd_bwd_impl(c, fwd_planes, bwd_planes, wscale, beta, residual, tgt_cache, idx_table, iter_ptr, B, per_image, C, coef, inverse, out,
                            grad_out, t, dx, dx_planes, dx_scale, loss_out, stream, nullptr, 1.f, 0, nullptr);
}

extern "C" int rdo_gdn_fwd_bwd_px_supported(int64_t M, int32_t C, int32_t H, int32_t W) {
    return rdo_gdn_fwd_bwd_supported(M, C) && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && M % ((int64_t)H * W) == 0 && M * C < (1LL << 31);
}

extern "C" int rdo_gdn_fwd_bwd_px(const float* c, const void* fwd_planes, const void* bwd_planes, float wscale, const float* beta,
                                  const float* residual, const float* tgt_cache, const int32_t* idx_table, const int32_t* iter_ptr, int32_t B,
                                  int32_t H, int32_t W, int32_t C, float coef, int32_t inverse, float* out, void* dup_planes, float dup_scale,
                                  void* dup_overflow_flag, float* t, float* dx, void* dx_planes, float dx_scale, float* loss_out, void* stream) {
    RDO_REQUIRE(dup_planes && (reinterpret_cast<uintptr_t>(dup_planes) & 15) == 0, "rdo_gdn_fwd_bwd_px: dup_planes null or not 16-byte aligned");
    RDO_REQUIRE(pow2(dup_scale), "rdo_gdn_fwd_bwd_px: dup_scale %g is not a power of two", (double)dup_scale);
    RDO_REQUIRE(B > 0 && rdo_gdn_fwd_bwd_px_supported((int64_t)B * H * W, C, H, W),
                "rdo_gdn_fwd_bwd_px: %d x %d x %d tokens x %d channels is not supported (rdo_gdn_fwd_bwd_px_supported)", B, H, W, C);
    return gdn_fwd_bwd_impl(c, fwd_planes, bwd_planes, wscale, beta, residual, tgt_cache, idx_table, iter_ptr, B, (int64_t)H * W * C, C, coef, inverse,
                            out, nullptr, t, dx, dx_planes, dx_scale, loss_out, stream, dup_planes, dup_scale, W, dup_overflow_flag);
}
