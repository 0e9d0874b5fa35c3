// The attention half of a Swin transformer block on the block-scaled matrix instruction, one launch (include/rdo_ptq_mxswinattn.h):
//   rdo_mx_swin_attn:  out = x + proj(window_attention(qkv(LN(x)))), every activation on the MX grid `act_format`, bit for bit the five
//                      launches rdo_mx_layer_norm_pack, rdo_mx_gemm, rdo_mx_window_attention, rdo_mx_quant_pack, rdo_mx_gemm and the add
// Built with -ffp-contract=off like mx_swin.hip and mx_attn.hip: acc + bias, raw * scale, + (bias + mask) and x + y are separate fp32
// operations.
//
// mx_swin_attn_kernel<NB, FA, FB>: NB = head dim rounded up to 32, over 32 (1 | 2), FA / FB the instruction's format numbers of the
// activations / of the weights.  One 256-thread workgroup owns a WINDOW with all of its heads: every stage behind the LayerNorm is local
// to the window, so no activation goes through global memory, and the workgroup sees every channel of a token, so the 32-channel blocks
// of proj's operand may straddle heads.  swin.hip's persistent grid over the windows (attn_item with one head), its pixel / region tables.
// Dynamic LDS (S* = mx_gdn.hip's row strides: blocks * bits dwords rounded up to four and made an odd number of 16-byte units):
//   attention images   mx_attn_device.h's: S fp32 [64][65] (before it the fp32 staging of v), Qp, Kp, Vt, Pp, 512 scale bytes
//   image A  [64][SA] dwords   the packed LayerNorm of the window's tokens, K = C; AFTER the last head the packed attention output
//   scales A [64][C / 32] bytes
//   tile O   fp32 [64][C + 4]  the attention output of every head (the stride keeps a lane's four channels one 16-byte store)
// beside 5 120 B static: mx_pack_tile's four wave-private byte tiles and the two tables.  In FP8, dynamic + static bytes:
//   C = 192, 8 heads of 24 (NB = 1):  33 536 + 13 312 + 384 + 50 176 = 97 408, + 5 120 = 102 528
//   C = 320, 5 heads of 64 (NB = 2):  37 632 + 21 504 + 640 + 82 944 = 142 720, + 5 120 = 147 840
// of the 163 840 B a gfx950 workgroup may have; C = 384 would need 168 448.  RDO_MXSWINATTN_MAX_C = 320 is also the widest row the
// row phase holds in its five float4 a lane (16 lanes x 5 x 4 channels).  The launch raises the kernel's dynamic-LDS attribute.
// One window:
//   tables     token -> pixel (shifted windows included) and -> mask region.                                      barrier
//   row phase  ln_pack_row (mx_swin_device.h) for the window's N <= 64 tokens, gathered by pixel: image A, scales A (-> `ln`).   barrier
//   per head, four barriers:
//     qkv      6 NB units of 32 tokens x 32 channels -- (q | k | v, head block, token half) -- to wave u % 4: unit_accumulate against the
//              head's rows of Wqkv (mx_gemm_accumulate's K order), + bqkv (-> `qkv`); a unit is one MX block a row, columns past hd and
//              rows past N are zeros: mx_pack_tile hands q's and k's rows to Qp / Kp as packed dwords; v goes to the staging image.  barrier
//     mx_attn_device.h's phases: Vt, Q K^T | barrier | scores | barrier | softmax, Pp | barrier | P V -> tile O (-> `attn`)
//     (no barrier before the next head's units: they write Qp, Kp and the staging image, which P V does not read)
//   pack       barrier; tile O's rows in blocks of 32 channels, ACROSS head boundaries -> image A, scales A (mx_quad_quant_store).   barrier
//   proj       2 C / 32 units against Wproj, + bproj (-> `branch`); x read again at the token's pixel, out = x + y stored there.     barrier
// No thread returns early or skips a barrier; a wave skips units that lie wholly past N between barriers.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxswinattn.h"
#include "mx_attn_device.h"
#include "mx_swin_device.h"

namespace {

constexpr int kVpl = 5;                                                         // float4 a lane of the row phase: C <= 16 * 5 * 4
static_assert(RDO_MXSWINATTN_MAX_C <= 64 * kVpl, "the row phase holds RDO_MXSWINATTN_MAX_C channels");
constexpr size_t kStaticLds = 4 * 32 * kPackRowDwords * sizeof(uint32_t) + 2 * NMAX * sizeof(int);
constexpr size_t kMaxLds = 160 * 1024;

struct SwinAttnArgs {
    const ln4 *x, *lw, *lb;                                                     // lw, lb nullable
    float eps;
    AttnGeom g;
    int windows, nbC, strideA, strideO;                                         // dwords of a row of image A, floats of a row of tile O
    MxFormat fa;
    const uint32_t *wqkv, *wproj;
    const uint8_t *sqkv, *sproj;
    const float *bqkv, *bproj, *bias;                                           // bqkv, bproj nullable
    float *out, *ln, *qkv, *attn, *branch;                                      // all but out nullable
};

inline size_t swin_attn_lds_bytes(int nb, int bits, int strideA, int strideO, int nbC) {
    return attn_lds_bytes(nb, bits, bits) + (size_t)64 * 4 * (strideA + strideO) + (size_t)64 * nbC;
}

template <int NB, int FA, int FB>
__global__ __launch_bounds__(256) void mx_swin_attn_kernel(SwinAttnArgs p) {
    constexpr int DF = hw_dwords(FA), SQ = row_dwords(NB, DF);
    extern __shared__ uint32_t lds[];
    const MxAttnTiles t = mx_attn_tiles<NB, FA, FA>(lds);
    uint32_t* imageA = lds + attn_lds_bytes(NB, DF, DF) / sizeof(uint32_t);
    float* O = reinterpret_cast<float*>(imageA + 64 * p.strideA);
    uint8_t* scalesA = reinterpret_cast<uint8_t*>(O + 64 * p.strideO);
    __shared__ int pix[NMAX], reg[NMAX];                                        // token -> pixel and -> mask region
    const AttnGeom& g = p.g;
    const int N = g.N, hd = g.hd, C = g.C, nbC = p.nbC, nbn = (N + 31) >> 5, strideA = p.strideA, strideO = p.strideO;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 15, kg = lane >> 4;
    const bool bias_vec = (N & 3) == 0 && reinterpret_cast<uintptr_t>(p.bias) % 16 == 0;
    const float* xf = reinterpret_cast<const float*>(p.x);

    for (int id = blockIdx.x; id < p.windows; id += gridDim.x) {
        int win, none;
        attn_item(id, p.windows, 1, win, none);
        if (tid < N) {
            pix[tid] = token_pixel(g, win, tid);
            reg[tid] = g.shift > 0 ? token_region(g, win, tid) : 0;
        }
        __syncthreads();
        // ---- row phase: LN(x) of the window's tokens -> packed blocks and scale bytes of image A ------------------------------------------
        {
            const int l16 = tid & 15, grp = tid >> 4, C4 = C >> 2;
            const float invC = 1.f / (float)C;
            for (int pass = 0; 16 * pass < 32 * nbn; ++pass) {
                const int lr = 16 * pass + grp;
                const bool live = lr < N;
                ln_pack_row<kVpl>(p.x, nullptr, p.lw, p.lb, C4, l16, invC, p.eps, live ? pix[lr] : 0, live, true, nullptr,
                                  reinterpret_cast<ln4*>(p.ln), p.fa, imageA + lr * strideA, scalesA + lr * nbC);
            }
        }
        __syncthreads();

        for (int head = 0; head < g.heads; ++head) {
            // ---- q, k, v of the head: units of the qkv GEMM -> Qp, Kp, the staging image of v ------------------------------------------
            for (int u = w; u < 6 * NB; u += 4) {
                const int m0 = 32 * (u & 1), hb = (u >> 1) % NB, which = (u >> 1) / NB;        // uniform over the wave
                if (m0 >= N) continue;
                const int n0 = which * C + head * hd + 32 * hb;                // the unit's first row of Wqkv = its first channel of qkv
                f32x4 acc[2][2], v[2][2];
                unit_accumulate<FA, FB>(imageA, strideA, scalesA, nbC, p.wqkv, p.sqkv, m0, n0, r, kg, acc, 3 * C - 1);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int d = 32 * hb + 16 * j + r, col = n0 + 16 * j + r;  // channel inside the head; channel of qkv
                    const bool cok = d < hd;
                    const float bj = (cok && p.bqkv) ? p.bqkv[col] : 0.f;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int tok = m0 + 16 * i + 4 * kg + q;
                            const bool live = cok && tok < N;
                            const float val = live ? acc[i][j][q] + bj : 0.f;
                            if (live) {
                                if (p.qkv) p.qkv[(long)pix[tok] * (3 * C) + col] = val;
                                if (which == 2) t.S[tok * SS + d] = val;
                            }
                            v[i][j][q] = val;
                        }
                }
                if (which < 2) {
                    uint32_t* image = which == 0 ? t.Qp : t.Kp;
                    uint8_t* sc = which == 0 ? t.sQ : t.sK;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the previous unit's byte-tile reads precede these writes
                    __builtin_amdgcn_wave_barrier();
                    mx_pack_tile(v, p.fa, [&](int row, int h, const unsigned (&d)[4], unsigned scale) {
                        const int lr = m0 + row;
                        mx_put_dwords(image + lr * SQ + hb * DF + h * (DF >> 1), d, DF);
                        if (h == 0) sc[lr * 2 + hb] = (uint8_t)(lr < N ? scale : 127u);
                    });
                }
            }
            __syncthreads();
            // ---- the attention of (window, head) on the images: mx_attn_device.h -----------------------------------------------------------
            mx_attn_vt<NB, FA>(t, p.fa, N, hd, nbn, w, lane);
            f32x4 raw[2][2];
            const bool unit = mx_attn_qk<NB, FA>(t, N, w, r, kg, raw);
            float bs[16];
            mx_attn_bias(p.bias, head, N, tid, bias_vec, bs);
            __syncthreads();                                                    // every wave has read the staging image: S may go over it
            if (unit) mx_attn_scores(t.S, raw, g.scale, w, r, kg);
            __syncthreads();
            mx_attn_softmax<FA>(t, p.fa, bs, reg, g.shift, N, nbn, tid, nullptr, nullptr, 0L, g.heads);
            __syncthreads();
            mx_attn_pv<NB, FA, FA>(t, N, hd, nbn, w, r, kg, [&](int tok, int c0, af4 o) {
                *reinterpret_cast<af4*>(O + tok * strideO + head * hd + c0) = o;
                if (p.attn) *reinterpret_cast<af4*>(p.attn + (long)pix[tok] * C + head * hd + c0) = o;
            });
        }
        __syncthreads();                                                        // tile O is complete; image A is dead
        // ---- pack: tile O's rows in blocks of 32 channels -> image A (eight lanes a block, four channels a lane) -------------------------
        for (int it = 0; it < nbn * nbC; ++it) {                                // 32 nbn rows x nbC blocks, 32 blocks a pass
            const int blk = (tid >> 3) + 32 * it, row = blk / nbC, kb = blk - row * nbC, s = tid & 7;
            const af4 o = *reinterpret_cast<const af4*>(O + row * strideO + 32 * kb + 4 * s);
            const bool live = row < N;                                          // (a row past N was never written: zeros)
            const float v[4] = {live ? o[0] : 0.f, live ? o[1] : 0.f, live ? o[2] : 0.f, live ? o[3] : 0.f};
            const unsigned sc = mx_quad_quant_store(v, p.fa, imageA + row * strideA + kb * DF, true);
            if (s == 0) scalesA[row * nbC + kb] = (uint8_t)sc;
        }
        __syncthreads();
        // ---- proj: branch = attn Wproj^T + bproj, out = x + branch at the token's pixel --------------------------------------------------
        for (int u = w; u < 2 * nbC; u += 4) {
            const int m0 = 32 * (u & 1), n0 = 32 * (u >> 1);
            if (m0 >= N) continue;
            f32x4 acc[2][2];
            unit_accumulate<FA, FB>(imageA, strideA, scalesA, nbC, p.wproj, p.sproj, m0, n0, r, kg, acc);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = n0 + 16 * j + r;
                const float bj = p.bproj ? p.bproj[col] : 0.f;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int tok = m0 + 16 * i + 4 * kg + q;
                        if (tok >= N) continue;
                        const long at = (long)pix[tok] * C + col;
                        const float y = acc[i][j][q] + bj;
                        if (p.branch) p.branch[at] = y;
                        p.out[at] = xf[at] + y;
                    }
            }
        }
        __syncthreads();                                                        // every wave is done with this window's tables and images
    }
}

using SwinAttnKernel = void (*)(SwinAttnArgs);

// [head blocks - 1][activation format][weight format], the instruction's format numbers
#define RDO_MXSWINATTN_ROW(NB, FA) \
    {mx_swin_attn_kernel<NB, FA, 0>, mx_swin_attn_kernel<NB, FA, 1>, mx_swin_attn_kernel<NB, FA, 2>, mx_swin_attn_kernel<NB, FA, 3>, mx_swin_attn_kernel<NB, FA, 4>}
#define RDO_MXSWINATTN_NB(NB) \
    {RDO_MXSWINATTN_ROW(NB, 0), RDO_MXSWINATTN_ROW(NB, 1), RDO_MXSWINATTN_ROW(NB, 2), RDO_MXSWINATTN_ROW(NB, 3), RDO_MXSWINATTN_ROW(NB, 4)}
const SwinAttnKernel kSwinAttn[2][5][5] = {RDO_MXSWINATTN_NB(1), RDO_MXSWINATTN_NB(2)};
#undef RDO_MXSWINATTN_NB
#undef RDO_MXSWINATTN_ROW

}  // namespace

extern "C" {

int rdo_mx_swin_attn(const rdo_attn_desc* desc, const float* x, const float* ln_weight, const float* ln_bias, float eps,
                     int32_t act_format, const void* wqkv, const uint8_t* wqkv_scales, const float* bqkv, const void* wproj,
                     const uint8_t* wproj_scales, const float* bproj, int32_t w_format, const float* bias, float* out, float* ln,
                     float* qkv, float* attn, float* branch, void* stream) {
    const char* who = "rdo_mx_swin_attn";
    SwinAttnArgs p;
    if (int rc = make_geom(desc, &p.g, who)) return rc;
    const AttnGeom& g = p.g;
    RDO_REQUIRE(g.hd % 4 == 0, "%s: head dim %d (C=%d, heads=%d) is no multiple of 4", who, g.hd, g.C, g.heads);
    RDO_REQUIRE(g.C % kBlock == 0, "%s: C %d is no multiple of the block size %d", who, g.C, kBlock);
    RDO_REQUIRE(g.C <= RDO_MXSWINATTN_MAX_C, "%s: C %d is above %d, the most whose window fits the kernel's LDS", who, g.C, RDO_MXSWINATTN_MAX_C);
    MxFormat fw;
    RDO_REQUIRE(mx_format(act_format, p.fa), "%s: unknown act_format %d (0 .. %d)", who, (int)act_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(mx_format(w_format, fw), "%s: unknown w_format %d (0 .. %d)", who, (int)w_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(x && wqkv && wqkv_scales && wproj && wproj_scales && bias && out, "%s: null pointer", who);
    RDO_REQUIRE(aligned16(x) && aligned16(ln_weight) && aligned16(ln_bias) && aligned16(bqkv) && aligned16(bproj) && aligned16(out) &&
                    aligned16(ln) && aligned16(qkv) && aligned16(attn) && aligned16(branch),
                "%s: x, ln_weight, ln_bias, bqkv, bproj, out, ln, qkv, attn and branch must be 16-byte aligned", who);
    RDO_REQUIRE(aligned4(bias) && aligned4(wqkv) && aligned4(wproj), "%s: bias, wqkv and wproj must be 4-byte aligned", who);
    p.x = reinterpret_cast<const ln4*>(x);
    p.lw = reinterpret_cast<const ln4*>(ln_weight);
    p.lb = reinterpret_cast<const ln4*>(ln_bias);
    p.eps = eps;
    p.windows = g.B * (g.H / g.ws) * (g.W / g.ws);
    p.nbC = g.C / kBlock;
    p.strideA = lds_row_dwords(p.nbC, p.fa.bits);
    p.strideO = g.C + 4;
    p.wqkv = static_cast<const uint32_t*>(wqkv);
    p.wproj = static_cast<const uint32_t*>(wproj);
    p.sqkv = wqkv_scales;
    p.sproj = wproj_scales;
    p.bqkv = bqkv;
    p.bproj = bproj;
    p.bias = bias;
    p.out = out;
    p.ln = ln;
    p.qkv = qkv;
    p.attn = attn;
    p.branch = branch;
    const int nb = (g.hd + kBlock - 1) / kBlock;
    const SwinAttnKernel kern = kSwinAttn[nb - 1][hw_format(act_format)][hw_format(w_format)];
    const size_t lds = swin_attn_lds_bytes(nb, p.fa.bits, p.strideA, p.strideO, p.nbC);
    RDO_REQUIRE(lds + kStaticLds <= kMaxLds, "%s: C %d needs %zu B of LDS", who, g.C, lds + kStaticLds);
    // the workgroup's whole LDS is above 64 KiB at every Swin width: C = 192 in FP8 is 97 408 B dynamic, 102 528 B in all
    if (lds + kStaticLds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return rdo::set_error(RDO_EHIP, "%s: hipFuncSetAttribute(%zu B LDS) failed", who, lds);
    const int windows = p.windows;
    const double pixels = (double)g.B * g.H * g.W, items = (double)windows * g.heads;
    const double wbytes = 4.0 * p.nbC * g.C * (4.0 * fw.bits + 1.0);
    return rdo::dispatch(
        [=](hipStream_t s) {
            const long grid = resident_grid(kern, lds, windows);
            hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, s, p);
            return rdo::check_launch("mx_swin_attn");
        },
        stream, "mx_swin_attn", 2.0 * pixels * g.C * 4.0 * g.C + 4.0 * items * g.N * g.N * g.hd,
        4.0 * pixels * g.C * (3.0 + (ln ? 1.0 : 0.0) + (qkv ? 3.0 : 0.0) + (attn ? 1.0 : 0.0) + (branch ? 1.0 : 0.0)) + wbytes);
}

}  // extern "C"
