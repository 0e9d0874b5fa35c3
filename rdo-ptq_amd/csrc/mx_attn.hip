// The window attention core with Q K^T and P V on the block-scaled matrix instruction (include/rdo_ptq_mxattn.h states the arithmetic):
//   rdo_mx_window_attention:  qkv -> Qp, Kp (blocks along hd) -> s = mx_gemm(Qp, Kp) * scale + (bias + mask) -> softmax -> Pp (blocks along j),
//                             Vt (blocks along the tokens) -> out = mx_gemm(Pp, Vt), one launch
// Built with -ffp-contract=off like the other MX files: raw * scale and + (bias + mask) are two fp32 operations.
//
// mx_win_attn_kernel<NB, F, FP>: NB = Hp / 32 head blocks (1 | 2), F / FP the instruction's format numbers of Q, K, V / of P.  One
// 256-thread workgroup per (window, head), swin.hip's persistent grid, item order (attn_item) and pixel / region tables.  Dynamic LDS:
//   S   fp32 [64][65]            the scores; BEFORE them the fp32 V staging, the same [64][65] -- dead once Vt is written
//   Qp, Kp  [64][SQ] dwords      packed rows of NB blocks;  Vt [64 channels][SV], Pp [64][SP]: packed rows of two token blocks
//   scale bytes [4][64][2]
//   row strides: blocks * bits dwords rounded up to four and made an odd number of 16-byte units (mx_gdn.hip's rule).  FP8 / FP8 at NB = 2:
//   16 640 + 4 x 5 120 + 512 = 37 632 B, four workgroups a CU by LDS.
// One item, five barriers (the phases behind the stash are mx_attn_device.h's, shared with mx_swin_attn.hip):
//   stash    the thread's 2 NB quads of q, k, v (fetched as unconditional 16-byte loads while the PREVIOUS item was multiplied; a quad past
//            hd or N re-reads a valid one and is zeroed) -- eight lanes hold the 32 channels of a block: mx_quad_quant_store writes the
//            packed dwords of Qp and Kp straight from the registers; v goes to the staging image.            barrier; fetch the next item
//   V, QK    thread (channel, token block, half) reads 16 values down a staging column (a wave reads 32 consecutive floats of two rows),
//            the lane pair l, l ^ 32 shares the block maximum, and each stores its half block of Vt.  Then wave w runs mx_mfma_step<F, F>
//            for the 32 x 32 unit (w >> 1, w & 1) of the scores from LDS fragments.                          barrier (the staging is dead)
//   scores   raw * scale -> S, in the accumulator layout.                                                    barrier
//   softmax  four threads a row, 16 CONSECUTIVE j each: s = S + (bias + mask), the bias row loaded before the two barriers above (16-byte
//            loads where N % 4 == 0), then softmax_rows256's arithmetic; a block of 32 is a thread pair, its maximum one shuffle; the
//            thread's half block of Pp is encoded in registers.                                              barrier
//   P V      transposed, O^T = Vt Pp^T: wave w owns token block w and every 16-channel tile, a lane's four accumulator values are four
//            consecutive channels of one token -- one 16-byte store.  With an FP8 operand the one-of-eight mask goes on the operand
//            rdo_mx_gemm(Pp, Vt) would mask (Pp if it is FP8, else Vt).                                      barrier (tables, images)
// Rows and columns past N or hd are zero codes under scale 127; a unit or tile wholly past N is skipped by its wave between barriers.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxattn.h"
#include "mx_attn_device.h"

namespace {

struct MxAttnArgs {
    const float *qkv, *bias;
    float *out, *scores, *probs;                                                // scores, probs nullable
    AttnGeom g;
    int windows, nitems;
    MxFormat f, fp;
};

template <int NB, int F, int FP>
__global__ __launch_bounds__(256, 3) void mx_win_attn_kernel(MxAttnArgs p) {
    constexpr int T = 2 * NB, QPP = 8 * NB;                                     // quads a thread and tile; quads a padded token row
    constexpr int DF = hw_dwords(F), SQ = row_dwords(NB, DF);                   // dwords of a block = element bits
    extern __shared__ uint32_t lds[];
    const MxAttnTiles t = mx_attn_tiles<NB, F, FP>(lds);
    float *S = t.S, *Vs = t.S;
    uint32_t *Qp = t.Qp, *Kp = t.Kp;
    uint8_t *sQ = t.sQ, *sK = t.sK;
    __shared__ int pix[2][NMAX], reg[2][NMAX];                                  // token -> pixel and -> mask region, per item
    const AttnGeom& g = p.g;
    const int N = g.N, hd = g.hd, nbn = (N + 31) >> 5;

    auto tables = [&](int b, int win) {
        if ((int)threadIdx.x < N) {
            pix[b][threadIdx.x] = token_pixel(g, win, threadIdx.x);
            reg[b][threadIdx.x] = g.shift > 0 ? token_region(g, win, threadIdx.x) : 0;
        }
    };
    // the thread's quads of a tile: quad e = thread + 256 it is channels 4 (e % QPP) .. + 3 of token e / QPP; one past hd or N loads a
    // valid quad instead (the loads stay unconditional, swin.hip's `tile_fetch`) and counts as zeros
    int ltok[T], lch[T];
    bool qok[T];
#pragma unroll
    for (int it = 0; it < T; ++it) {
        const int e = threadIdx.x + 256 * it, tok = e / QPP, ch = 4 * (e % QPP);
        qok[it] = tok < N && ch < hd;
        ltok[it] = tok < N ? tok : N - 1;
        lch[it] = ch < hd ? ch : hd - 4;
    }
    af4 rq[T], rk[T], rv[T];
    auto fetch = [&](int b, int head) {
#pragma unroll
        for (int it = 0; it < T; ++it) {
            const float* src = p.qkv + (long)pix[b][ltok[it]] * (3 * g.C) + head * hd + lch[it];
            rq[it] = *reinterpret_cast<const af4*>(src);
            rk[it] = *reinterpret_cast<const af4*>(src + g.C);
            rv[it] = *reinterpret_cast<const af4*>(src + 2 * g.C);
        }
    };

    const bool bias_vec = (N & 3) == 0 && reinterpret_cast<uintptr_t>(p.bias) % 16 == 0;
    int id = blockIdx.x, buf = 0, win, head;
    attn_item(id, p.windows, g.heads, win, head);
    tables(0, win);
    __syncthreads();
    fetch(0, head);
    for (;;) {
        // Index arithmetic from an opaque copy of the thread id: hipcc otherwise hoists every address of every phase out of the item loop
        // (some sixty VGPRs of loop invariants beside the prefetch registers, and scratch)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 15, kg = lane >> 4;
        // ---- stash: Qp, Kp from the registers, v to the staging image ------------------------------------------------------------------
#pragma unroll
        for (int it = 0; it < T; ++it) {
            const int e = tid + 256 * it, tok = e / QPP, quad = e % QPP, kb = quad >> 3;
            const bool ok = qok[it];
            const float q4[4] = {ok ? rq[it][0] : 0.f, ok ? rq[it][1] : 0.f, ok ? rq[it][2] : 0.f, ok ? rq[it][3] : 0.f};
            const float k4[4] = {ok ? rk[it][0] : 0.f, ok ? rk[it][1] : 0.f, ok ? rk[it][2] : 0.f, ok ? rk[it][3] : 0.f};
            const unsigned scq = mx_quad_quant_store(q4, p.f, Qp + tok * SQ + kb * DF, true);
            const unsigned sck = mx_quad_quant_store(k4, p.f, Kp + tok * SQ + kb * DF, true);
            if ((quad & 7) == 0) {
                sQ[tok * 2 + kb] = (uint8_t)(tok < N ? scq : 127u);
                sK[tok * 2 + kb] = (uint8_t)(tok < N ? sck : 127u);
            }
            if (ok) {
                float* d = Vs + tok * SS + 4 * quad;                            // (an odd row stride: scalar LDS stores)
                d[0] = rv[it][0]; d[1] = rv[it][1]; d[2] = rv[it][2]; d[3] = rv[it][3];
            }
        }
        const int nid = id + gridDim.x;
        const bool more = nid < p.nitems;
        int nwin = 0, nhead = 0;
        if (more) {
            attn_item(nid, p.windows, g.heads, nwin, nhead);
            tables(buf ^ 1, nwin);
        }
        __syncthreads();                                                        // tiles of this item and tables of the next are visible
        if (more) fetch(buf ^ 1, nhead);                                        // in flight while this item is multiplied
        // ---- Vt, raw = Qp Kp^T, the bias row (in flight under the barriers and the S image): mx_attn_device.h ---------------------------------
        mx_attn_vt<NB, F>(t, p.f, N, hd, nbn, w, lane);
        f32x4 acc[2][2];
        const bool unit = mx_attn_qk<NB, F>(t, N, w, r, kg, acc);
        float bs[16];
        mx_attn_bias(p.bias, head, N, tid, bias_vec, bs);
        __syncthreads();                                                        // every wave has read the staging image: S may go over it
        if (unit) mx_attn_scores(S, acc, g.scale, w, r, kg);
        __syncthreads();
        mx_attn_softmax<FP>(t, p.fp, bs, reg[buf], g.shift, N, nbn, tid, p.scores, p.probs, ((long)win * N * N) * g.heads + head, g.heads);
        __syncthreads();
        {
            const int tok = 16 * w + r;
            float* orow = p.out + (long)pix[buf][tok < N ? tok : N - 1] * g.C + head * hd;
            mx_attn_pv<NB, F, FP>(t, N, hd, nbn, w, r, kg, [&](int, int c0, af4 o) { *reinterpret_cast<af4*>(orow + c0) = o; });
        }
        if (!more) break;
        __syncthreads();                                                        // every wave is done with this item's tables and images
        id = nid; win = nwin; head = nhead; buf ^= 1;
    }
}

using AttnKernel = void (*)(MxAttnArgs);

// [head blocks - 1][format of q, k, v][format of p], the instruction's format numbers
#define RDO_MXATTN_ROW(NB, F) \
    {mx_win_attn_kernel<NB, F, 0>, mx_win_attn_kernel<NB, F, 1>, mx_win_attn_kernel<NB, F, 2>, mx_win_attn_kernel<NB, F, 3>, mx_win_attn_kernel<NB, F, 4>}
#define RDO_MXATTN_NB(NB) {RDO_MXATTN_ROW(NB, 0), RDO_MXATTN_ROW(NB, 1), RDO_MXATTN_ROW(NB, 2), RDO_MXATTN_ROW(NB, 3), RDO_MXATTN_ROW(NB, 4)}
const AttnKernel kAttn[2][5][5] = {RDO_MXATTN_NB(1), RDO_MXATTN_NB(2)};
#undef RDO_MXATTN_NB
#undef RDO_MXATTN_ROW

}  // namespace

extern "C" {

int rdo_mx_window_attention(const rdo_attn_desc* desc, const float* qkv, const float* bias, int32_t format, int32_t p_format, float* out,
                            float* scores, float* probs, void* stream) {
    const char* who = "rdo_mx_window_attention";
    MxAttnArgs p;
    if (int rc = make_geom(desc, &p.g, who)) return rc;
    const AttnGeom& g = p.g;
    RDO_REQUIRE(g.hd % 4 == 0, "%s: head dim %d (C=%d, heads=%d) is no multiple of 4", who, g.hd, g.C, g.heads);
    RDO_REQUIRE(mx_format(format, p.f), "%s: unknown format %d (0 .. %d)", who, (int)format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(mx_format(p_format, p.fp), "%s: unknown p_format %d (0 .. %d)", who, (int)p_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(qkv && bias && out, "%s: null pointer", who);
    RDO_REQUIRE(aligned16(qkv) && aligned16(out), "%s: qkv and out must be 16-byte aligned", who);
    RDO_REQUIRE(aligned4(bias) && aligned4(scores) && aligned4(probs), "%s: bias, scores and probs must be 4-byte aligned", who);
    p.qkv = qkv;
    p.bias = bias;
    p.out = out;
    p.scores = scores;
    p.probs = probs;
    p.windows = g.B * (g.H / g.ws) * (g.W / g.ws);
    p.nitems = p.windows * g.heads;
    const int nb = (g.hd + kBlock - 1) / kBlock;
    const AttnKernel kern = kAttn[nb - 1][hw_format(format)][hw_format(p_format)];
    const size_t lds = attn_lds_bytes(nb, p.f.bits, p.fp.bits);
    const double pairs = (double)p.nitems, pix = (double)g.B * g.H * g.W;
    return rdo::dispatch(
        [=](hipStream_t s) {
            const long grid = resident_grid(kern, lds, p.nitems);
            hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, s, p);
            return rdo::check_launch("mx_window_attention");
        },
        stream, "mx_window_attention", 4.0 * pairs * g.N * g.N * g.hd,
        4.0 * (pix * g.C * 4.0 + (scores ? pairs * g.N * g.N : 0.0) + (probs ? pairs * g.N * g.N : 0.0)));
}

}  // extern "C"
