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
// One item, five barriers:
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
#include "attn_device.h"
#include "mx_pack_store_device.h"

#include <vector>

namespace {

typedef float af4 __attribute__((ext_vector_type(4)));

// dwords of an LDS operand row of nb blocks of `bits` dwords: a multiple of four, an odd number of 16-byte units
constexpr int row_dwords(int nb, int bits) {
    const int s = (nb * bits + 3) & ~3;
    return ((s >> 2) & 1) ? s : s + 4;
}
constexpr size_t attn_lds_bytes(int nb, int bits, int pbits) {
    return sizeof(uint32_t) * 64 * (SS + 2 * row_dwords(nb, bits) + row_dwords(2, bits) + row_dwords(2, pbits)) + 4 * 64 * 2;
}

struct MxAttnArgs {
    const float *qkv, *bias;
    float *out, *scores, *probs;                                                // scores, probs nullable
    AttnGeom g;
    int windows, nitems;
    MxFormat f, fp;
};

// sixteen codes of BITS bits -> BITS / 2 dwords of the block's little-endian bit string
template <int BITS>
__device__ __forceinline__ void pack16(const unsigned (&c)[16], unsigned (&d)[4]) {
    d[0] = d[1] = d[2] = d[3] = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int bit = k * BITS, w = bit >> 5, sh = bit & 31;
        d[w] |= c[k] << sh;
        if (sh + BITS > 32) d[w + 1] |= c[k] >> (32 - sh);
    }
}

// Sixteen neighbouring elements of a block whose other half lane ^ PARTNER holds: block maximum by one shuffle, mx_block_exponent /
// mx_encode as everywhere, the half's BITS / 2 packed dwords to dst[0 ..] where `store`.  Returns the scale byte (255 and zero codes for a
// block that holds a NaN or an infinity).  Called by both lanes of a pair.
template <int BITS, int PARTNER>
__device__ __forceinline__ unsigned half_block_quant(const float (&v)[16], const MxFormat& f, uint32_t* dst, bool store) {
    unsigned pat[16], amax = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        pat[k] = __builtin_bit_cast(unsigned, v[k]);
        const unsigned m = pat[k] & 0x7FFFFFFFu;
        amax = m > amax ? m : amax;
    }
    const unsigned u = __shfl_xor(amax, PARTNER, 64);
    amax = u > amax ? u : amax;
    const bool finite = amax < 0x7F800000u;
    const int E = finite ? mx_block_exponent(amax, f) : -127;
    unsigned c[16], d[4];
#pragma unroll
    for (int k = 0; k < 16; ++k) c[k] = finite ? mx_encode(pat[k] & 0x7FFFFFFFu, E, f) | ((pat[k] & 0x80000000u) >> (32 - BITS)) : 0u;
    pack16<BITS>(c, d);
    if (store) {
#pragma unroll
        for (int n = 0; n < BITS / 2; ++n) dst[n] = d[n];
    }
    return finite ? (unsigned)(E + 127) : 255u;
}

// the lane's operand registers and scale for K block kg of a row of an LDS tile that holds nb blocks (one K step: kg >= nb is zero under 127)
template <int DW>
__device__ __forceinline__ i32x8 lds_fragment(const uint32_t* row, const uint8_t* sc, int kg, int nb, int& scale) {
    scale = kg < nb ? (int)sc[kg] : 127;
    return load_fragment<DW>(row, 0, kg, nb, true);
}

template <int NB, int F, int FP>
__global__ __launch_bounds__(256, 3) void mx_win_attn_kernel(MxAttnArgs p) {
    constexpr int T = 2 * NB, QPP = 8 * NB;                                     // quads a thread and tile; quads a padded token row
    constexpr int DF = hw_dwords(F), DP = hw_dwords(FP);                       // dwords of a block = element bits
    constexpr int SQ = row_dwords(NB, DF), SV = row_dwords(2, DF), SP = row_dwords(2, DP);
    extern __shared__ uint32_t lds[];
    float* S = reinterpret_cast<float*>(lds);
    float* Vs = S;
    uint32_t* Qp = lds + 64 * SS;
    uint32_t* Kp = Qp + 64 * SQ;
    uint32_t* Vt = Kp + 64 * SQ;
    uint32_t* Pp = Vt + 64 * SV;
    uint8_t* sQ = reinterpret_cast<uint8_t*>(Pp + 64 * SP);
    uint8_t* sK = sQ + 128;
    uint8_t* sV = sK + 128;
    uint8_t* sP = sV + 128;
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
        const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 15, kg = lane >> 4, ti = w >> 1, tj = w & 1;
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
        // ---- Vt: blocks down the token axis ----------------------------------------------------------------------------------------------
        {
            const int d = 32 * (w >> 1) + (lane & 31), tb = w & 1, half = lane >> 5;
            if ((w >> 1) < NB && tb < nbn) {                                    // uniform over the wave
                float v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int tok = 32 * tb + 16 * half + k;
                    v[k] = (d < hd && tok < N) ? Vs[tok * SS + d] : 0.f;
                }
                const unsigned sc = half_block_quant<DF, 32>(v, p.f, Vt + d * SV + tb * DF + half * (DF / 2), true);
                if (half == 0) sV[d * 2 + tb] = (uint8_t)(d < hd ? sc : 127u);
            }
        }
        // ---- raw = Qp Kp^T: one K step -----------------------------------------------------------------------------------------------------
        const bool unit = 32 * ti < N && 32 * tj < N;                           // uniform over the wave
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (unit) {
            i32x8 fa[2], fb[2];
            int xa[2], xb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ra = 32 * ti + 16 * i + r, rb = 32 * tj + 16 * i + r;
                fa[i] = lds_fragment<DF>(Qp + ra * SQ, sQ + ra * 2, kg, NB, xa[i]);
                fb[i] = lds_fragment<DF>(Kp + rb * SQ, sK + rb * 2, kg, NB, xb[i]);
            }
            mx_mfma_step<F, F>(fa, fb, xa, xb, acc);
        }
        // bias of the thread's softmax columns (row tid / 4, 16 columns from 16 (tid & 3)): in flight under the barriers and the S image
        float bs[16];
        {
            const int i = tid >> 2, j0 = 16 * (tid & 3);
            const float* brow = p.bias + ((long)head * N + (i < N ? i : N - 1)) * N;
            if (bias_vec) {                                                     // N % 4 == 0: a quad lies inside the row or past it
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4) {
                    const int j = j0 + 4 * v4;
                    const af4 b = *reinterpret_cast<const af4*>(brow + (j < N ? j : N - 4));
                    bs[4 * v4] = b[0]; bs[4 * v4 + 1] = b[1]; bs[4 * v4 + 2] = b[2]; bs[4 * v4 + 3] = b[3];
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) bs[k] = brow[j0 + k < N ? j0 + k : N - 1];
            }
        }
        __syncthreads();                                                        // every wave has read the staging image: S may go over it
        if (unit) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        S[(32 * ti + 16 * i + 4 * kg + q) * SS + 32 * tj + 16 * j + r] = acc[i][j][q] * g.scale;
        }
        __syncthreads();
        // ---- softmax rows, Pp ----------------------------------------------------------------------------------------------------------
        {
            const int i = tid >> 2, part = tid & 3, blk = part >> 1;
            const bool rowok = i < N;
            const int ri = reg[buf][rowok ? i : 0];
            const long orow = (((long)win * N + i) * N) * g.heads + head;        // [windows, N, N, heads]
            float v[16];
            float mx = -3.0e38f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int j = 16 * part + k;
                float sv = -3.0e38f;
                if (rowok && j < N) {
                    const float bm = bs[k] + (g.shift > 0 && reg[buf][j] != ri ? -100.0f : 0.f);
                    sv = S[i * SS + j] + bm;
                    if (p.scores) p.scores[orow + (long)j * g.heads] = sv;
                }
                v[k] = sv;
                mx = fmaxf(mx, sv);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const float e = (rowok && 16 * part + k < N) ? __expf(v[k] - mx) : 0.f;
                v[k] = e;
                sum += e;
            }
            sum += __shfl_xor(sum, 1, 64);
            sum += __shfl_xor(sum, 2, 64);
            const float inv = rowok ? 1.0f / sum : 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int j = 16 * part + k;
                v[k] *= inv;
                if (p.probs && rowok && j < N) p.probs[orow + (long)j * g.heads] = v[k];
            }
            const bool st = blk < nbn;
            const unsigned sc = half_block_quant<DP, 1>(v, p.fp, Pp + i * SP + blk * DP + (part & 1) * (DP / 2), st);
            if (st && !(part & 1)) sP[i * 2 + blk] = (uint8_t)(rowok ? sc : 127u);
        }
        __syncthreads();
        // ---- O^T = Vt Pp^T: token block w, every 16-channel tile -------------------------------------------------------------------------
        if (16 * w < N) {
            const int tok = 16 * w + r;
            int xp;
            const i32x8 fp = lds_fragment<DP>(Pp + tok * SP, sP + tok * 2, kg, nbn, xp);
            float* orow = p.out + (long)pix[buf][tok < N ? tok : N - 1] * g.C + head * hd;
#pragma unroll
            for (int db = 0; db < 2 * NB; ++db) {
                if (16 * db >= hd) break;
                const int d = 16 * db + r;
                int xv;
                const i32x8 fv = lds_fragment<DF>(Vt + d * SV, sV + d * 2, kg, nbn, xv);
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if constexpr (DF == 8 || DP == 8) {
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const i32x8 mp = DP == 8 ? keep_one_of_eight(fp, t) : fp;
                        const i32x8 mv = DP == 8 ? fv : keep_one_of_eight(fv, t);
                        o = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mv, mp, o, F, FP, 0, xv, 0, xp);
                    }
                } else {
                    o = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fv, fp, o, F, FP, 0, xv, 0, xp);
                }
                // The products are complete BEFORE the store's per-lane condition: the matrix instruction reads every lane's operand
                // registers whatever EXEC says, and hipcc otherwise sinks it and the mask arithmetic into the branch of the lanes that
                // store -- the other lanes' operands are then stale registers (a head dim that is no multiple of 16: NaNs in `out`)
                asm volatile("" : "+v"(o));
                const int c0 = 16 * db + 4 * kg;                                // the lane's four channels of token `tok`
                if (tok < N && c0 < hd) *reinterpret_cast<af4*>(orow + c0) = af4{o[0], o[1], o[2], o[3]};
            }
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

// swin.hip's persistent grid: as many workgroups as are resident at once (registers count as well as LDS), a multiple of 8 so that a
// workgroup's items stay on one XCD; never more than there are items
long resident_grid(AttnKernel kern, size_t lds, int nitems) {
    struct Memo { AttnKernel kern; int dev; long resident; };
    static thread_local std::vector<Memo> memo;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    long resident = 0;
    for (const Memo& m : memo)
        if (m.kern == kern && m.dev == dev) resident = m.resident;
    if (resident == 0) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), 256, lds) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 8) cus = 256;
        resident = (long)per_cu * cus / 8 * 8;
        memo.push_back(Memo{kern, dev, resident});
    }
    return nitems < resident ? nitems : resident;
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

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
