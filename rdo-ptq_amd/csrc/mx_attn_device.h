// The phases of the MX window attention of one (window, head) on LDS images, stated once for mx_attn.hip (a workgroup per (window, head),
// q, k, v from global memory) and mx_swin_attn.hip (a workgroup per window, q, k, v from its own qkv GEMM): include/rdo_ptq_mxattn.h
// states the arithmetic, the header comment of mx_attn.hip the images and which thread does what.  A phase is one function; the caller
// places the workgroup barriers between them:
//   [Qp, Kp, their scale bytes and the fp32 staging image of v are written]      barrier
//   mx_attn_vt, mx_attn_qk, mx_attn_bias                                         barrier (the staging image is dead: S goes over it)
//   mx_attn_scores                                                               barrier
//   mx_attn_softmax                                                              barrier
//   mx_attn_pv
// Every function is called by all 256 threads with w = wave (uniform), lane, r = lane & 15, kg = lane >> 4; the files that include
// this are built with -ffp-contract=off.
#pragma once
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

// the images of one (window, head) in attn_lds_bytes(NB, bits of F, bits of FP) bytes from `lds`; Vs, the fp32 staging of v, is S
struct MxAttnTiles {
    float* S;
    uint32_t *Qp, *Kp, *Vt, *Pp;
    uint8_t *sQ, *sK, *sV, *sP;
};
template <int NB, int F, int FP>
__device__ __forceinline__ MxAttnTiles mx_attn_tiles(uint32_t* lds) {
    constexpr int DF = hw_dwords(F), DP = hw_dwords(FP);
    constexpr int SQ = row_dwords(NB, DF), SV = row_dwords(2, DF), SP = row_dwords(2, DP);
    MxAttnTiles t;
    t.S = reinterpret_cast<float*>(lds);
    t.Qp = lds + 64 * SS;
    t.Kp = t.Qp + 64 * SQ;
    t.Vt = t.Kp + 64 * SQ;
    t.Pp = t.Vt + 64 * SV;
    t.sQ = reinterpret_cast<uint8_t*>(t.Pp + 64 * SP);
    t.sK = t.sQ + 128;
    t.sV = t.sK + 128;
    t.sP = t.sV + 128;
    return t;
}

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

// ---- Vt: blocks down the token axis.  Thread (channel, token block, half) reads 16 values down a staging column, the lane pair l, l ^ 32
// shares the block maximum, and each stores its half block of Vt.
template <int NB, int F>
__device__ __forceinline__ void mx_attn_vt(const MxAttnTiles& t, const MxFormat& f, int N, int hd, int nbn, int w, int lane) {
    constexpr int DF = hw_dwords(F), SV = row_dwords(2, DF);
    const int d = 32 * (w >> 1) + (lane & 31), tb = w & 1, half = lane >> 5;
    if ((w >> 1) < NB && tb < nbn) {                                            // uniform over the wave
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int tok = 32 * tb + 16 * half + k;
            v[k] = (d < hd && tok < N) ? t.S[tok * SS + d] : 0.f;
        }
        const unsigned sc = half_block_quant<DF, 32>(v, f, t.Vt + d * SV + tb * DF + half * (DF / 2), true);
        if (half == 0) t.sV[d * 2 + tb] = (uint8_t)(d < hd ? sc : 127u);
    }
}

// ---- raw = Qp Kp^T, one K step: wave w runs mx_mfma_step<F, F> for the 32 x 32 unit (w >> 1, w & 1) of the scores from LDS fragments.
// Returns whether the unit has a row and a column below N (uniform over the wave); acc is zero where it has not.
template <int NB, int F>
__device__ __forceinline__ bool mx_attn_qk(const MxAttnTiles& t, int N, int w, int r, int kg, f32x4 (&acc)[2][2]) {
    constexpr int DF = hw_dwords(F), SQ = row_dwords(NB, DF);
    const int ti = w >> 1, tj = w & 1;
    const bool unit = 32 * ti < N && 32 * tj < N;
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
            fa[i] = lds_fragment<DF>(t.Qp + ra * SQ, t.sQ + ra * 2, kg, NB, xa[i]);
            fb[i] = lds_fragment<DF>(t.Kp + rb * SQ, t.sK + rb * 2, kg, NB, xb[i]);
        }
        mx_mfma_step<F, F>(fa, fb, xa, xb, acc);
    }
    return unit;
}

// ---- the bias of the thread's softmax columns (row tid / 4, 16 columns from 16 (tid & 3)); 16-byte loads where bias_vec (N % 4 == 0: a
// quad lies inside the row or past it)
__device__ __forceinline__ void mx_attn_bias(const float* bias, int head, int N, int tid, bool bias_vec, float (&bs)[16]) {
    const int i = tid >> 2, j0 = 16 * (tid & 3);
    const float* brow = bias + ((long)head * N + (i < N ? i : N - 1)) * N;
    if (bias_vec) {
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

// ---- raw * scale -> S, in the accumulator layout
__device__ __forceinline__ void mx_attn_scores(float* S, const f32x4 (&acc)[2][2], float scale, int w, int r, int kg) {
    const int ti = w >> 1, tj = w & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[(32 * ti + 16 * i + 4 * kg + q) * SS + 32 * tj + 16 * j + r] = acc[i][j][q] * scale;
}

// ---- softmax rows, Pp: four threads a row, 16 CONSECUTIVE j each: s = S + (bias + mask), then softmax_rows256's arithmetic; a block of 32
// is a thread pair, its maximum one shuffle; the thread's half block of Pp is encoded in registers.  reg: the tokens' mask regions;
// scores / probs (nullable) [windows, N, N, heads] with orow the offset of (window, row 0, column 0, head).
template <int FP>
__device__ __forceinline__ void mx_attn_softmax(const MxAttnTiles& t, const MxFormat& fp, const float (&bs)[16], const int* reg, int shift, int N,
                                                int nbn, int tid, float* scores, float* probs, long orow0, int heads) {
    constexpr int DP = hw_dwords(FP), SP = row_dwords(2, DP);
    const int i = tid >> 2, part = tid & 3, blk = part >> 1;
    const bool rowok = i < N;
    const int ri = reg[rowok ? i : 0];
    const long orow = orow0 + ((long)i * N) * heads;
    float v[16];
    float mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int j = 16 * part + k;
        float sv = -3.0e38f;
        if (rowok && j < N) {
            const float bm = bs[k] + (shift > 0 && reg[j] != ri ? -100.0f : 0.f);
            sv = t.S[i * SS + j] + bm;
            if (scores) scores[orow + (long)j * heads] = sv;
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
        if (probs && rowok && j < N) probs[orow + (long)j * heads] = v[k];
    }
    const bool st = blk < nbn;
    const unsigned sc = half_block_quant<DP, 1>(v, fp, t.Pp + i * SP + blk * DP + (part & 1) * (DP / 2), st);
    if (st && !(part & 1)) t.sP[i * 2 + blk] = (uint8_t)(rowok ? sc : 127u);
}

// ---- P V, transposed: O^T = Vt Pp^T.  Wave w owns token block w and every 16-channel tile, a lane's four accumulator values are four
// consecutive channels c0 .. c0 + 3 of one token: store(tok, c0, values) for tok < N and c0 < hd.  With an FP8 operand the one-of-eight
// mask goes on the operand rdo_mx_gemm(Pp, Vt) would mask (Pp if it is FP8, else Vt).
template <int NB, int F, int FP, class Store>
__device__ __forceinline__ void mx_attn_pv(const MxAttnTiles& t, int N, int hd, int nbn, int w, int r, int kg, Store store) {
    constexpr int DF = hw_dwords(F), DP = hw_dwords(FP), SV = row_dwords(2, DF), SP = row_dwords(2, DP);
    if (16 * w < N) {
        const int tok = 16 * w + r;
        int xp;
        const i32x8 fp = lds_fragment<DP>(t.Pp + tok * SP, t.sP + tok * 2, kg, nbn, xp);
#pragma unroll
        for (int db = 0; db < 2 * NB; ++db) {
            if (16 * db >= hd) break;
            const int d = 16 * db + r;
            int xv;
            const i32x8 fv = lds_fragment<DF>(t.Vt + d * SV, t.sV + d * 2, kg, nbn, xv);
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if constexpr (DF == 8 || DP == 8) {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const i32x8 mp = DP == 8 ? keep_one_of_eight(fp, s) : fp;
                    const i32x8 mv = DP == 8 ? fv : keep_one_of_eight(fv, s);
                    o = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(mv, mp, o, F, FP, 0, xv, 0, xp);
                }
            } else {
                o = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fv, fp, o, F, FP, 0, xv, 0, xp);
            }
            // The products are complete BEFORE the store's per-lane condition: the matrix instruction reads every lane's operand
            // registers whatever EXEC says, and hipcc otherwise sinks it and the mask arithmetic into the branch of the lanes that
            // store -- the other lanes' operands are then stale registers (a head dim that is no multiple of 16: NaNs in `out`)
            asm volatile("" : "+v"(o));
            const int c0 = 16 * db + 4 * kg;                                    // the lane's four channels of token `tok`
            if (tok < N && c0 < hd) store(tok, c0, af4{o[0], o[1], o[2], o[3]});
        }
    }
}

// swin.hip's persistent grid: as many workgroups as are resident at once (registers count as well as LDS), a multiple of 8 so that a
// workgroup's items stay on one XCD; never more than there are items
template <class Kernel>
long resident_grid(Kernel kern, size_t lds, int nitems) {
    struct Memo { Kernel kern; int dev; long resident; };
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
