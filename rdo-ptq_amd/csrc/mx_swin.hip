// The LayerNorm producer and the MLP half of a Swin transformer block on the block-scaled matrix instruction (include/rdo_ptq_mxswin.h):
//   rdo_mx_layer_norm_pack:  ln = LN(a + b) -> mx_quant_pack(ln)                                   (norm1 -> qkv: the producer of the GEMM)
//   rdo_mx_swin_mlp:         out = (a + b) + mx_gemm(mx_quant_pack(gelu(mx_gemm(mx_quant_pack(ln), W1, b1))), W2, b2), one launch
// Built with -ffp-contract=off like mx_gemm.hip, mx_chain.hip and mx_gdn.hip: acc + bias, gelu's products and s + y are separate fp32
// operations; the LayerNorm row states its own arithmetic (ln_row_device.h).
//
// Row phase, shared by both kernels (ln_pack_row, mx_swin_device.h; unit_accumulate is there as well).  add_ln_kernel's layout: 16 lanes a row, lane l16 holds float4 l16 + 16 k.  A 32-channel
//   MX block is then the eight neighbouring lanes 8 t .. 8 t + 7 of one k -- block 2 k + (l16 >> 3) -- which is what mx_quad_quant_store
//   (mx_pack_store_device.h) quantises and places: the LayerNorm never leaves the registers between ln_row and the packed dwords.  A row
//   past `rows` is not read; its codes in an LDS image are zeros.
//
// mx_ln_pack_kernel<VPL>: 256 threads = 16 rows a pass, grid-stride over row groups, straight to global memory.  No LDS, no barrier.
//
// mx_swin_mlp_kernel<VPL, FA, FB>: a workgroup of 256 threads owns 64 token rows; the grid is ceil(rows / 64).  Dynamic LDS:
//   image A  [64][strideA] dwords   the packed ln tile, K = C            scales A [64][C / 32] bytes
//   image H  [64][strideH] dwords   the packed hidden tile, K = Hd       scales H [64][Hd / 32] bytes
//   (row strides by mx_gdn.hip's rule: blocks * bits dwords rounded up to four and made an odd number of 16-byte units), beside the
//   4 608 B of mx_pack_tile's static wave-private byte tiles.  In FP8, dynamic + static bytes: C = 192 / Hd = 384: 40 064 + 4 608 =
//   44 672; C = 320 / Hd = 640: 65 408 + 4 608 = 70 016; C = 512 / Hd = 1024: 103 424 + 4 608 = 108 032 (gfx950 has 163 840 a workgroup;
//   where the sum is above 65 536 the launch raises the kernel's dynamic-LDS attribute).
// Phase 1.  Four passes of the row phase (rows 16 pass + thread / 16) write image A and scales A.           __syncthreads.
// Phase 2.  2 Hd / 32 units of 32 rows x 32 hidden channels, unit u = (channel block u >> 1, row half u & 1) to wave u % 4.  A unit runs
//   mx_gemm_accumulate's loop (A fragments from image A, B from global W1: L2 resident), then in the accumulator layout v = acc + b1
//   (-> pre), g = gelu(v), and mx_pack_tile quantises the unit's 32 x 32 values -- one MX block a row -- and hands every lane its dwords:
//   they go to image H / scales H (and to `hidden` when asked).                                            __syncthreads.
// Phase 3.  2 C / 32 units likewise from image H against W2; y = acc + b2, s = a (+ b) read again (the lines phase 1 read), out = s + y,
//   stored in the accumulator layout as mx_store_tiles does.
// Ragged tiles: no thread returns or skips a barrier.  A unit whose 32 rows lie past `rows` is skipped by its wave between the barriers
// (its rows of image H are then neither written nor read); rows past `rows` inside a unit are zero codes and store nothing.
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxswin.h"
#include "mx_swin_device.h"

namespace {

struct LnPackArgs {
    const ln4 *a, *b, *w, *bias;                                                // b, w, bias nullable
    int rows, C4, nb;
    float eps;
    MxFormat f;
    uint32_t* packed;
    uint8_t* scales;
    ln4 *sum_out, *ln;                                                          // nullable
};

template <int VPL>
__global__ __launch_bounds__(256) void mx_ln_pack_kernel(LnPackArgs p) {
    const int l16 = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const float invC = 1.f / (float)(4 * p.C4);
    for (long row0 = (long)blockIdx.x * 16; row0 < p.rows; row0 += (long)gridDim.x * 16) {
        const long row = row0 + grp;
        ln_pack_row<VPL>(p.a, p.b, p.w, p.bias, p.C4, l16, invC, p.eps, row, row < p.rows, false, p.sum_out, p.ln, p.f,
                         p.packed + row * p.nb * p.f.bits, p.scales + row * p.nb);
    }
}

struct SwinMlpArgs {
    const ln4 *a, *b, *lw, *lb;                                                 // b, lw, lb nullable
    float eps;
    int rows, C, Hd, nbC, nbH, strideA, strideH;                                // strides: dwords of an LDS operand row
    MxFormat fa;                                                                // the activation format
    const uint32_t *w1, *w2;
    const uint8_t *s1, *s2;
    const float *b1, *b2;                                                       // nullable
    float *out, *ln, *pre;                                                      // ln, pre nullable
    uint32_t* hidden;                                                           // nullable, with hs
    uint8_t* hs;
};

template <int VPL, int FA, int FB>
__global__ __launch_bounds__(256) void mx_swin_mlp_kernel(SwinMlpArgs p) {
    extern __shared__ uint32_t lds[];
    uint32_t* imageA = lds;
    uint32_t* imageH = imageA + 64 * p.strideA;
    uint8_t* scalesA = reinterpret_cast<uint8_t*>(imageH + 64 * p.strideH);
    uint8_t* scalesH = scalesA + 64 * p.nbC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row0 = (long)blockIdx.x * 64;
    const int C = p.C, Hd = p.Hd, nbC = p.nbC, nbH = p.nbH, bits = p.fa.bits;

    // ---- phase 1: LN(a + b) -> packed blocks and scale bytes of image A ---------------------------------------------------------------
    {
        const int l16 = threadIdx.x & 15, grp = threadIdx.x >> 4, C4 = C >> 2;
        const float invC = 1.f / (float)C;
        for (int pass = 0; pass < 4; ++pass) {
            const int lr = 16 * pass + grp;
            const long row = row0 + lr;
            ln_pack_row<VPL>(p.a, p.b, p.lw, p.lb, C4, l16, invC, p.eps, row, row < p.rows, true, nullptr, reinterpret_cast<ln4*>(p.ln), p.fa,
                             imageA + lr * p.strideA, scalesA + lr * nbC);
        }
    }
    __syncthreads();

    // ---- phase 2: pre = ln W1^T + b1, hidden = pack(gelu(pre)) -> image H -------------------------------------------------------------
    const int r = lane & 15, kg = lane >> 4;
    for (int u = wave; u < 2 * nbH; u += 4) {
        const int m0 = 32 * (u & 1), hb = u >> 1, n0 = 32 * hb;
        if (row0 + m0 >= p.rows) continue;                                      // uniform over the wave; no barrier inside the loop
        f32x4 acc[2][2], g[2][2];
        unit_accumulate<FA, FB>(imageA, p.strideA, scalesA, nbC, p.w1, p.s1, m0, n0, r, kg, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + 16 * j + r;
            const float bj = p.b1 ? p.b1[col] : 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long row = row0 + m0 + 16 * i + 4 * kg + q;
                    const bool live = row < p.rows;
                    const float v = acc[i][j][q] + bj;
                    if (live && p.pre) p.pre[row * Hd + col] = v;
                    g[i][j][q] = live ? rdo::gelu(v) : 0.f;
                }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                  // the previous unit's byte-tile reads precede these writes
        __builtin_amdgcn_wave_barrier();
        mx_pack_tile(g, p.fa, [&](int t, int h, const unsigned (&d)[4], unsigned scale) {
            const int lr = m0 + t;
            const long row = row0 + lr;
            mx_put_dwords(imageH + lr * p.strideH + hb * bits + h * (bits >> 1), d, bits);
            if (h == 0) scalesH[lr * nbH + hb] = (uint8_t)scale;
            if (p.hidden && row < p.rows) {
                const long blk = row * nbH + hb;
                mx_put_dwords(p.hidden + blk * bits + h * (bits >> 1), d, bits);
                if (h == 0) p.hs[blk] = (uint8_t)scale;
            }
        });
    }
    __syncthreads();

    // ---- phase 3: out = (a + b) + (hidden W2^T + b2) ----------------------------------------------------------------------------------
    const float* af = reinterpret_cast<const float*>(p.a);
    const float* bf = reinterpret_cast<const float*>(p.b);
    for (int u = wave; u < 2 * nbC; u += 4) {
        const int m0 = 32 * (u & 1), n0 = 32 * (u >> 1);
        if (row0 + m0 >= p.rows) continue;
        f32x4 acc[2][2];
        unit_accumulate<FA, FB>(imageH, p.strideH, scalesH, nbH, p.w2, p.s2, m0, n0, r, kg, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + 16 * j + r;
            const float bj = p.b2 ? p.b2[col] : 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long row = row0 + m0 + 16 * i + 4 * kg + q;
                    if (row >= p.rows) continue;
                    const long at = row * C + col;
                    const float y = acc[i][j][q] + bj;
                    float s = af[at];
                    if (bf) s = s + bf[at];
                    p.out[at] = s + y;
                }
        }
    }
}

using MlpKernel = void (*)(SwinMlpArgs);

// [row-phase width: VPL 3 / 5 / 8 as add_ln_kernel's dispatch][activation format][weight format]
#define RDO_MXSWIN_ROW(V, FA) \
    {mx_swin_mlp_kernel<V, FA, 0>, mx_swin_mlp_kernel<V, FA, 1>, mx_swin_mlp_kernel<V, FA, 2>, mx_swin_mlp_kernel<V, FA, 3>, mx_swin_mlp_kernel<V, FA, 4>}
#define RDO_MXSWIN_VPL(V) {RDO_MXSWIN_ROW(V, 0), RDO_MXSWIN_ROW(V, 1), RDO_MXSWIN_ROW(V, 2), RDO_MXSWIN_ROW(V, 3), RDO_MXSWIN_ROW(V, 4)}
const MlpKernel kMlp[3][5][5] = {RDO_MXSWIN_VPL(3), RDO_MXSWIN_VPL(5), RDO_MXSWIN_VPL(8)};
#undef RDO_MXSWIN_VPL
#undef RDO_MXSWIN_ROW

// LDS of a workgroup beside the dynamic part: mx_pack_tile's four wave-private byte tiles
constexpr size_t kStaticLds = 4 * 32 * kPackRowDwords * sizeof(uint32_t);

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

int rdo_mx_layer_norm_pack(const float* a, const float* b, const float* weight, const float* bias, int32_t rows, int32_t C, float eps,
                           int32_t format, void* out_packed, uint8_t* out_scales, float* sum_out, float* ln, void* stream) {
    const char* who = "rdo_mx_layer_norm_pack";
    RDO_REQUIRE(a && out_packed && out_scales, "%s: null pointer", who);
    RDO_REQUIRE(rows > 0, "%s: non-positive rows %d", who, (int)rows);
    RDO_REQUIRE(C > 0 && C % kBlock == 0, "%s: C %d is no positive multiple of the block size %d", who, (int)C, kBlock);
    RDO_REQUIRE(C <= RDO_MXSWIN_MAX_C, "%s: C %d is above %d", who, (int)C, RDO_MXSWIN_MAX_C);
    LnPackArgs p;
    RDO_REQUIRE(mx_format(format, p.f), "%s: unknown format %d (0 .. %d)", who, (int)format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(!sum_out || b, "%s: sum_out without a second addend", who);
    RDO_REQUIRE(aligned16(a) && aligned16(b) && aligned16(weight) && aligned16(bias) && aligned16(sum_out) && aligned16(ln),
                "%s: a, b, weight, bias, sum_out and ln must be 16-byte aligned", who);
    RDO_REQUIRE(aligned4(out_packed), "%s: out_packed must be 4-byte aligned", who);
    p.a = reinterpret_cast<const ln4*>(a);
    p.b = reinterpret_cast<const ln4*>(b);
    p.w = reinterpret_cast<const ln4*>(weight);
    p.bias = reinterpret_cast<const ln4*>(bias);
    p.rows = rows;
    p.C4 = C / 4;
    p.nb = C / kBlock;
    p.eps = eps;
    p.packed = static_cast<uint32_t*>(out_packed);
    p.scales = out_scales;
    p.sum_out = reinterpret_cast<ln4*>(sum_out);
    p.ln = reinterpret_cast<ln4*>(ln);
    long blocks = rdo::ceil_div((long)rows, 16L);
    if (blocks > 4096) blocks = 4096;
    const double elems = (double)rows * C;
    return rdo::dispatch(
        [=](hipStream_t s) {
            auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, p); };
            if (p.C4 <= 48) go(mx_ln_pack_kernel<3>);
            else if (p.C4 <= 80) go(mx_ln_pack_kernel<5>);
            else go(mx_ln_pack_kernel<8>);
            return rdo::check_launch("mx_layer_norm_pack");
        },
        stream, "mx_layer_norm_pack", 0.0,
        elems * 4.0 * (1.0 + (b ? 1.0 : 0.0) + (sum_out ? 1.0 : 0.0) + (ln ? 1.0 : 0.0)) + (double)rows * p.nb * (4.0 * p.f.bits + 1.0));
}

int rdo_mx_swin_mlp(const float* a, const float* b, const float* ln_weight, const float* ln_bias, float eps, int32_t rows, int32_t C,
                    int32_t Hd, int32_t act_format, const void* w1, const uint8_t* w1_scales, const float* b1, const void* w2,
                    const uint8_t* w2_scales, const float* b2, int32_t w_format, float* out, float* ln, float* pre, void* hidden,
                    uint8_t* hidden_scales, void* stream) {
    const char* who = "rdo_mx_swin_mlp";
    RDO_REQUIRE(a && w1 && w1_scales && w2 && w2_scales && out, "%s: null pointer", who);
    RDO_REQUIRE(rows > 0, "%s: non-positive rows %d", who, (int)rows);
    RDO_REQUIRE(C > 0 && C % kBlock == 0 && Hd > 0 && Hd % kBlock == 0, "%s: C %d or Hd %d is no positive multiple of the block size %d", who,
                (int)C, (int)Hd, kBlock);
    RDO_REQUIRE(C <= RDO_MXSWIN_MAX_C && Hd <= RDO_MXSWIN_MAX_HIDDEN, "%s: C %d is above %d or Hd %d above %d, the most whose 64-row operands fit the kernel's LDS",
                who, (int)C, RDO_MXSWIN_MAX_C, (int)Hd, RDO_MXSWIN_MAX_HIDDEN);
    SwinMlpArgs p;
    MxFormat fw;
    RDO_REQUIRE(mx_format(act_format, p.fa), "%s: unknown act_format %d (0 .. %d)", who, (int)act_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(mx_format(w_format, fw), "%s: unknown w_format %d (0 .. %d)", who, (int)w_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE((hidden == nullptr) == (hidden_scales == nullptr), "%s: hidden and hidden_scales go together", who);
    RDO_REQUIRE(aligned16(a) && aligned16(b) && aligned16(ln_weight) && aligned16(ln_bias) && aligned16(b1) && aligned16(b2) && aligned16(out) &&
                    aligned16(ln) && aligned16(pre),
                "%s: a, b, ln_weight, ln_bias, b1, b2, out, ln and pre must be 16-byte aligned", who);
    RDO_REQUIRE(aligned4(w1) && aligned4(w2) && aligned4(hidden), "%s: w1, w2 and hidden must be 4-byte aligned", who);
    p.a = reinterpret_cast<const ln4*>(a);
    p.b = reinterpret_cast<const ln4*>(b);
    p.lw = reinterpret_cast<const ln4*>(ln_weight);
    p.lb = reinterpret_cast<const ln4*>(ln_bias);
    p.eps = eps;
    p.rows = rows;
    p.C = C;
    p.Hd = Hd;
    p.nbC = C / kBlock;
    p.nbH = Hd / kBlock;
    p.strideA = lds_row_dwords(p.nbC, p.fa.bits);
    p.strideH = lds_row_dwords(p.nbH, p.fa.bits);
    p.w1 = static_cast<const uint32_t*>(w1);
    p.w2 = static_cast<const uint32_t*>(w2);
    p.s1 = w1_scales;
    p.s2 = w2_scales;
    p.b1 = b1;
    p.b2 = b2;
    p.out = out;
    p.ln = ln;
    p.pre = pre;
    p.hidden = static_cast<uint32_t*>(hidden);
    p.hs = hidden_scales;
    const MlpKernel kern = kMlp[C <= 192 ? 0 : C <= 320 ? 1 : 2][hw_format(act_format)][hw_format(w_format)];
    const unsigned grid = (unsigned)rdo::ceil_div(rows, 64);
    const size_t lds = (size_t)64 * 4 * (p.strideA + p.strideH) + (size_t)64 * (p.nbC + p.nbH);
    // the workgroup's whole LDS, static tiles included, decides: C = 320 / Hd = 640 in FP8 is 65 408 B dynamic, 70 016 B in all
    if (lds + kStaticLds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return rdo::set_error(RDO_EHIP, "%s: hipFuncSetAttribute(%zu B LDS) failed", who, lds);
    const double tokens = (double)rows, wbytes = 2.0 * p.nbC * Hd * (4.0 * fw.bits + 1.0);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, p);
            return rdo::check_launch("mx_swin_mlp");
        },
        stream, "mx_swin_mlp", 4.0 * tokens * C * Hd,
        tokens * C * 4.0 * ((b ? 4.0 : 2.0) + 1.0 + (ln ? 1.0 : 0.0)) + wbytes + (pre ? tokens * Hd * 4.0 : 0.0) +
            (hidden ? tokens * p.nbH * (4.0 * p.fa.bits + 1.0) : 0.0));
}

}  // extern "C"
