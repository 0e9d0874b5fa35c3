// The GDN / IGDN forward with its norm pool on the block-scaled matrix instruction, one launch (include/rdo_ptq_mxgdn.h):
//   a = mx_quant_pack(x o x),  norm = mx_gemm(a, gamma', beta'),  y = x * norm^(-+1/2)  (fp32, or quantised and packed for the next conv).
// Built with -ffp-contract=off like mx_gemm.hip and mx_chain.hip: x * x, acc + beta and x * rsqrt(norm) are separate fp32 operations.
//
// A workgroup of 256 threads owns 64 pixel rows and all C channels; the grid is ceil(rows / 64).
//
// Phase 1, producer.  Wave w reads rows 16 w .. 16 w + 15 of x as float4 (lane -> four consecutive channels, eight lanes a block, 64
//   lanes 1 KB of a row-major run), squares them and runs mx_quad_quant_store (mx_pack_store_device.h: mx_device.h's integer cast): the
//   block's packed dwords and its E8M0 byte go to LDS in the packed-operand layout of rdo_ptq_mxgemm.h, [64 rows][C / 32 blocks][bits
//   dwords] with a padded row stride, and [64][C / 32] scale bytes behind it.  Nothing of x o x or of the operand reaches memory.  A row
//   past `rows` is not read and packs zeros.  The row stride is C / 32 * bits dwords rounded up to a multiple of four and made an odd
//   number of 16-byte units: the sixteen rows a fragment load touches then start in eight different 16-byte bank groups instead of two.
// One __syncthreads.
// Phase 2, GEMM.  The 64 x C pool is cut into units of 32 rows x 32 channels -- the wave shape of mx_gemm.hip, acc[2][2] tiles of
//   16 x 16 -- and unit u = (channel block u >> 1, row half u & 1) goes to wave u % 4, so the 2 C / 32 units are dealt evenly whatever
//   C / 16 is (C = 192: three units a wave) and the two waves that share a channel block run side by side and read gamma' through the
//   same L1 lines.  A unit runs mx_gemm_accumulate's K loop: per step of 128, A fragments by load_fragment from the LDS rows (the row
//   layout is the global one, so the function is the GEMM's own), B fragments by load_fragment from global gamma' (<= 100 KB, L2
//   resident), scales likewise, one mx_mfma_step.  Equal fragments, scales and order: the accumulators are rdo_mx_gemm's bit for bit.
//   Sixteen accumulator VGPRs whatever C is; a unit whose 32 rows lie past `rows` is skipped.
// Phase 3, epilogue, per unit.  The accumulators are column-major per lane (col = lane & 15, row = 4 (lane >> 4) + reg); acc + beta goes
//   through a wave-private LDS tile [32][36 floats] (the wave-private exchange of mx_pack_store: in-order LDS, a wavefront fence) and
//   comes back as float4 rows: lane -> row 8 pass + (lane >> 3), channels 4 (lane & 7) ...  The tile write has lanes of one kg on 16
//   consecutive banks and kg on rows 4 kg apart (144 kg dwords = banks 16 kg): two lanes a bank, the least 64 dword lanes can have.
//   x is loaded again as float4 (the lines phase 1 read, L2-hot), y = x * __frsqrt_rn(n) or x * __fsqrt_rn(n) as in gdn::loss_gdn_quad,
//   and the lane stores the float4, or its eight-lane group runs mx_quad_quant_store on the block straight into global memory (the
//   unit's 32 channels are one block of the next layer's K).  norm, when asked for, is stored from the same tile.
//
// The kernel is a template over the (x o x, gamma') formats, immediates of the instruction: 25 instantiations; inverse, norm, the output
// kind and its format are run-time arguments (uniform branches in the epilogue).
#include "rdo_common.h"
#include "../../include/rdo_ptq_mxgdn.h"
#include "mx_pack_store_device.h"

namespace {

constexpr int kTileStride = 36;                                                 // floats: 32 channels + 4 of padding, float4-aligned rows

struct GdnArgs {
    const float* x;
    int rows, C, nb, stride;                                                    // nb = C / 32; stride: dwords of an LDS operand row
    MxFormat fx;
    const uint32_t* g;
    const uint8_t* sg;
    const float* beta;
    int inverse;
    float* y;                                                                   // fp32 entry
    float* norm;                                                                // nullable
    MxFormat fo;                                                                // packed entry
    uint32_t* yp;
    uint8_t* ys;
};

template <int FA, int FB>
__global__ __launch_bounds__(256) void mx_gdn_kernel(GdnArgs p) {
    constexpr int DA = hw_dwords(FA), DB = hw_dwords(FB);
    extern __shared__ uint32_t image[];                                         // [64][stride] dwords, then [64][nb] scale bytes
    __shared__ __attribute__((aligned(16))) float tiles[4][32 * kTileStride];
    uint8_t* scales = reinterpret_cast<uint8_t*>(image + 64 * p.stride);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row0 = (long)blockIdx.x * 64;
    const int C = p.C, nb = p.nb;

    // ---- phase 1: x -> x o x -> packed blocks and scale bytes in LDS ------------------------------------------------------------------
    const int quads = C >> 2;                                                   // float4 a row; a multiple of eight
    for (int it = 0; it < (C >> 4); ++it) {                                     // 16 rows x C / 4 quads over 64 lanes
        const int idx = it * 64 + lane;
        const int rl = idx / quads, c4 = idx - rl * quads;
        const int lr = 16 * wave + rl;
        const long row = row0 + lr;
        f32x4 xv = {0.f, 0.f, 0.f, 0.f};
        if (row < p.rows) xv = *reinterpret_cast<const f32x4*>(p.x + row * C + 4 * c4);
        float sq[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) sq[k] = xv[k] * xv[k];
        const int kb = c4 >> 3;
        const unsigned sc = mx_quad_quant_store(sq, p.fx, image + lr * p.stride + kb * DA, true);
        if ((c4 & 7) == 0) scales[lr * nb + kb] = (uint8_t)sc;
    }
    __syncthreads();

    // ---- phases 2 and 3, unit by unit -------------------------------------------------------------------------------------------------
    const int r = lane & 15, kg = lane >> 4;
    float* tile = tiles[wave];
    for (int u = wave; u < 2 * nb; u += 4) {
        const int m0 = 32 * (u & 1), cg = u >> 1, n0 = 32 * cg;
        if (row0 + m0 >= p.rows) continue;                                      // uniform over the wave; no barrier follows
        const uint32_t* arow[2];
        long brow[2];
        int srow[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            arow[i] = image + (m0 + 16 * i + r) * p.stride;
            srow[i] = (m0 + 16 * i + r) * nb;
            brow[i] = (long)(n0 + 16 * i + r) * nb;
        }
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < nb; k0 += 4) {                                    // mx_gemm_accumulate's loop, A from LDS
            const int kb = k0 + kg;
            const bool kok = kb < nb;
            i32x8 fa[2], fb[2];
            int xa[2], xb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = load_fragment<DA>(arow[i], k0, kg, nb, true);
                fb[i] = load_fragment<DB>(p.g + brow[i] * DB, k0, kg, nb, true);
                xa[i] = kok ? (int)scales[srow[i] + kb] : 127;
                xb[i] = kok ? (int)p.sg[brow[i] + kb] : 127;
            }
            mx_mfma_step<FA, FB>(fa, fb, xa, xb, acc);
        }

        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                  // the previous unit's tile reads precede these writes
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float bj = p.beta[n0 + 16 * j + r];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) tile[(16 * i + 4 * kg + q) * kTileStride + 16 * j + r] = acc[i][j][q] + bj;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int s = lane & 7;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int t = 8 * pass + (lane >> 3);
            const long row = row0 + m0 + t;
            const bool live = row < p.rows;
            const long at = row * C + n0 + 4 * s;
            const f32x4 nv = *reinterpret_cast<const f32x4*>(tile + t * kTileStride + 4 * s);
            f32x4 xv = {0.f, 0.f, 0.f, 0.f};
            if (live) xv = *reinterpret_cast<const f32x4*>(p.x + at);
            float yv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) yv[k] = xv[k] * (p.inverse ? __fsqrt_rn(nv[k]) : __frsqrt_rn(nv[k]));
            if (live && p.norm) *reinterpret_cast<f32x4*>(p.norm + at) = nv;
            if (p.yp) {
                const long blk = row * nb + cg;
                const unsigned sc = mx_quad_quant_store(yv, p.fo, p.yp + blk * p.fo.bits, live);
                if (live && s == 0) p.ys[blk] = (uint8_t)sc;
            } else if (live) {
                *reinterpret_cast<f32x4*>(p.y + at) = f32x4{yv[0], yv[1], yv[2], yv[3]};
            }
        }
    }
}

using GdnKernel = void (*)(GdnArgs);

#define RDO_MXGDN_ROW(FA) {mx_gdn_kernel<FA, 0>, mx_gdn_kernel<FA, 1>, mx_gdn_kernel<FA, 2>, mx_gdn_kernel<FA, 3>, mx_gdn_kernel<FA, 4>}
const GdnKernel kGdn[5][5] = {RDO_MXGDN_ROW(0), RDO_MXGDN_ROW(1), RDO_MXGDN_ROW(2), RDO_MXGDN_ROW(3), RDO_MXGDN_ROW(4)};
#undef RDO_MXGDN_ROW

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// what both entries check of their inputs; fills everything of `a` but the outputs
int gdn_check(const char* who, const float* x, int32_t rows, int32_t C, int32_t x2_format, const void* g, const uint8_t* g_scales,
              int32_t g_format, const float* beta, int32_t inverse, const float* norm, GdnArgs& a, MxFormat& fg) {
    RDO_REQUIRE(x && g && g_scales && beta, "%s: null pointer", who);
    RDO_REQUIRE(rows > 0 && C > 0, "%s: non-positive size rows %d C %d", who, (int)rows, (int)C);
    RDO_REQUIRE(C % kBlock == 0, "%s: C %d is no multiple of the block size %d", who, (int)C, kBlock);
    RDO_REQUIRE(C <= RDO_MXGDN_MAX_C, "%s: C %d is above %d, the most whose 64-row operand fits the kernel's LDS", who, (int)C,
                RDO_MXGDN_MAX_C);
    RDO_REQUIRE(mx_format(x2_format, a.fx), "%s: unknown x2_format %d (0 .. %d)", who, (int)x2_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(mx_format(g_format, fg), "%s: unknown g_format %d (0 .. %d)", who, (int)g_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(inverse == 0 || inverse == 1, "%s: inverse %d is neither 0 (GDN) nor 1 (IGDN)", who, (int)inverse);
    RDO_REQUIRE(aligned4(g) && aligned4(beta), "%s: g and beta must be 4-byte aligned", who);
    RDO_REQUIRE(aligned16(x) && aligned16(norm), "%s: x, y and norm must be 16-byte aligned", who);
    a.x = x;
    a.rows = rows;
    a.C = C;
    a.nb = C / kBlock;
    int stride = (a.nb * a.fx.bits + 3) & ~3;
    if (((stride >> 2) & 1) == 0) stride += 4;
    a.stride = stride;
    a.g = static_cast<const uint32_t*>(g);
    a.sg = g_scales;
    a.beta = beta;
    a.inverse = inverse;
    a.norm = const_cast<float*>(norm);
    a.y = nullptr;
    a.yp = nullptr;
    a.ys = nullptr;
    a.fo = a.fx;
    return RDO_OK;
}

int gdn_launch(const char* tag, const GdnArgs& a, int32_t x2_format, int32_t g_format, const MxFormat& fg, double out_bytes, void* stream) {
    const GdnKernel kern = kGdn[hw_format(x2_format)][hw_format(g_format)];
    const unsigned grid = (unsigned)rdo::ceil_div(a.rows, 64);
    const size_t lds = (size_t)64 * a.stride * 4 + (size_t)64 * a.nb;
    const double elems = (double)a.rows * a.C;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, a);
            return rdo::check_launch(tag);
        },
        stream, tag, 2.0 * elems * a.C,
        elems * 4.0 + (double)a.C * a.nb * (4.0 * fg.bits + 1.0) + a.C * 4.0 + out_bytes + (a.norm ? elems * 4.0 : 0.0));
}

}  // namespace

extern "C" {

int rdo_mx_gdn(const float* x, int32_t rows, int32_t C, int32_t x2_format, const void* g, const uint8_t* g_scales, int32_t g_format,
               const float* beta, int32_t inverse, float* y, float* norm, void* stream) {
    const char* who = "rdo_mx_gdn";
    RDO_REQUIRE(y, "%s: null pointer", who);
    GdnArgs a;
    MxFormat fg;
    if (const int rc = gdn_check(who, x, rows, C, x2_format, g, g_scales, g_format, beta, inverse, norm, a, fg)) return rc;
    RDO_REQUIRE(aligned16(y), "%s: x, y and norm must be 16-byte aligned", who);
    a.y = y;
    return gdn_launch("mx_gdn", a, x2_format, g_format, fg, (double)rows * C * 4.0, stream);
}

int rdo_mx_gdn_packed(const float* x, int32_t rows, int32_t C, int32_t x2_format, const void* g, const uint8_t* g_scales, int32_t g_format,
                      const float* beta, int32_t inverse, int32_t out_format, void* y_packed, uint8_t* y_scales, float* norm, void* stream) {
    const char* who = "rdo_mx_gdn_packed";
    RDO_REQUIRE(y_packed && y_scales, "%s: null pointer", who);
    GdnArgs a;
    MxFormat fg;
    if (const int rc = gdn_check(who, x, rows, C, x2_format, g, g_scales, g_format, beta, inverse, norm, a, fg)) return rc;
    RDO_REQUIRE(mx_format(out_format, a.fo), "%s: unknown out_format %d (0 .. %d)", who, (int)out_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(aligned4(y_packed), "%s: y_packed must be 4-byte aligned", who);
    a.yp = static_cast<uint32_t*>(y_packed);
    a.ys = y_scales;
    return gdn_launch("mx_gdn_packed", a, x2_format, g_format, fg, (double)rows * a.nb * (4.0 * a.fo.bits + 1.0), stream);
}

}  // extern "C"
