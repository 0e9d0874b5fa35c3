// The packed-output epilogue of the block-scaled kernels (include/rdo_ptq_mxchain.h), stated once for mx_gemm.hip, mx_conv.hip and
// mx_tconv.hip: a wave's 32 x 32 accumulators -> bias, activation, one MX block per output row (n0 % 32 == 0: the wave's 32 channels ARE
// block n0 / 32 of the row) -> the packed dwords and the E8M0 byte rdo_mx_quant_pack writes from the fp32 result, bit for bit.  No
// fp32 tile reaches memory.  The files that include it are built with -ffp-contract=off: v = acc + bias and 0.01f * v round as the
// un-fused kernels' (mx_store_tiles; lrelu_fwd_kernel of elementwise.hip).
//
// Register layout in: lane (r = lane & 15, kg = lane >> 4) holds acc[i][j][q] = row 16 i + 4 kg + q, channel 16 j + r.
//   1. v = act(acc + bias[channel]) in fp32.
//   2. Block maximum of row (i, kg, q): the unsigned max of the sign-cleared patterns over j, then over the 16 lanes that share kg --
//      one DPP row (row_ror 8, 4, 2, 1: a rotation reduce leaves the maximum in every lane of the row), no LDS, no ds_bpermute.
//      E = mx_block_exponent(amax); a block that holds a NaN or an infinity gets the scale byte 255 and zero codes.
//   3. Sixteen codes a lane: mx_encode(mag, E) | sign >> (32 - bits) -- mx_device.h's functions, unchanged.
//   4. The registers are channel-minor ACROSS lanes, the packed block is channel-minor INSIDE dwords: transpose through a wave-private
//      LDS tile [32 rows][36 bytes] -- 32 code bytes, the row's scale byte at 32, 3 bytes of padding.  Each lane writes its sixteen
//      codes as bytes (lanes r == 0 also the scale byte); then lane L reads the sixteen codes of row L >> 1, half L & 1, as four dwords
//      and squeezes them into bits / 2 dwords (16 codes x 4 / 6 / 8 bits = 2 / 3 / 4 whole dwords: no dword straddles the halves).
//      Bank conflicts with the row stride of 9 dwords: one byte-store instruction has 64 lanes in four runs (one per kg) of 4
//      consecutive dwords, four lanes to a dword, starting at dwords 36 kg + const = banks 4 kg + const (mod 32; 0, 36, 8, 44 mod 64):
//      disjoint runs, 0 conflicts.  One dword-read instruction has lane L at dword 9 (L >> 1) + 4 (L & 1) + d: 9 is odd, so the even
//      lanes cover every one of 32 banks once and so do the odd ones -- 2 lanes a bank, the least 64 lanes x 4 bytes can have on 32
//      banks, 0 conflicts beyond it.
//      The exchange stays inside the wave: the kernels return per wave before it (a ragged tile) and have no workgroup barrier.  The
//      LDS unit runs one wave's instructions in order, so the reads follow the writes; the wavefront fence keeps the compiler from
//      reordering them.
//   5. Lane L stores its bits / 2 dwords to packed[(row N / 32 + n0 / 32) bits + (L & 1) bits / 2 ...] (4-byte stores), lane L even
//      the scale byte to scales[row N / 32 + n0 / 32]; `row_of` maps a tile row 0 .. 31 to the packed row (the output pixel) or to
//      -1 past the last row, which stores nothing.
#pragma once
#include "../../include/rdo_ptq_mxchain.h"
#include "mx_mfma_device.h"

namespace {

// where the packed variants write: the output format by value as in mx_quant_pack_kernel, the activation id, the two outputs
struct MxPackedOut {
    MxFormat f;
    int act;
    uint32_t* packed;
    uint8_t* scales;
};

constexpr int kPackRowDwords = 9;                                               // 36 bytes: 32 codes, the scale byte, padding

__device__ __forceinline__ float mx_act(float v, int act) {
    if (act == RDO_MX_ACT_LRELU) return v > 0.f ? v : 0.01f * v;
    if (act == RDO_MX_ACT_RELU) return v > 0.f ? v : 0.f;
    return v;
}

// max over the DPP row (16 lanes) of `v`, in every lane of the row
__device__ __forceinline__ unsigned row16_max(unsigned v) {
#define RDO_ROR_MAX(ctrl)                                                                             \
    {                                                                                                 \
        const unsigned u = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xF, 0xF, false);   \
        v = u > v ? u : v;                                                                            \
    }
    RDO_ROR_MAX(0x128)                                                          // row_ror:8
    RDO_ROR_MAX(0x124)                                                          // row_ror:4
    RDO_ROR_MAX(0x122)                                                          // row_ror:2
    RDO_ROR_MAX(0x121)                                                          // row_ror:1
#undef RDO_ROR_MAX
    return v;
}

// the four code bytes of `w` as 4 x 4 = 16 bits / 4 x 6 = 24 bits, element 0 lowest
__device__ __forceinline__ unsigned squeeze4(unsigned w) {
    return (w & 0xFu) | ((w >> 4) & 0xF0u) | ((w >> 8) & 0xF00u) | ((w >> 12) & 0xF000u);
}
__device__ __forceinline__ unsigned squeeze6(unsigned w) {
    return (w & 0x3Fu) | ((w >> 2) & 0xFC0u) | ((w >> 4) & 0x3F000u) | ((w >> 6) & 0xFC0000u);
}

// Steps 2 .. 4 on the wave's 32 x 32 values v (the register layout above): lane L ends with the bits / 2 dwords d[] of half h = L & 1 of
// tile row t = L >> 1 and the row's scale byte, and hands them to put(t, h, d, scale) -- step 5, or an LDS operand tile (mx_swin.hip).
template <class Put>
__device__ __forceinline__ void mx_pack_tile(const f32x4 (&v)[2][2], const MxFormat& f, Put put) {
    __shared__ uint32_t tiles[4][32 * kPackRowDwords];                         // one tile a wave, 4608 bytes a workgroup
    const int lane = threadIdx.x & 63, r = lane & 15, kg = lane >> 4;
    uint32_t* tile = tiles[threadIdx.x >> 6];
    uint8_t* bytes = reinterpret_cast<uint8_t*>(tile);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned pat[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float e = v[i][j][q];                                     // a copy: bit_cast of a vector element takes the vector's address
                pat[j] = __builtin_bit_cast(unsigned, e);
            }
            const unsigned m0 = pat[0] & 0x7FFFFFFFu, m1 = pat[1] & 0x7FFFFFFFu;
            const unsigned amax = row16_max(m0 > m1 ? m0 : m1);
            const bool finite = amax < 0x7F800000u;
            const int E = finite ? mx_block_exponent(amax, f) : -127;
            uint8_t* row = bytes + (16 * i + 4 * kg + q) * (4 * kPackRowDwords);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned code = finite ? mx_encode(pat[j] & 0x7FFFFFFFu, E, f) | ((pat[j] & 0x80000000u) >> (32 - f.bits)) : 0u;
                row[16 * j + r] = (uint8_t)code;
            }
            if (r == 0) row[32] = (uint8_t)(finite ? E + 127 : 255);
        }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int t = lane >> 1, h = lane & 1;
    const uint32_t* src = tile + t * kPackRowDwords;
    unsigned c[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) c[d] = src[4 * h + d];
    const unsigned scale = src[8] & 0xFFu;
    unsigned d[4] = {c[0], c[1], c[2], c[3]};
    if (f.bits == 4) {
        d[0] = squeeze4(c[0]) | (squeeze4(c[1]) << 16);
        d[1] = squeeze4(c[2]) | (squeeze4(c[3]) << 16);
    } else if (f.bits == 6) {
        const unsigned p0 = squeeze6(c[0]), p1 = squeeze6(c[1]), p2 = squeeze6(c[2]), p3 = squeeze6(c[3]);
        d[0] = p0 | (p1 << 24);
        d[1] = (p1 >> 8) | (p2 << 16);
        d[2] = (p2 >> 16) | (p3 << 8);
    }
    put(t, h, d, scale);
}

// the lane's bits / 2 dwords of mx_pack_tile to dst[0 ..]
__device__ __forceinline__ void mx_put_dwords(uint32_t* dst, const unsigned (&d)[4], int bits) {
    dst[0] = d[0];
    dst[1] = d[1];
    if (bits >= 6) dst[2] = d[2];
    if (bits == 8) dst[3] = d[3];
}

template <class RowOf>
__device__ __forceinline__ void mx_pack_store(const f32x4 (&acc)[2][2], const float* __restrict__ bias, const MxPackedOut& o, long n0, int N,
                                              RowOf row_of) {
    const int r = threadIdx.x & 15;
    f32x4 v[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float bj = bias ? bias[n0 + 16 * j + r] : 0.f;                    // n0 + 31 < N: N % 32 == 0
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[i][j][q] = mx_act(acc[i][j][q] + bj, o.act);
    }
    mx_pack_tile(v, o.f, [&](int t, int h, const unsigned (&d)[4], unsigned scale) {
        const long row = row_of(t);
        if (row < 0) return;
        const long blk = row * (N / kBlock) + n0 / kBlock;
        mx_put_dwords(o.packed + blk * o.f.bits + h * (o.f.bits >> 1), d, o.f.bits);
        if (h == 0) o.scales[blk] = (uint8_t)scale;
    });
}

// The row-major form of the same quantiser, for a kernel whose lanes hold four consecutive channels of a row (mx_gdn.hip: the x o x
// producer and the packed epilogue): the eight lanes 8 t .. 8 t + 7 of a wave hold one block, lane s = lane & 7 its elements 4 s ..
// 4 s + 3 in v.  Block maximum by three xor shuffles inside the eight; mx_block_exponent / mx_encode as above; the lane's four codes are
// 16 / 24 / 32 consecutive bits of the block's bit string, put into whole dwords by one more shuffle (FP4: a lane pair makes a dword;
// FP6: four lanes make three) and stored to dst[0 .. bits - 1], the block's packed image in global memory or LDS.  Returns the scale
// byte (255 and zero codes for a block that holds a NaN or an infinity).  Called by all 64 lanes; `live` guards the stores alone.
__device__ __forceinline__ unsigned mx_quad_quant_store(const float (&v)[4], const MxFormat& f, uint32_t* dst, bool live) {
    const int lane = threadIdx.x & 63, s = lane & 7;
    unsigned pat[4], amax = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pat[k] = __builtin_bit_cast(unsigned, v[k]);
        const unsigned m = pat[k] & 0x7FFFFFFFu;
        amax = m > amax ? m : amax;
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        const unsigned u = __shfl_xor(amax, o, 64);
        amax = u > amax ? u : amax;
    }
    const bool finite = amax < 0x7F800000u;
    const int E = finite ? mx_block_exponent(amax, f) : -127;
    unsigned w = 0u;
    if (finite) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w |= (mx_encode(pat[k] & 0x7FFFFFFFu, E, f) | ((pat[k] & 0x80000000u) >> (32 - f.bits))) << (k * f.bits);
    }
    if (f.bits == 8) {
        if (live) dst[s] = w;
    } else if (f.bits == 4) {
        const unsigned hi = __shfl_xor(w, 1, 64);
        if (live && !(s & 1)) dst[s >> 1] = w | (hi << 16);
    } else {
        const unsigned next = __shfl(w, (lane + 1) & 63, 64);                   // (lane 3 of a four stores nothing: its `next` is unused)
        const int i = s & 3;
        if (live && i < 3) dst[3 * (s >> 2) + i] = (w >> (8 * i)) | (next << (24 - 8 * i));
    }
    return finite ? (unsigned)(E + 127) : 255u;
}

// what every packed entry checks beyond its fp32 twin; the message starts with `who`
inline int mx_packed_out_check(const char* who, int32_t out_format, int32_t act, int64_t N, void* y_packed, uint8_t* y_scales,
                               MxPackedOut& o) {
    RDO_REQUIRE(y_packed && y_scales, "%s: null output pointer", who);
    RDO_REQUIRE(aligned4(y_packed), "%s: y_packed must be 4-byte aligned", who);
    RDO_REQUIRE(mx_format(out_format, o.f), "%s: unknown out_format %d (0 .. %d)", who, (int)out_format, RDO_MX_FORMATS - 1);
    RDO_REQUIRE(act == RDO_MX_ACT_NONE || act == RDO_MX_ACT_LRELU || act == RDO_MX_ACT_RELU,
                "%s: unknown act %d (0 none, 1 LeakyReLU(0.01), 2 ReLU)", who, (int)act);
    RDO_REQUIRE(N > 0 && N % kBlock == 0, "%s: N %lld is no multiple of the block size %d: the output's blocks run along N", who,
                (long long)N, kBlock);
    o.act = act;
    o.packed = static_cast<uint32_t*>(y_packed);
    o.scales = y_scales;
    return RDO_OK;
}

}  // namespace
