// The learned-rounding step on the MX grids for every weight tensor of a unit (include/rdo_ptq_mxroundbatch.h): what adaround.hip's
// batched step is on the integer grids.  Built with -ffp-contract=off, like mx_round.hip, whose single-tensor step it reproduces bit
// for bit: both run ada_element (ada_device.h) on an MxGrid (mx_grid_device.h) and sum the slabs with slab_sum.
//
// Two launches.
//   mx_step_batch_kernel   Workgroups are dealt to tensors by a blk_end table; behind the step's own come the workgroups of the next
//       iteration's gather (gather_body.h).  A step workgroup walks runs of 1024 consecutive elements of a tensor's [rows][inner] matrix,
//       a thread one float4 of every stream (lo, gap, alpha, m, v, nsplit slabs; alpha, m, v, wq back).  The four new soft weights stay
//       in registers and are split there: numel % 4 == 0 keeps them inside one 16-channel slice of the conv fragment order and inside
//       one 8-element record of the Linear fragment order, so each plane takes ONE 8-byte store per thread.  No LDS but block_sum's
//       4 floats.  A pinned element (gap == 0) never has its alpha, m or v stored: a thread with one falls back to per-element stores.
//   mx_dgrad_batch_kernel  One workgroup per 32 rows x 32 input channels of ONE tap.  Thread (r = tid / 8, q = tid % 8) loads the four
//       channels 4q .. 4q + 3 of row r (16 bytes where Cin % 4 == 0) into a 32 x 33-word LDS tile (row r at words 33 r ..: a column
//       read meets 32 banks), then owns the four rows 4q .. 4q + 3 of channel r: 16-byte stores along the rows into wd
//       [Cin][KH][KW][rows] where rows % 4 == 0, 8-byte stores into wd_planes and the transposed Linear planes.  Shapes that do not
//       allow it (rows % 4 != 0, Cin % 4 != 0) take element stores with the same index arithmetic.  Its first thread moves the
//       iteration counter when asked: this launch reads no counter.
#include "rdo_common.h"
#include "gather_body.h"
#include "../../include/rdo_ptq_mxroundbatch.h"
#include "ada_device.h"
#include "mx_grid_device.h"

namespace {

constexpr int kMaxBatch = 8;
static_assert(sizeof(rdo_mx_round_step_item) == 160, "hipops/_lib.py::MxRoundStepItem mirrors this layout");

struct MxItem {
    rdo_ada_desc d;
    const float* lo;
    const float* gap;
    const float* slabs;
    int nsplit;
    float* alpha;
    float* m;
    float* v;
    float* wq;
    float* wd;
    unsigned short* wq_planes;   // fragment order of the forward conv; wq_pscale == 0: bf16 three-way, > 0: fp16 two-way of wq * scale
    unsigned short* wd_planes;   // the same of wd, in the dgrad conv's fragment order
    unsigned short* lin_fwd;     // fp16 two-way planes of wq * lin_pscale in the split-fp16 Linear kernel's order; lin_bwd: of the transpose
    unsigned short* lin_bwd;
    float wq_pscale, wd_pscale, lin_pscale;
};

struct MxBatch {
    MxItem a[kMaxBatch];
    int blk_end[kMaxBatch];      // workgroups [blk_end[t - 1], blk_end[t]) belong to tensor t
    int n;
    float grad_scale, round_weight;
    const rdo_sched_row* sched;
    const int32_t* iter_ptr;
    float* round_loss_out;
    int32_t* iter_shadow;        // step launch: block 0 leaves *iter_ptr + 1 here
    int32_t* advance;            // dgrad launch: block 0 increments it
    int* ovf;                    // sticky fp16 overflow word of the conv planes
    int gather_beg;              // step launch: first gather workgroup (= the number of step workgroups)
    rdo::gq::Gather g;
};

// element (n, k) of W [rows][inner] in the fragment order of the split-fp16 Linear kernel (linear_h2.hip): half index inside a plane,
// nblk = rows / 16.  Eight consecutive k of a row are one 16-byte record.
__device__ __forceinline__ long lin_frag_index(int n, int k, int nblk) {
    return ((((long)(k >> 5) * nblk + (n >> 4)) * 64 + (n & 15) + 16 * ((k & 31) >> 3)) << 3) + (k & 7);
}

__device__ __forceinline__ int tensor_of(const MxBatch& b, int bid, int& beg) {
    int t = 0;
    while (t + 1 < b.n && bid >= b.blk_end[t]) ++t;
    beg = t ? b.blk_end[t - 1] : 0;
    return t;
}

// ---- the step of one tensor: workgroup `bid` of its `nblk` ---------------------------------------------------------------------------------
__device__ __forceinline__ void mx_step_body(const MxBatch& b, const MxItem& a, long bid, long nblk) {
    const rdo_ada_desc d = a.d;
    const int it = *b.iter_ptr;
    const rdo_sched_row sc = b.sched[it];
    const unsigned inner = (unsigned)(d.numel / d.rows);
    float rl_local = 0.f;
    int bad = 0;
    const long nq = d.numel / 4;
    for (long qi = bid * 256 + threadIdx.x; qi < nq; qi += nblk * 256) {
        // ---- load the streams
        const long e0 = qi * 4;
        const f32x4 lo4 = *reinterpret_cast<const f32x4*>(a.lo + e0);
        const f32x4 gp4 = *reinterpret_cast<const f32x4*>(a.gap + e0);
        f32x4 al4 = *reinterpret_cast<const f32x4*>(a.alpha + e0);
        const f32x4 g4 = slab_sum(lo4 * 0.f, a.slabs + e0, a.nsplit, d.numel);
        f32x4 m4 = *reinterpret_cast<const f32x4*>(a.m + e0);
        f32x4 v4 = *reinterpret_cast<const f32x4*>(a.v + e0);
        f32x4 o4 = lo4;
        bool any_pinned = false;
        // ---- the element step (mode 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const MxGrid grid{lo4[k], gp4[k]};
            if (!(grid.gap > 0.f)) {                                            // pinned (or a non-finite block): the weight stays lo
                any_pinned = true;
                o4[k] = lower_bound_fwd(d, grid.lo);
                continue;
            }
            ada_element(grid, d, 0, k, g4, al4, m4, v4, o4, b.grad_scale, b.round_weight, sc.b, sc.round_on, sc.step_size, sc.bc2_sqrt, rl_local);
        }
        // ---- store the state and the next soft weight
        if (!any_pinned) {
            *reinterpret_cast<f32x4*>(a.m + e0) = m4;
            *reinterpret_cast<f32x4*>(a.v + e0) = v4;
            *reinterpret_cast<f32x4*>(a.alpha + e0) = al4;
        } else {                                                                // a pinned element's alpha, m and v are never written
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (gp4[k] > 0.f) {
                    a.m[e0 + k] = m4[k];
                    a.v[e0 + k] = v4[k];
                    a.alpha[e0 + k] = al4[k];
                }
            }
        }
        *reinterpret_cast<f32x4*>(a.wq + e0) = o4;
        // ---- the planes of the new soft weight, from registers
        if (a.wq_planes) {
            // fragment order: four consecutive channels stay consecutive (Cin % 16 == 0 and e0 % 4 == 0); any other Cin: element order
            const long f0 = d.Cin > 0 ? rdo::frag_index(e0, d.rows, d.KH, d.KW, d.Cin) : e0;
            if (a.wq_pscale > 0.f) h2_store4(o4, a.wq_pscale, a.wq_planes, d.numel, f0, bad);
            else split3_store4(o4, a.wq_planes, d.numel, f0);
        }
        if (a.lin_fwd) {                                                        // (numel < 2^31 and inner % 32 == 0: the host checks)
            const unsigned row = (unsigned)e0 / inner;
            int none = 0;                                                       // the Linear split raises no overflow word
            h2_store4(o4, a.lin_pscale, a.lin_fwd, d.numel, lin_frag_index((int)row, (int)((unsigned)e0 - row * inner), d.rows >> 4), none);
        }
    }
    rdo::h2_report(bad, b.ovf);
    publish_round_loss(b.round_loss_out, sc.round_on, it, bid, rl_local);
}

__global__ __launch_bounds__(256) void mx_step_batch_kernel(MxBatch b) {
    // counter hand-over: this launch only reads *iter_ptr; the shadow word is another one (the host checks)
    if (b.iter_shadow && blockIdx.x == 0 && threadIdx.x == 0) *b.iter_shadow = *b.iter_ptr + 1;
    if ((int)blockIdx.x >= b.gather_beg) {                   // the next iteration's mini-batch (nothing behind the last iteration)
        const int it1 = *b.iter_ptr + 1;
        if (it1 < b.g.n_iters) {
            if (b.g.planes.p) rdo::gq::gather_h2_body(b.g, it1, (long)blockIdx.x - b.gather_beg, (long)gridDim.x - b.gather_beg);
            else rdo::gq::gather_fp32_body(b.g, it1, (long)blockIdx.x - b.gather_beg, (long)gridDim.x - b.gather_beg);
        }
        return;
    }
    int beg;
    const int t = tensor_of(b, (int)blockIdx.x, beg);
    mx_step_body(b, b.a[t], (long)blockIdx.x - beg, (long)b.blk_end[t] - beg);
}

// ---- the dgrad layouts of one tensor: tile `bid` ----------------------------------------------------------------------------------------
// four values of wd at o .. o + 3 (VEC: rows % 4 == 0, one store per buffer) or at o, o + 1, .. with `live` of them inside the tensor
template <bool VEC>
__device__ __forceinline__ void dgrad_store(const MxItem& a, const f32x4& t4, long o, int ci, int co, int tapf, int live, int& bad) {
    const rdo_ada_desc& d = a.d;
    const int taps = d.KH * d.KW;
    if constexpr (VEC) {
        if (a.wd) *reinterpret_cast<f32x4*>(a.wd + o) = t4;
        if (a.wd_planes) {
            // wd is the weight [Cin][KH][KW][rows] of the dgrad conv: its planes go in THAT conv's fragment order (slices of 16 rows)
            const long f0 = (d.rows & 15) ? o : (((((long)(co >> 4) * taps + tapf) * d.Cin + ci) << 4) + (co & 15));
            if (a.wd_pscale > 0.f) h2_store4(t4, a.wd_pscale, a.wd_planes, d.numel, f0, bad);
            else split3_store4(t4, a.wd_planes, d.numel, f0);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= live) break;
            if (a.wd) a.wd[o + k] = t4[k];
            if (a.wd_planes) {
                const long f = rdo::frag_index(o + k, d.Cin, d.KH, d.KW, d.rows);
                if (a.wd_pscale > 0.f) rdo::h2_split_store(t4[k], a.wd_pscale, a.wd_planes, d.numel, f, bad);
                else split3_store(t4[k], a.wd_planes, d.numel, f);
            }
        }
    }
}

__device__ __forceinline__ void mx_dgrad_body(const MxBatch& b, const MxItem& a, int bid) {
    const rdo_ada_desc d = a.d;
    const int Cin = d.Cin, taps = d.KH * d.KW, nrows = d.rows;
    const int ctiles = (Cin + 31) >> 5;
    const int ct = bid % ctiles; bid /= ctiles;
    const int tap = bid % taps;
    const int rt = bid / taps;
    const int q = threadIdx.x & 7, r = threadIdx.x >> 3;
    float(&tile)[32][33] = lds_tile32();
    // ---- wq [row][tap][ci] -> tile[row][ci]
    {
        const int row = rt * 32 + r, ci = ct * 32 + 4 * q;
        if (row < nrows && ci < Cin) {
            const float* src = a.wq + ((long)row * taps + tap) * Cin + ci;
            if ((Cin & 3) == 0) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
                for (int k = 0; k < 4; ++k) tile[r][4 * q + k] = w4[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ci + k < Cin) tile[r][4 * q + k] = src[k];
            }
        }
    }
    __syncthreads();
    // ---- tile[co][ci] -> wd [ci][KH-1-kh][KW-1-kw][co]: this thread owns four consecutive rows co of one input channel
    const int ci = ct * 32 + r, co = rt * 32 + 4 * q;
    if (ci >= Cin || co >= nrows) return;
    const int live = nrows - co < 4 ? nrows - co : 4;
    f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < live) t4[k] = tile[4 * q + k][r];
    const int kh = tap / d.KW, kw = tap - kh * d.KW;
    const int tapf = (d.KH - 1 - kh) * d.KW + (d.KW - 1 - kw);
    const long o = ((long)ci * taps + tapf) * nrows + co;
    int bad = 0;
    if ((nrows & 3) == 0) dgrad_store<true>(a, t4, o, ci, co, tapf, 4, bad);
    else dgrad_store<false>(a, t4, o, ci, co, tapf, live, bad);
    rdo::h2_report(bad, b.ovf);
    if (a.lin_bwd) {                                          // the transpose [Cin][rows] in the Linear kernel's order (rows % 32 == 0)
        int none = 0;
        h2_store4(t4, a.lin_pscale, a.lin_bwd, d.numel, lin_frag_index(ci, co, Cin >> 4), none);
    }
}

__global__ __launch_bounds__(256) void mx_dgrad_batch_kernel(MxBatch b) {
    // the counter moves here: no thread of this launch reads it, and every reader of the iteration ran before (stream order)
    if (b.advance && blockIdx.x == 0 && threadIdx.x == 0) *b.advance += 1;
    if (b.n == 0) return;
    int beg;
    const int t = tensor_of(b, (int)blockIdx.x, beg);
    mx_dgrad_body(b, b.a[t], (int)blockIdx.x - beg);
}

inline bool aligned(const void* p, uintptr_t by) { return reinterpret_cast<uintptr_t>(p) % by == 0; }

}  // namespace

extern "C" int rdo_mx_round_step_batch(const rdo_mx_round_step_item* items, int32_t n, float grad_scale, float round_weight,
                                       const rdo_sched_row* sched, const int32_t* iter_ptr, float* round_loss_out, int32_t* advance_iter,
                                       int32_t* iter_shadow, const rdo_gather_desc* next, void* stream) {
    const char* who = "rdo_mx_round_step_batch";
    RDO_REQUIRE(items && n >= 1 && n <= kMaxBatch, "%s: bad argument (items, 1 <= n <= %d)", who, kMaxBatch);
    RDO_REQUIRE(sched && iter_ptr, "%s: schedule / iteration counter missing", who);
    RDO_REQUIRE(!(advance_iter && iter_shadow), "%s: advance_iter and iter_shadow are alternatives", who);
    RDO_REQUIRE(iter_shadow != iter_ptr, "%s: iter_shadow must not be the word iter_ptr reads", who);
    RDO_REQUIRE(aligned(sched, 4) && aligned(iter_ptr, 4) && aligned(round_loss_out, 4) && aligned(advance_iter, 4) && aligned(iter_shadow, 4),
                "%s: sched, iter_ptr, round_loss_out, advance_iter and iter_shadow must be 4-byte aligned", who);
    MxBatch b{}, bw{};
    int blocks = 0, wblocks = 0;
    double bytes = 0.0;
    for (int i = 0; i < n; ++i) {
        const rdo_mx_round_step_item& it = items[i];
        if (int rc = check_desc(&it.d, who, false)) return rc;
        RDO_REQUIRE(it.d.numel % 4 == 0 && it.d.numel < (1L << 31), "%s: numel %ld of item %d is not a multiple of 4 below 2^31", who,
                    (long)it.d.numel, i);
        RDO_REQUIRE(it.lo && it.gap && it.slabs && it.alpha && it.adam_m && it.adam_v && it.wq, "%s: null pointer in item %d", who, i);
        RDO_REQUIRE(it.nsplit >= 1, "%s: item %d: nsplit %d (at least one gradient slab)", who, i, it.nsplit);
        RDO_REQUIRE(aligned(it.lo, 16) && aligned(it.gap, 16) && aligned(it.slabs, 16) && aligned(it.alpha, 16) && aligned(it.adam_m, 16) &&
                    aligned(it.adam_v, 16) && aligned(it.wq, 16), "%s: item %d: lo, gap, slabs, alpha, adam_m, adam_v and wq must be 16-byte aligned",
                    who, i);
        RDO_REQUIRE(aligned(it.wd, it.d.rows % 4 == 0 ? 16 : 4), "%s: item %d: wd must be %d-byte aligned", who, i, it.d.rows % 4 == 0 ? 16 : 4);
        RDO_REQUIRE(aligned(it.wq_planes, 8) && aligned(it.wd_planes, 8) && aligned(it.lin_fwd_planes, 8) && aligned(it.lin_bwd_planes, 8),
                    "%s: item %d: planes must be 8-byte aligned", who, i);
        RDO_REQUIRE(it.wq_plane_scale >= 0.f && it.wd_plane_scale >= 0.f && std::isfinite(it.wq_plane_scale) && std::isfinite(it.wd_plane_scale),
                    "%s: item %d: plane scales must be 0 (bf16 planes) or positive (fp16 planes)", who, i);
        RDO_REQUIRE(!it.wd_planes || it.wd, "%s: item %d: wd_planes without wd", who, i);
        RDO_REQUIRE(!(it.wd || it.lin_fwd_planes || it.lin_bwd_planes) || it.d.Cin > 0, "%s: item %d: wd and Linear planes need a conv layout", who, i);
        if (it.lin_fwd_planes || it.lin_bwd_planes)
            RDO_REQUIRE(it.d.rows % 32 == 0 && it.d.Cin % 32 == 0 && it.d.KH * it.d.KW == 1 && it.lin_plane_scale > 0.f && std::isfinite(it.lin_plane_scale),
                        "%s: item %d: Linear planes need a 1 x 1 layout with rows and inner in blocks of 32 and a positive scale", who, i);
        MxItem& a = b.a[i];
        a.d = it.d; a.lo = it.lo; a.gap = it.gap; a.slabs = it.slabs; a.nsplit = it.nsplit;
        a.alpha = it.alpha; a.m = it.adam_m; a.v = it.adam_v; a.wq = it.wq; a.wd = it.wd;
        a.wq_planes = static_cast<unsigned short*>(it.wq_planes); a.wd_planes = static_cast<unsigned short*>(it.wd_planes);
        a.lin_fwd = static_cast<unsigned short*>(it.lin_fwd_planes); a.lin_bwd = static_cast<unsigned short*>(it.lin_bwd_planes);
        a.wq_pscale = it.wq_plane_scale; a.wd_pscale = it.wd_plane_scale; a.lin_pscale = it.lin_plane_scale;
        blocks += (int)rdo::grid_for(it.d.numel / 4);
        b.blk_end[i] = blocks;
        bytes += 4.0 * it.d.numel * (it.nsplit + 9.0);
        if (it.wd || it.lin_bwd_planes) {
            bw.a[bw.n] = a;
            wblocks += (int)tile_blocks(it.d);
            bw.blk_end[bw.n++] = wblocks;
            bytes += 8.0 * it.d.numel;
        }
    }
    b.n = n;
    b.grad_scale = grad_scale; b.round_weight = round_weight; b.sched = sched; b.iter_ptr = iter_ptr; b.round_loss_out = round_loss_out;
    b.iter_shadow = iter_shadow;
    b.gather_beg = blocks;
    if (next) {
        const char* gw = "rdo_mx_round_step_batch (gather)";
        RDO_REQUIRE(next->cache_q && next->cache_fp && next->idx_table && (next->out || next->out_planes) && next->n_iters > 0,
                    "%s: null pointer in the gather descriptor", gw);
        RDO_REQUIRE(next->B > 0 && next->batch_offset >= 0 && next->per_image > 0 && next->per_image % 4 == 0 &&
                    (long)(next->batch_offset + next->B) * next->per_image < (1L << 32), "%s: bad gather shape", gw);
        RDO_REQUIRE(!next->out_planes || (next->C > 0 && next->C % 16 == 0 && next->per_image % next->C == 0 && next->out_scale > 0.f),
                    "%s: the plane form needs C %% 16 == 0 and a positive power-of-two scale", gw);
        RDO_REQUIRE(next->prob >= 0.f && next->prob <= 1.f, "%s: prob out of [0,1]", gw);
        RDO_REQUIRE(aligned(next->cache_q, 16) && aligned(next->cache_fp, 16) && aligned(next->out, 16) && aligned(next->out_planes, 16) &&
                    aligned(next->idx_table, 4) && aligned(next->overflow_flag, 4), "%s: misaligned pointer in the gather descriptor", gw);
    }
    // behind the last argument check: the look-up may allocate the word
    b.ovf = rdo::h2_overflow_flag();
    if (next) {
        const double t = floor((double)next->prob * 4294967296.0);
        const unsigned long long thr = (unsigned long long)(t > 4294967296.0 ? 4294967296.0 : t);
        b.g = rdo::gq::Gather{next->cache_q, next->cache_fp, next->idx_table, next->n_iters, next->B, next->batch_offset, (long)next->per_image,
                              next->C, thr, next->seed, next->out,
                              rdo::gq::H2Out{static_cast<unsigned short*>(next->out_planes), next->out_scale,
                                             next->overflow_flag ? reinterpret_cast<int*>(next->overflow_flag) : b.ovf}};
        const long gb = rdo::gq::gather_blocks(b.g);
        const long cap = b.g.planes.p ? 8192 : 2048;            // the grids of the stand-alone gather kernels
        blocks += (int)(gb > cap ? cap : gb);
        bytes += (8.0 + (next->out ? 4.0 : 0.0) + (next->out_planes ? 4.0 : 0.0)) * next->B * (double)next->per_image;
    }
    bw.ovf = b.ovf;
    bw.advance = advance_iter;
    const bool second = bw.n > 0 || advance_iter;
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(mx_step_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, b);
            if (second) hipLaunchKernelGGL(mx_dgrad_batch_kernel, dim3((unsigned)(wblocks > 0 ? wblocks : 1)), dim3(256), 0, s, bw);
            return rdo::check_launch("mx_round_step_batch");
        },
        stream, next ? "mx_round_step_gather" : "mx_round_step_batch", 0.0, bytes);
}
