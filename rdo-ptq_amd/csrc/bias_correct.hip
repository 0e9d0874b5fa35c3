// Empirical bias correction after calibration (include/rdo_ptq_bias.h): the tap sums of a layer's input and the bias shift they give.
// Built with -ffp-contract=off (the order and the rounding of every addition is the one written here).
//
// rdo_tap_sums.  A conv / transposed-conv / Linear layer fuses its activation into the kernel epilogue, so the pre-activation output,
// whose mean a bias correction needs, never exists in memory.  Its sum over all output pixels is n b[o] + W[o] . S with
// S[kh][kw][c] = the sum of the INPUT over the pixels tap (kh, kw) reads: one read of the input, exact for padding, stride and borders.
// The taps a pixel belongs to depend on its row alone (a mask over kh) and on its column alone (a mask over kw), and few distinct masks
// exist per axis (borders, and one per residue of the stride): a "class" is one distinct non-empty mask.  The host describes every axis
// as segments (start, step, count) of indices of one class; a workgroup takes a share of the pixels of ONE row segment and walks it
// once per column class with ONE running sum per lane (never k * k of them), leaving a partial row [column class][C].  tap_fold_kernel
// adds, per tap, the partial rows of the row segments and column classes that hold it: two launches.  Nothing is atomic: the order of
// the fp32 additions is a function of the geometry alone -- a lane's pixels in ascending order, closed into a second sum every
// kTapChain pixels, lane 0 adding the pixel lanes 1 .. PL - 1 onto its own, the fold as described at tap_fold_kernel.  A value
// only ever meets values of its own channel.
//
// rdo_bias_shift.  shift[o] = (W_ref[o] . S_ref - W_q[o] . S_q) / n in float64: each product is of the size of the layer's mean output
// and the two nearly cancel, so fp32 would leave nothing of the difference.
#include <algorithm>
#include <utility>

#include "rdo_common.h"
#include "../../include/rdo_ptq_bias.h"

namespace {

constexpr int kTapChain = 1024;      // pixels a lane adds before its running sum is closed into the second-level sum
constexpr int kTapBlocks = 512;      // workgroups of the partial pass: two per CU of an MI355X
constexpr int kTapMaxSegs = 48;      // segments per axis the kernel arguments hold
constexpr int kTapFlight = 4;        // loads a lane keeps in flight
inline int tap_max_cls(int k) { return 4 * k + 4; }   // >= the distinct non-empty masks of an axis (conv: < 3 k; transposed: intervals, k (k + 1) / 2)

struct TapSeg { int start, step, count, cls; };
struct TapPlan {
    int nrs, ncs, NR, NC, nblk;
    TapSeg rs[kTapMaxSegs];          // row segments: low border, interior, high border
    TapSeg cs[kTapMaxSegs];          // column segments, sorted by class (stable)
    int blk0[kTapMaxSegs + 1];       // first workgroup of a row segment
    unsigned char rmask[32], cmask[32];   // taps of a class
};

// tap mask of index `h` of an axis of `H` inputs and `Ho` outputs
inline unsigned tap_mask(int h, int k, int stride, int pad, int Ho, bool transposed) {
    unsigned m = 0;
    for (int kh = 0; kh < k; ++kh) {
        bool in;
        if (transposed) {
            const long t = (long)h * stride - pad + kh;
            in = t >= 0 && t < Ho;
        } else {
            const long u = (long)h + pad - kh;
            in = u >= 0 && u % stride == 0 && u / stride < Ho;
        }
        if (in) m |= 1u << kh;
    }
    return m;
}

// one axis -> segments (start, step, count) of indices of one class, classes numbered by first appearance; O(k) work whatever the size of
// the axis (a Linear layer's tokens are one axis of millions).  false: more classes or segments than the kernel arguments hold.
// Only the first and the last few indices can lose a tap to an end of the axis: conv, u = h + pad - kh >= 0 holds from h = k - 1 on and
// u / stride < Ho up to h = H - k (Ho stride > H + 2 pad - k); transposed, with b = ceil(pad / stride), 0 <= h stride - pad + kh < Ho holds
// for every kh on b <= h < H - b.  Those indices are segments of their own; between them a conv's mask depends on (h + pad) mod stride
// alone (one segment of step `stride` per residue that holds a tap), a transposed conv's is full.
bool tap_axis(int H, int k, int stride, int pad, int Ho, bool transposed, int max_cls, TapSeg* segs, int* nsegs, unsigned char* masks, int* ncls) {
    int cls_of[128];                 // mask -> class, or -1
    for (int i = 0; i < 128; ++i) cls_of[i] = -1;
    *nsegs = *ncls = 0;
    auto add = [&](long start, long step, long count) -> bool {
        const unsigned m = tap_mask((int)start, k, stride, pad, Ho, transposed);
        if (!m || count <= 0) return true;          // no output reads these indices
        if (cls_of[m] < 0) {
            if (*ncls == max_cls) return false;
            masks[*ncls] = (unsigned char)m;
            cls_of[m] = (*ncls)++;
        }
        if (*nsegs == kTapMaxSegs) return false;
        segs[(*nsegs)++] = TapSeg{(int)start, (int)step, (int)count, cls_of[m]};
        return true;
    };
    const long edge = transposed ? ((long)pad + stride - 1) / stride : k - 1;
    const long L = std::min<long>(H, edge), R = std::max<long>(L, transposed ? H - edge : (long)H - k + 1);
    if (L + (H - R) > kTapMaxSegs) return false;
    for (long h = 0; h < L; ++h)
        if (!add(h, 1, 1)) return false;
    if (transposed) {
        if (!add(L, 1, R - L)) return false;
    } else if (R > L) {
        if (stride <= k) {
            for (long h0 = L; h0 < R && h0 < L + stride; ++h0)
                if (!add(h0, stride, (R - 1 - h0) / stride + 1)) return false;
        } else {                                    // at most k residues hold a tap: h + pad = kh (mod stride)
            for (int kh = 0; kh < k; ++kh) {
                const long h0 = L + (((kh - pad - L) % stride) + stride) % stride;
                if (h0 < R && !add(h0, stride, (R - 1 - h0) / stride + 1)) return false;
            }
        }
    }
    for (long h = R; h < H; ++h)
        if (!add(h, 1, 1)) return false;
    return true;
}

// thread = (pixel lane, group of V channels): qpb groups side by side, PL pixel lanes of them in a workgroup of 256
struct TapGeom { int QN, qpb, PL; };
__host__ __device__ inline TapGeom tap_geom(int C, int V) {
    const int QN = C / V, qpb = QN < 256 ? QN : 256;
    return TapGeom{QN, qpb, 256 / qpb};
}

// the whole plan of a call (V = channels per load).  false: more classes or segments than the kernel arguments hold.  nblk == 0: no tap
// reads any pixel.
bool tap_plan(int N, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo, bool transposed, int V, TapPlan* out) {
    TapPlan& pl = *out;
    const int mc = tap_max_cls(k);
    if (!tap_axis(H, k, stride, pad, Ho, transposed, mc, pl.rs, &pl.nrs, pl.rmask, &pl.NR) ||
        !tap_axis(W, k, stride, pad, Wo, transposed, mc, pl.cs, &pl.ncs, pl.cmask, &pl.NC))
        return false;
    pl.nblk = 0;
    if (pl.nrs == 0 || pl.ncs == 0) return true;
    // column segments by class (stable): a workgroup completes one class before the next
    for (int a = 1; a < pl.ncs; ++a)
        for (int b = a; b > 0 && pl.cs[b - 1].cls > pl.cs[b].cls; --b) std::swap(pl.cs[b - 1], pl.cs[b]);
    const int PL = tap_geom(C, V).PL;
    // workgroups per row segment: in proportion to its pixels, at least one, each with >= 16 pixels per lane where there are as many
    int64_t cols = 0;
    for (int j = 0; j < pl.ncs; ++j) cols += pl.cs[j].count;
    int64_t total = 0;
    for (int s = 0; s < pl.nrs; ++s) total += (int64_t)N * pl.rs[s].count * cols;
    const int64_t want = std::min<int64_t>(kTapBlocks, std::max<int64_t>(1, rdo::ceil_div(total, (int64_t)PL * 16)));
    pl.blk0[0] = 0;
    for (int s = 0; s < pl.nrs; ++s) {
        const int64_t pix = (int64_t)N * pl.rs[s].count * cols;
        const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(pix * want / total, rdo::ceil_div(pix, (int64_t)PL * 16)));
        pl.blk0[s + 1] = pl.blk0[s] + (int)nb;
    }
    pl.nblk = pl.blk0[pl.nrs];                            // <= kTapBlocks + kTapMaxSegs: what the workspace holds
    return true;
}

// The pixels of one (row segment, column segment) pair that one pixel lane of one workgroup adds, in order: the workgroup `ci` of the `nb`
// of the row segment takes the share [e0, e1) of the nrows * cs.count pixels (row-major: row t = member t % count of image t / count),
// its lane `lane` of `PL` the pixels e0 + lane, e0 + lane + PL, ..  Host and device walk with this one struct.
struct TapWalk {
    long e, e1, n;                   // pixel index in the pair, end of the share, image
    unsigned i, m, ccount, rcount, PL;   // member of the column segment, of the row segment
    int rstart, rstep, cstart, cstep;
    __host__ __device__ TapWalk(const TapSeg& rs, const TapSeg& cs, long nrows, int ci, int nb, int lane, int PL_)
        : ccount((unsigned)cs.count), rcount((unsigned)rs.count), PL((unsigned)PL_), rstart(rs.start), rstep(rs.step), cstart(cs.start),
          cstep(cs.step) {
        const long items = nrows * cs.count;
        e = items * ci / nb + lane;
        e1 = items * (ci + 1) / nb;
        const long row = e / cs.count;
        i = (unsigned)(e - row * cs.count);
        n = row / rs.count;
        m = (unsigned)(row - n * rs.count);
    }
    // pixel index in [0, N H W) of the current position (valid while e < e1)
    __host__ __device__ long pixel(int H, int W) const { return (n * H + (rstart + (long)m * rstep)) * W + (cstart + (long)i * cstep); }
    __host__ __device__ void next() {
        e += PL;
        i += PL;
        if (i >= ccount) {
            const unsigned d = i / ccount;
            i -= d * ccount;
            m += d;
            if (m >= rcount) {
                const unsigned d2 = m / rcount;
                m -= d2 * rcount;
                n += d2;
            }
        }
    }
};

// ---- partial pass: part[workgroup][column class][C]
template <int V>
__global__ __launch_bounds__(256) void tap_partial_kernel(const float* __restrict__ x, int N, int H, int W, int C, TapPlan pl, float* part) {
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const TapGeom g = tap_geom(C, V);
    const int lane = threadIdx.x / g.qpb, ql = threadIdx.x - lane * g.qpb;
    __shared__ float sm[V * 256];                         // [channel of the group][thread]
    int si = 0;
    while (si + 1 < pl.nrs && (int)blockIdx.x >= pl.blk0[si + 1]) ++si;
    const TapSeg rs = pl.rs[si];
    const int nb = pl.blk0[si + 1] - pl.blk0[si], ci = blockIdx.x - pl.blk0[si];
    const long nrows = (long)N * rs.count;                // rows of this segment over all images: row t = image t / count, member t % count
    float* dst = part + (long)blockIdx.x * pl.NC * C;
    for (int qb = 0; qb < g.QN; qb += g.qpb) {
        const int q = qb + ql;
        const bool live = lane < g.PL && q < g.QN;
        vec_t acc, tot;
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = tot[e] = 0.f;
        int run = 0;
        for (int j = 0; j < pl.ncs; ++j) {
            const TapSeg cs = pl.cs[j];
            if (live) {
                TapWalk wk(rs, cs, nrows, ci, nb, lane, g.PL);
                while (wk.e < wk.e1) {
                    long off[kTapFlight];
                    bool ok[kTapFlight];
#pragma unroll
                    for (int u = 0; u < kTapFlight; ++u) {
                        ok[u] = wk.e < wk.e1;
                        off[u] = wk.pixel(H, W) * C + (long)q * V;
                        wk.next();
                    }
                    vec_t v[kTapFlight];
#pragma unroll
                    for (int u = 0; u < kTapFlight; ++u)
                        if (ok[u]) v[u] = *reinterpret_cast<const vec_t*>(x + off[u]);
#pragma unroll
                    for (int u = 0; u < kTapFlight; ++u)
                        if (ok[u]) {
                            acc += v[u];
                            if (++run == kTapChain) {
                                run = 0;
                                tot += acc;
#pragma unroll
                                for (int e2 = 0; e2 < V; ++e2) acc[e2] = 0.f;
                            }
                        }
                }
            }
            if (j + 1 == pl.ncs || pl.cs[j + 1].cls != cs.cls) {          // the class is complete: fold the pixel lanes, leave its row
                if (live) {
#pragma unroll
                    for (int e = 0; e < V; ++e) sm[e * 256 + threadIdx.x] = tot[e] + acc[e];
                }
                __syncthreads();
                if (live && lane == 0) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        float r = sm[e * 256 + ql];
                        for (int t = 1; t < g.PL; ++t) r += sm[e * 256 + t * g.qpb + ql];
                        dst[(long)cs.cls * C + q * V + e] = r;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] = tot[e] = 0.f;
                run = 0;
            }
        }
    }
}

// ---- fold of the partial rows into the taps: out[kh][kw][c] += the sum over the pairs (row segment whose class holds kh, column class
// that holds kw), in segment order then class order, of the segment's workgroups.  A workgroup folds sixteen consecutive entries (kh, kw,
// c): thread = (entry cl, lane j of sixteen), so the sixteen threads that share j read sixteen consecutive floats of one partial row (one
// 64-byte run: with the lanes of an entry side by side instead, every lane of a wave asks for a line of its own, and the fold cost as
// much as the pass over x).  Lane j adds the workgroups j, j + 16, .. of every pair in order, eight loads in flight; thread (cl, 0) then
// adds the lanes 1 .. 15 onto its own through LDS.  The fold is latency, not traffic.
__global__ __launch_bounds__(256) void tap_fold_kernel(const float* part, TapPlan pl, int C, int k, float* out) {
    const int cl = threadIdx.x & 15, j = threadIdx.x >> 4;
    const long i = (long)blockIdx.x * 16 + cl;
    const bool live = i < (long)k * k * C;
    const int c = live ? (int)(i % C) : 0, tap = live ? (int)(i / C) : 0, kw = tap % k, kh = tap / k;
    const long n = (long)pl.NC * C;                       // entries of a partial row
    __shared__ float sm[16][17];
    float r = 0.f;
    if (live) {
        for (int s = 0; s < pl.nrs; ++s) {
            if (!((pl.rmask[pl.rs[s].cls] >> kh) & 1)) continue;
            const int end = pl.blk0[s + 1];
            for (int cc = 0; cc < pl.NC; ++cc) {
                if (!((pl.cmask[cc] >> kw) & 1)) continue;
                const float* src = part + (long)cc * C + c;
                int b = pl.blk0[s] + j;
                for (; b + 112 < end; b += 128) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = src[(long)(b + 16 * u) * n];
#pragma unroll
                    for (int u = 0; u < 8; ++u) r = r + v[u];
                }
                for (; b < end; b += 16) r = r + src[(long)b * n];
            }
        }
    }
    sm[j][cl] = r;
    __syncthreads();
    if (live && j == 0) {
        for (int t = 1; t < 16; ++t) r = r + sm[t][cl];
        out[i] = out[i] + r;
    }
}

// ---- bias shift: one workgroup per output row; thread t adds the products t, t + 256, .. in float64, then a fixed tree
__global__ __launch_bounds__(256) void bias_shift_kernel(const float* w_ref, const float* w_q, const double* s_ref, const double* s_q,
                                                         double inv_n, const float* org_bias, int K, double* shift, float* bias_out) {
    const int o = blockIdx.x;
    const float* a = w_ref + (long)o * K;
    const float* b = w_q + (long)o * K;
    double da = 0.0, db = 0.0;
    for (int j = threadIdx.x; j < K; j += 256) {
        da = da + (double)a[j] * s_ref[j];
        db = db + (double)b[j] * s_q[j];
    }
    __shared__ double sa[256], sb[256];
    sa[threadIdx.x] = da;
    sb[threadIdx.x] = db;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            sa[threadIdx.x] = sa[threadIdx.x] + sa[threadIdx.x + h];
            sb[threadIdx.x] = sb[threadIdx.x] + sb[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double s = (sa[0] - sb[0]) * inv_n;
        shift[o] = s;
        bias_out[o] = (float)((double)org_bias[o] + s);
    }
}

}  // namespace

// every geometry check of rdo_tap_sums (and of rdo_tap_sums_lane_pixels): RDO_OK or RDO_EINVAL with the message set
static int tap_validate(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                        int32_t transposed) {
    RDO_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "rdo_tap_sums: non-positive size N %d H %d W %d C %d", N, H, W, C);
    RDO_REQUIRE(k >= 1 && k <= RDO_TAP_MAX_K, "rdo_tap_sums: k %d outside [1, %d]", k, RDO_TAP_MAX_K);
    RDO_REQUIRE(stride >= 1, "rdo_tap_sums: stride %d < 1", stride);
    RDO_REQUIRE(pad >= 0, "rdo_tap_sums: pad %d < 0", pad);
    RDO_REQUIRE(transposed == 0 || transposed == 1, "rdo_tap_sums: transposed must be 0 or 1, got %d", transposed);
    RDO_REQUIRE(Ho > 0 && Wo > 0, "rdo_tap_sums: non-positive output size Ho %d Wo %d", Ho, Wo);
    for (int ax = 0; ax < 2; ++ax) {
        const int64_t in = ax ? W : H, o = ax ? Wo : Ho;
        if (transposed) {
            const int64_t lo = (in - 1) * stride - 2 * (int64_t)pad + k;
            RDO_REQUIRE(o >= lo && o < lo + stride, "rdo_tap_sums: a transposed conv of %lld inputs (k %d stride %d pad %d) gives %lld .. %lld "
                        "outputs, not %lld", (long long)in, k, stride, pad, (long long)lo, (long long)(lo + stride - 1), (long long)o);
        } else {
            const int64_t span = in + 2 * (int64_t)pad - k;
            RDO_REQUIRE(span >= 0 && o == span / stride + 1, "rdo_tap_sums: a conv of %lld inputs (k %d stride %d pad %d) does not give %lld outputs",
                        (long long)in, k, stride, pad, (long long)o);
        }
    }
    const int64_t npix = (int64_t)N * H * W;
    RDO_REQUIRE(npix <= 0x7fffffffLL, "rdo_tap_sums: %lld pixels are beyond 32-bit pixel indices", (long long)npix);
    RDO_REQUIRE((int64_t)k * k * C <= 0x7fffffffLL && (int64_t)tap_max_cls(k) * C <= 0x7fffffffLL,
                "rdo_tap_sums: %d channels are too many for 32-bit entry indices", C);
    return RDO_OK;
}

extern "C" {

int64_t rdo_tap_sums_workspace(int32_t C, int32_t k) {
    if (C <= 0 || k < 1 || k > RDO_TAP_MAX_K) return 0;
    const int64_t mc = tap_max_cls(k);
    return (int64_t)(kTapBlocks + kTapMaxSegs) * mc * C;
}

int rdo_tap_sums(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, int32_t Ho,
                 int32_t Wo, int32_t transposed, float* out, float* ws, void* stream) {
    RDO_REQUIRE(x && out && ws, "rdo_tap_sums: null pointer");
    if (const int e = tap_validate(N, H, W, C, k, stride, pad, Ho, Wo, transposed)) return e;
    const int64_t npix = (int64_t)N * H * W;
    TapPlan pl{};
    const bool vec = C % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    RDO_REQUIRE(tap_plan(N, H, W, C, k, stride, pad, Ho, Wo, transposed != 0, vec ? 4 : 1, &pl),
                "rdo_tap_sums: the geometry has more than %d tap classes or %d index runs per axis", tap_max_cls(k), kTapMaxSegs);
    if (pl.nblk == 0) return RDO_OK;                      // no tap reads any pixel (a stride beyond the kernel on a tiny map): nothing to add
    float* part = ws;
    return rdo::dispatch(
        [=](hipStream_t s) {
            if (vec) hipLaunchKernelGGL(tap_partial_kernel<4>, dim3(pl.nblk), dim3(256), 0, s, x, N, H, W, C, pl, part);
            else hipLaunchKernelGGL(tap_partial_kernel<1>, dim3(pl.nblk), dim3(256), 0, s, x, N, H, W, C, pl, part);
            hipLaunchKernelGGL(tap_fold_kernel, dim3((unsigned)rdo::ceil_div((int64_t)k * k * C, 16)), dim3(256), 0, s, part, pl, C, k, out);
            return rdo::check_launch("tap_sums");
        },
        stream, "tap_sums", 0.0, 4.0 * (double)npix * C);
}

int64_t rdo_tap_sums_lane_pixels(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad, int32_t Ho, int32_t Wo,
                                 int32_t transposed, int32_t vec) {
    if (tap_validate(N, H, W, C, k, stride, pad, Ho, Wo, transposed)) return -1;
    TapPlan pl{};
    const int V = vec && C % 4 == 0 ? 4 : 1;
    if (!tap_plan(N, H, W, C, k, stride, pad, Ho, Wo, transposed != 0, V, &pl)) {
        rdo::set_error(RDO_EINVAL, "rdo_tap_sums_lane_pixels: the geometry has more than %d tap classes or %d index runs per axis",
                       tap_max_cls(k), kTapMaxSegs);
        return -1;
    }
    const int64_t PL = tap_geom(C, V).PL;
    int64_t worst = 0;
    for (int s = 0; s < pl.nrs; ++s) {
        const int64_t nb = pl.blk0[s + 1] - pl.blk0[s], nrows = (int64_t)N * pl.rs[s].count;
        int64_t run = 0;
        for (int j = 0; j < pl.ncs; ++j) {
            run += rdo::ceil_div(rdo::ceil_div(nrows * pl.cs[j].count, nb), PL);
            if (j + 1 == pl.ncs || pl.cs[j + 1].cls != pl.cs[j].cls) {
                worst = std::max(worst, run);
                run = 0;
            }
        }
    }
    return worst;
}

int rdo_bias_shift(const float* w_ref, const float* w_q, const double* s_ref, const double* s_q, double inv_n, const float* org_bias,
                   int32_t O, int32_t K, double* shift, float* bias_out, void* stream) {
    RDO_REQUIRE(w_ref && w_q && s_ref && s_q && org_bias && shift && bias_out, "rdo_bias_shift: null pointer");
    RDO_REQUIRE(O > 0 && K > 0, "rdo_bias_shift: non-positive size O %d K %d", O, K);
    RDO_REQUIRE(inv_n == inv_n && inv_n > 0.0 && inv_n <= 1.0, "rdo_bias_shift: inv_n %g is not 1 / (a pixel count)", inv_n);
    return rdo::dispatch(
        [=](hipStream_t s) {
            hipLaunchKernelGGL(bias_shift_kernel, dim3(O), dim3(256), 0, s, w_ref, w_q, s_ref, s_q, inv_n, org_bias, K, shift, bias_out);
            return rdo::check_launch("bias_shift");
        },
        stream, "bias_shift", 4.0 * O * K, 8.0 * O * K);
}

}  // extern "C"
