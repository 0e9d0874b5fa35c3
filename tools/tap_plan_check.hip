// Host-only check of the plan and the pixel walk of csrc/bias_correct.hip (tap_plan, TapWalk: the code the kernel runs, compiled for the
// host): over some 39 000 geometries (k 1-7, stride 1-9, pad 0 .. k + 1, maps of 1-65, conv and transposed, the shapes of the tests and the
// benchmark) every pixel a lane visits is in bounds, visited once, of the class its masks say, and the taps folded from the classes equal
// the definition over the outputs.  No HIP call is made and no GPU is needed; meant to run under the host sanitizers:
//   hipcc -O1 -g -std=c++20 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/tap_plan_check.hip -o /tmp/tap_plan_check && /tmp/tap_plan_check
#include "../rdo-ptq_amd/csrc/bias_correct.hip"

#include <cstdlib>
#include <vector>
// stubs for the symbols of runtime.hip
namespace rdo {
Recorder& recorder() { static Recorder r; return r; }
int set_error(int code, const char*, ...) { return code; }
}

static int check(int N, int H, int W, int C, int V, int k, int s, int p, int Ho, int Wo, bool tr) {
    TapPlan pl{};
    if (!tap_plan(N, H, W, C, k, s, p, Ho, Wo, tr, V, &pl)) { printf("plan refused N%d H%d W%d k%d s%d p%d tr%d\n", N, H, W, k, s, p, tr); return 1; }
    const long npix = (long)N * H * W;
    std::vector<int> x(npix);
    for (auto& v : x) v = rand() % 9 - 4;
    // definition over the outputs
    std::vector<long> ref(k * k, 0);
    auto reads = [&](int in, int o, int kk, int n_in) -> bool {   // does output o read input `in` through tap kk?
        return tr ? (in * s - p + kk == o) : (o * s - p + kk == in);
    };
    std::vector<std::vector<char>> rt(k, std::vector<char>(H, 0)), ct(k, std::vector<char>(W, 0));
    for (int kk = 0; kk < k; ++kk) {
        for (int h = 0; h < H; ++h) for (int o = 0; o < Ho; ++o) if (reads(h, o, kk, H)) rt[kk][h] = 1;
        for (int w = 0; w < W; ++w) for (int o = 0; o < Wo; ++o) if (reads(w, o, kk, W)) ct[kk][w] = 1;
    }
    for (int n = 0; n < N; ++n) for (int h = 0; h < H; ++h) for (int w = 0; w < W; ++w)
        for (int kh = 0; kh < k; ++kh) for (int kw = 0; kw < k; ++kw)
            if (rt[kh][h] && ct[kw][w]) ref[kh * k + kw] += x[((long)n * H + h) * W + w];
    if (pl.nblk == 0) {
        for (long v : ref) if (v) { printf("empty plan but taps\n"); return 1; }
        return 0;
    }
    if (pl.nblk > kTapBlocks + kTapMaxSegs) { printf("too many blocks %d\n", pl.nblk); return 1; }
    std::vector<char> seen(npix, 0);
    std::vector<long> T((long)pl.NR * pl.NC, 0);
    const TapGeom g = tap_geom(C, V);
    for (int b = 0; b < pl.nblk; ++b) {
        int si = 0;
        while (si + 1 < pl.nrs && b >= pl.blk0[si + 1]) ++si;
        const TapSeg rs = pl.rs[si];
        const int nb = pl.blk0[si + 1] - pl.blk0[si], ci = b - pl.blk0[si];
        const long nrows = (long)N * rs.count;
        for (int j = 0; j < pl.ncs; ++j) {
            const TapSeg cs = pl.cs[j];
            if (j && pl.cs[j - 1].cls > cs.cls) { printf("unsorted\n"); return 1; }
            for (int lane = 0; lane < g.PL; ++lane) {
                TapWalk wk(rs, cs, nrows, ci, nb, lane, g.PL);
                while (wk.e < wk.e1) {
                    const long px = wk.pixel(H, W);
                    if (px < 0 || px >= npix) { printf("OOB pixel %ld of %ld\n", px, npix); return 1; }
                    if (seen[px]++) { printf("pixel twice\n"); return 1; }
                    const int h = (int)(px / W % H), w = (int)(px % W);
                    if (tap_mask(h, k, s, p, Ho, tr) != pl.rmask[rs.cls] || tap_mask(w, k, s, p, Wo, tr) != pl.cmask[cs.cls]) { printf("class\n"); return 1; }
                    T[(long)rs.cls * pl.NC + cs.cls] += x[px];
                    wk.next();
                }
            }
        }
    }
    for (int kh = 0; kh < k; ++kh) for (int kw = 0; kw < k; ++kw) {
        long r = 0;
        for (int rc = 0; rc < pl.NR; ++rc) for (int cc = 0; cc < pl.NC; ++cc)
            if (((pl.rmask[rc] >> kh) & 1) && ((pl.cmask[cc] >> kw) & 1)) r += T[(long)rc * pl.NC + cc];
        if (r != ref[kh * k + kw]) { printf("tap (%d,%d): %ld != %ld  N%d H%d W%d k%d s%d p%d tr%d\n", kh, kw, r, ref[kh * k + kw], N, H, W, k, s, p, tr); return 1; }
    }
    return 0;
}

int main() {
    int bad = 0, n = 0;
    const int Cs[][2] = {{4, 4}, {3, 1}, {192, 4}, {2, 1}, {320, 4}, {1028, 4}, {1, 1}};
    for (int k = 1; k <= 7; ++k)
        for (int s = 1; s <= 9; ++s)
            for (int p = 0; p <= k + 1; ++p)
                for (int H : {1, 2, 3, 5, 8, 17, 33})
                    for (int W : {1, 4, 7, 16, 65}) {
                        const auto& cv = Cs[(n / 3) % 7];
                        const int N = 1 + n % 3;
                        if (H + 2 * p - k >= 0 && W + 2 * p - k >= 0) {
                            bad += check(N, H, W, cv[0], cv[1], k, s, p, (H + 2 * p - k) / s + 1, (W + 2 * p - k) / s + 1, false);
                            ++n;
                        }
                        for (int op = 0; op < s && op < 3; ++op) {
                            const int Ho = (H - 1) * s - 2 * p + k + op, Wo = (W - 1) * s - 2 * p + k + op;
                            if (Ho > 0 && Wo > 0) { bad += check(N, H, W, cv[0], cv[1], k, s, p, Ho, Wo, true); ++n; }
                        }
                        if (bad > 5) return 1;
                    }
    // the shapes of the tests and the benchmark
    bad += check(3, 33, 65, 192, 4, 3, 1, 1, 33, 65, false);
    bad += check(4, 128, 128, 192, 4, 3, 1, 1, 128, 128, false);
    bad += check(2, 256, 256, 3, 1, 3, 2, 1, 128, 128, false);
    bad += check(1, 1, 65536, 192, 4, 1, 1, 0, 1, 65536, false);
    bad += check(1, 1, 4099, 192, 4, 1, 1, 0, 1, 4099, false);
    bad += check(32, 16, 16, 320, 4, 5, 1, 2, 16, 16, false);
    bad += check(2, 1024, 1024, 2, 1, 3, 1, 1, 1024, 1024, false);
    printf("%d geometries, %d bad\n", n + 7, bad);
    return bad != 0;
}
