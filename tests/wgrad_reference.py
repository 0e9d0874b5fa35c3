"""CPU reference of the fp32-input weight-gradient kernels behind rdo_conv2d_wgrad (csrc/conv_wgrad.hip, conv_wgrad_x6.hip, conv_thin.hip,
conv_thincout.hip, the token-matrix kernel of conv_wgrad_h2.hip), of rdo_reduce_slabs and of the transposed-conv route (pixel_unshuffle ->
phase-conv weight gradient -> rdo_tconv_fold): plain torch / numpy, NHWC as the kernels see their operands, no GPU and no import of the
library.  tests/test_wgrad_reference.py pins it; tests/test_gpu_wgrad_parity.py compares the kernels with it.

For x [B,H,W,Cin], dy [B,Ho,Wo,Cout], (K, stride, pad), `square_input` and a set of output pixels (a range [m0, m1) of m = (b Ho + ho) Wo + wo,
or an index tensor in ascending order; default: all) `WgradRef.part` gives
  * `ref`: float64 dw[co][kh][kw][ci] = sum_m dy[m][co] x[pix(m,kh,kw)][ci] (x^2 when squared; zero outside the image);
  * `S`:   the same sum over |dy| |x| (|dy| x^2), float64;
  * `q`:   the error of the reference's OWN sequential float32 chain over the same pixels in ascending m (float32 square, float32 product,
           numpy.cumsum in float32), in units of u S, u = 2^-24.  Where a case has more than MAX_PRODUCTS products the chain is formed for
           evenly spaced output elements (first and last included), the same ones for every pixel set of the case, as tape_reference.chain32
           subsamples pixels: a maximum over fewer elements is never larger, the bound never wider.
The bound of an element is tape_reference.bound:  (2 q + d) u S + 2 u |ref|,  d = D_OF[kernel] (0 on fp32 / thin / thin-Cout, 2 on the
split-bf16 kernel).  Nothing in it comes from a kernel.

Slabs (`chunks`, `thincout_patches`): which pixels a slab owns, restated from the launchers.
Transposed conv: float64 dW of F.conv_transpose2d by autograd in both weight layouts of ops.TconvPhase, `tconv_phase` (its window / index
tables as pure Python), `unshuffle` and `fold` (the gather rdo_tconv_fold performs).

Two input families, drawn on the CPU with a seed fixed by the case's name (`inputs`):
  * 'randn': x ~ randn, dy ~ 0.1 randn; where a tensor has two channels or more its first is scaled by 1e-3 and its last by 1e3, so that
    max |ref| belongs to one corner of the weight and the max-norm cannot stand in for the per-element bound;
  * 'exact': integers in [-3, 3], about a quarter of them zero.  max S < 2^24 over the case table (27 * 4128 ~ 1.1e5 squared at M = 4128), so
    every product and partial sum is a float32 integer in any order; the three-way bf16 split and a power-of-two-scaled fp16 split of
    such values are exact: a correct kernel returns float32(ref) bit for bit."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tape_reference import D_OF, MAX_PRODUCTS, U, _seed, bound  # noqa: F401  (U, bound, D_OF: the project's own, not restated)

F32 = np.float32
PK = 32          # pixels per reduction step of the fp32, split-bf16, token-matrix and scalar thin kernels
PK_THIN_MFMA = 8


# ---- which pixels a slab owns ---------------------------------------------------------------------------------------------------------------
def chunks(M, ns, step=PK):
    """[(m0, m1)] of the ns slabs: chunk c owns [c mchunk, min(M, (c + 1) mchunk)), mchunk = ceil(ceil(M / ns) / step) step
    (rdo_conv2d_wgrad, rdo_launch_thin_wgrad; step = 8 for thin_wgrad_mfma_kernel).  Trailing chunks may be empty: (M, M)."""
    per = -(-M // ns)
    mchunk = -(-per // step) * step
    return [(min(M, c * mchunk), min(M, (c + 1) * mchunk)) for c in range(ns)]


def thincout_patches(B, H, W):
    """[index tensor] of the pixels of every 16 x 16 patch in the order thincout_wgrad_kernel numbers them (patch_of, conv_thincout.hip):
    id = (b (H / 16) + patch row) (W / 16) + patch column -- image slowest, then the patch row, the patch column fastest.  One slab each."""
    out = []
    m = torch.arange(B * H * W).view(B, H, W)
    for b in range(B):
        for pr in range(H // 16):
            for pc in range(W // 16):
                out.append(m[b, 16 * pr:16 * pr + 16, 16 * pc:16 * pc + 16].reshape(-1))      # ascending m
    return out


# ---- the weight gradient --------------------------------------------------------------------------------------------------------------------
class Part:
    __slots__ = ("ref", "S", "q")

    def __init__(self, ref, S, q):
        self.ref, self.S, self.q = ref, S, q

    def bound(self, d):
        return bound(self.S, self.ref, self.q, d)


class WgradRef:
    """x [B,H,W,Cin], dy [B,Ho,Wo,Cout]: float32 CPU tensors (NHWC)."""

    def __init__(self, x, dy, K, stride, pad, square_input=False, max_products=MAX_PRODUCTS):
        B, H, W, Cin = x.shape
        _, Ho, Wo, Cout = dy.shape
        assert Ho == (H + 2 * pad - K) // stride + 1 and Wo == (W + 2 * pad - K) // stride + 1 and dy.shape[0] == B
        self.shape_w = (Cout, K, K, Cin)
        self.M, self.n = B * Ho * Wo, K * K * Cin

        def im2col(t):                                                                  # [B,H,W,Cin] -> [M, taps * Cin], tap-major
            cols = F.unfold(t.permute(0, 3, 1, 2), (K, K), padding=pad, stride=stride)  # [B, Cin * taps, L], channel-major
            return cols.view(B, Cin, K * K, Ho * Wo).permute(0, 3, 2, 1).reshape(self.M, self.n).contiguous()

        x32 = x.float()
        self.X32 = im2col(x32 * x32 if square_input else x32).numpy()                   # the float32 square is the chain's own first step
        x64 = x.double()
        self.X64 = im2col(x64 * x64 if square_input else x64)
        self.Y32 = dy.float().reshape(self.M, Cout).contiguous().numpy()
        self.Y64 = dy.double().reshape(self.M, Cout)
        E = Cout * self.n
        keep = max(1, max_products // max(1, self.M))
        self.eidx = np.arange(E) if E <= keep else np.unique(np.linspace(0, E - 1, keep).round().astype(np.int64))
        self._parts = {}

    def _rows(self, sel):
        if sel is None:
            return slice(0, self.M), ("all",)
        if isinstance(sel, tuple):
            return slice(sel[0], sel[1]), ("range",) + tuple(sel)
        idx = torch.as_tensor(sel, dtype=torch.long)
        assert bool((idx[1:] > idx[:-1]).all())
        return idx, ("idx", int(idx[0]), int(idx[-1]), int(idx.numel()), int(idx.sum()))

    def chain32(self, sel=None):
        """-> float32 [len(eidx)]: sum over the pixels of `sel`, ascending, of float32 products, added one after the other from 0"""
        rows, _ = self._rows(sel)
        rows = rows if isinstance(rows, slice) else rows.numpy()
        Y, X = self.Y32[rows], self.X32[rows]
        out = np.zeros(len(self.eidx), F32)
        if Y.shape[0] == 0:
            return out
        step = max(1, (1 << 24) // Y.shape[0])
        for i in range(0, len(self.eidx), step):
            e = self.eidx[i:i + step]
            out[i:i + step] = np.cumsum(Y[:, e // self.n] * X[:, e % self.n], axis=0, dtype=F32)[-1]
        return out

    def products32(self, sel=None):
        """float32 products [pixels, len(eidx)] of `sel` (for the other summation orders of the admission test)"""
        rows, _ = self._rows(sel)
        rows = rows if isinstance(rows, slice) else rows.numpy()
        return self.Y32[rows][:, self.eidx // self.n] * self.X32[rows][:, self.eidx % self.n]

    def part(self, sel=None):
        rows, key = self._rows(sel)
        if key not in self._parts:
            Y, X = self.Y64[rows], self.X64[rows]
            ref = (Y.t() @ X).view(self.shape_w)
            S = (Y.abs().t() @ X.abs()).view(self.shape_w)
            c = torch.from_numpy(self.chain32(sel)).double()
            r, s = ref.reshape(-1)[self.eidx], S.reshape(-1)[self.eidx]
            err = (c - r).abs()
            assert bool((err[s == 0] == 0).all())
            live = s > 0
            q = float((err[live] / (U * s[live])).max()) if bool(live.any()) else 0.0
            self._parts[key] = Part(ref, S, q)
        return self._parts[key]


# ---- transposed conv ------------------------------------------------------------------------------------------------------------------------
def tconv_phase(K, stride, pad, flipped):
    """ops.TconvPhase(K, stride, pad, flipped) restated: dict(pad, Kp, S2, inv) with inv[tap of the kernel-layout weight [K][K]] = index
    into the phase weight's [s^2][Kp][Kp].  Output row a + s i of a transposed conv reads input row i + d through tap kh for the pairs
    (d, kh) of phase a: kh = r + s t, d = q - t with r = (a + pad) % s, q = (a + pad) // s."""
    s = stride
    win = []
    for a in range(s):
        r, q = (a + pad) % s, (a + pad) // s
        win.append([(q - t, r + s * t) for t in range(K) if r + s * t < K])
    ds = [d for w in win for d, _ in w]
    pp = max(max(ds), -min(ds), 0)
    Kp = 2 * pp + 1
    fl = (lambda k: K - 1 - k) if flipped else (lambda k: k)
    inv = [-1] * (K * K)
    for a in range(s):
        for b in range(s):
            for dh, kh in win[a]:
                for dw, kw in win[b]:
                    inv[fl(kh) * K + fl(kw)] = ((a * s + b) * Kp + dh + pp) * Kp + dw + pp
    assert min(inv) >= 0
    return {"pad": pp, "Kp": Kp, "S2": s * s, "inv": inv}


def unshuffle(dy, r):
    """[B, H r, W r, C] -> [B, H, W, C r r], channel c r r + dy r + dx (rdo_pixel_shuffle, inverse)"""
    B, Hr, Wr, Cc = dy.shape
    H, W = Hr // r, Wr // r
    return dy.view(B, H, r, W, r, Cc).permute(0, 1, 3, 5, 2, 4).reshape(B, H, W, Cc * r * r).contiguous()


def fold(wp, ph, Cout, K):
    """[..., Cout s^2, Kp, Kp, Cin] -> [..., Cout, K, K, Cin]: out[co][tap] = wp[co][inv[tap]] (what rdo_tconv_fold gathers, per slab)"""
    lead, Cin = tuple(wp.shape[:-4]), wp.shape[-1]
    flat = wp.reshape(lead + (Cout, ph["S2"] * ph["Kp"] * ph["Kp"], Cin))
    return flat[..., torch.tensor(ph["inv"]), :].reshape(lead + (Cout, K, K, Cin))


def tconv_dw64(x, dy, K, stride, pad, opad, flipped):
    """float64 dL/dW of y = F.conv_transpose2d(x, W, stride, pad, output_padding) for dL/dy = dy, by autograd; x [B,H,W,Cin], dy
    [B,Ho,Wo,Cout] NHWC -> kernel layout [Cout][K][K][Cin] (`flipped`: taps stored as [K-1-kh][K-1-kw], the engine's; else as in W)"""
    Cin, Cout = x.shape[3], dy.shape[3]
    Wt = torch.zeros(Cin, Cout, K, K, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), Wt, None, stride, pad, output_padding=opad)
    (g,) = torch.autograd.grad(y, Wt, dy.double().permute(0, 3, 1, 2))
    if flipped:
        g = g.flip(2, 3)
    return g.permute(1, 2, 3, 0).contiguous()


# ---- inputs and the case table --------------------------------------------------------------------------------------------------------------
def _draw(shape, gen, family, scale):
    if family == "exact":
        v = torch.randint(-3, 4, shape, generator=gen).float()
        return v * (torch.rand(shape, generator=gen) >= 0.125).float()                  # 1/7 + 6/7 * 1/8 = a quarter zeros
    v = torch.randn(shape, generator=gen) * scale
    if shape[-1] >= 2:
        v[..., 0] *= 1e-3
        v[..., -1] *= 1e3
    return v


def inputs(name, family, x_shape, dy_shape):
    gen = torch.Generator().manual_seed(_seed(name + ":" + family))
    return _draw(tuple(x_shape), gen, family, 1.0), _draw(tuple(dy_shape), gen, family, 0.1)


FAMILIES = ("randn", "exact")

# name -> (B, H, W, Cin, Cout, K, stride, pad, square_input, kernel, flags, slab counts)
#   kernel: the launch the case must reach -- fp32_64v | fp32_64s | fp32_192v | fp32_192s (conv_wgrad_kernel<64|192, vec|scalar loads>) |
#           x6 (conv_wgrad_x6w8_kernel) | thin_s4 | thin_s32 (thin_wgrad_kernel<4|32, 8>) | thin_m4 | thin_m6 | thin_m8
#           (thin_wgrad_mfma_kernel<CT>) | thincout1 | thincout2 | thincout3 (thincout_wgrad_kernel<NT>) | h2 (linear_wgrad_h2_kernel)
#   flags:  "big" = rdo_debug_force_wgrad_choice(1, -1); "misalign" = x starts one float past a 16-byte boundary; "mfma_off" =
#           set_tuning("thin_mfma", 0)
#   slab counts: None = the library's own count
CASES = {
    # fp32 MFMA <64,64,vec>
    "f64v_5x5_s2": (3, 5, 7, 36, 20, 5, 2, 2, False, "fp32_64v", (), (None,)),
    "f64v_tiles_2x3": (2, 6, 6, 68, 132, 3, 1, 1, False, "fp32_64v", (), (None, 1, 2, 4)),        # M = 72: ns 2 -> 64 + 8, ns 4 -> one empty
    "f64v_1x1_sq": (1, 4, 4, 8, 8, 1, 1, 0, True, "fp32_64v", (), (None,)),
    # fp32 MFMA <64,64,scalar>: by shape, and by pointer alignment alone
    "f64s_6_to_10": (2, 7, 5, 6, 10, 3, 1, 1, False, "fp32_64s", (), (None, 3)),
    "f64s_misaligned": (1, 4, 4, 8, 8, 1, 1, 0, True, "fp32_64s", ("misalign",), (None,)),
    # fp32 MFMA <192,192,...>, forced at Wo = 7 (the split-bf16 predicate stays false)
    "f192v": (2, 6, 7, 196, 200, 3, 1, 1, False, "fp32_192v", ("big",), (None, 2, 5)),            # M = 84: ns 2 -> 64 + 20, ns 5 -> two empty
    "f192s": (1, 6, 7, 194, 30, 3, 1, 1, False, "fp32_192s", ("big",), (None,)),
    # split-bf16, forced big
    "x6_m240": (3, 5, 16, 20, 36, 3, 1, 1, False, "x6", ("big",), (None, 3, 9)),                 # 7.5 steps; ns 9 -> 32-pixel chunks, one empty
    "x6_5x5_s2": (1, 9, 32, 24, 196, 5, 2, 2, False, "x6", ("big",), (None,)),                    # Ho x Wo = 5 x 16, two Cout tiles
    "x6_1x1_sq": (2, 4, 16, 200, 16, 1, 1, 0, True, "x6", ("big",), (None, 2)),
    "x6_unforced_4096": (1, 64, 64, 160, 160, 3, 1, 1, False, "x6", (), (None,)),                # the real predicate at its threshold
    # thin
    "thin_s4_s2": (2, 9, 9, 3, 70, 1, 2, 0, False, "thin_s4", (), (None, 2)),
    "thin_s4_cin4": (1, 8, 8, 4, 64, 1, 1, 0, False, "thin_s4", (), (None,)),
    "thin_m4_cin1": (1, 7, 9, 1, 70, 3, 1, 1, False, "thin_m4", (), (None, 3)),
    "thin_m6_cin2_s2": (2, 9, 7, 2, 129, 3, 2, 1, False, "thin_m6", (), (None,)),                  # an 18-value patch
    "thin_m6_192": (1, 6, 6, 3, 192, 3, 1, 1, False, "thin_m6", (), (None, 5)),                   # M = 36, ns 5 -> 8-pixel chunks, the last with 4
    "thin_m8_193": (1, 6, 6, 3, 193, 3, 1, 1, False, "thin_m8", (), (None, 2)),
    "thin_m8_5x5": (1, 5, 5, 1, 256, 5, 1, 2, False, "thin_m8", (), (None, 4)),                   # M = 25, ns 4 -> the last chunk is one pixel
    "thin_s32_260": (1, 9, 11, 3, 260, 3, 1, 1, False, "thin_s32", (), (None, 2)),
    "thin_s32_mfma_off": (1, 6, 6, 3, 192, 3, 1, 1, False, "thin_s32", ("mfma_off",), (None, 5)),
    # thin-Cout: one slab per 16 x 16 patch; NT = 1, 2, 3 by Cin / 16
    "thincout_16_to_1": (1, 16, 16, 16, 1, 3, 1, 1, False, "thincout1", (), (None,)),
    "thincout_32_to_3": (2, 16, 32, 32, 3, 3, 1, 1, False, "thincout2", (), (None,)),
    "thincout_48_to_16": (1, 32, 16, 48, 16, 3, 1, 1, False, "thincout3", (), (None,)),
    "thincout_shape_given_ns": (1, 16, 16, 16, 1, 3, 1, 1, False, "fp32_64s", (), (2,)),            # ns != patches: the 64 x 64 kernel
    # token matrix [tokens, 1, 1, Cin]
    "h2_4096_96": (4096, 1, 1, 96, 96, 1, 1, 0, False, "h2", (), (None,)),
    "h2_4096_96_sq": (4096, 1, 1, 96, 96, 1, 1, 0, True, "h2", (), (None,)),
    "h2_4128_192_96": (4128, 1, 1, 192, 96, 1, 1, 0, False, "h2", (), (None, 5)),
    "h2_4128_192_96_sq": (4128, 1, 1, 192, 96, 1, 1, 0, True, "h2", (), (None,)),
}
TAG_OF = {"fp32_64v": "conv_wgrad_64x64", "fp32_64s": "conv_wgrad_64x64", "fp32_192v": "conv_wgrad_192x192", "fp32_192s": "conv_wgrad_192x192",
          "x6": "conv_wgrad_x6_192x192", "h2": "linear_wgrad_h2", "thin_s4": "conv_thin_wgrad", "thin_s32": "conv_thin_wgrad",
          "thin_m4": "conv_thin_wgrad", "thin_m6": "conv_thin_wgrad", "thin_m8": "conv_thin_wgrad", "thincout1": "conv_thincout_wgrad",
          "thincout2": "conv_thincout_wgrad", "thincout3": "conv_thincout_wgrad"}
# the figure the suite already holds for the slab sum of each kernel, of max |ref| (test_conv_wgrad_matches_fp64 and its kin): taken over
MAXNORM = {"fp32": 3e-6, "thin": 3e-6, "thincout": 3e-6, "x6": 1e-5, "h2": 2e-6}


def family_of(kernel):
    """kernel -> the key of D_OF / MAXNORM / FIGURES"""
    return "fp32" if kernel.startswith("fp32") else ("thincout" if kernel.startswith("thincout") else kernel.split("_")[0])


def out_hw(H, W, K, stride, pad):
    return (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1


def slab_step(kernel):
    return PK_THIN_MFMA if kernel.startswith("thin_m") else PK


def slab_sets(name, ns):
    """the pixel sets of the ns slabs of a case: ranges (m0, m1), or index tensors for the thin-Cout patches"""
    B, H, W, Cin, Cout, K, s, p, sq, kernel, flags, _ = CASES[name]
    Ho, Wo = out_hw(H, W, K, s, p)
    if kernel.startswith("thincout"):
        sets = thincout_patches(B, H, W)
        assert len(sets) == ns
        return sets
    return chunks(B * Ho * Wo, ns, slab_step(kernel))


@functools.lru_cache(maxsize=None)
def case(name, family):
    """-> dict(x, dy, ref: WgradRef) of one CASES entry, built once and left unchanged"""
    B, H, W, Cin, Cout, K, s, p, sq, kernel, flags, _ = CASES[name]
    Ho, Wo = out_hw(H, W, K, s, p)
    x, dy = inputs(name, family, (B, H, W, Cin), (B, Ho, Wo, Cout))
    return {"x": x, "dy": dy, "ref": WgradRef(x, dy, K, s, p, sq)}


# transposed-conv route at x [2,5,6,12] -> dy [2,10,12,8]: name -> (K, stride, pad, output_padding, flipped, slab count of the phase conv)
TCONV_SHAPE = (2, 5, 6, 12, 8)
TCONV_CASES = {
    "tconv_5x5": (5, 2, 2, 1, True, 3),
    "tconv_3x3": (3, 2, 1, 1, True, 4),
    "tconv_4x4": (4, 2, 1, 0, True, 3),
    "tconv_5x5_unflipped": (5, 2, 2, 1, False, 3),
}
TCONV_GEOMETRIES = ((5, 2, 2), (3, 2, 1), (4, 2, 1))


@functools.lru_cache(maxsize=None)
def tconv_case(name, family):
    """-> dict(x, dy [B, sH, sW, Cout], dyp (unshuffled), ph, ref: WgradRef of the phase conv, dw: float64 autograd dW in kernel layout)"""
    K, s, p, op, flipped, _ = TCONV_CASES[name]
    B, H, W, Cin, Cout = TCONV_SHAPE
    x, dy = inputs(name, family, (B, H, W, Cin), (B, H * s, W * s, Cout))
    ph = tconv_phase(K, s, p, flipped)
    dyp = unshuffle(dy, s)
    return {"x": x, "dy": dy, "dyp": dyp, "ph": ph, "ref": WgradRef(x, dyp, ph["Kp"], 1, ph["pad"]),
            "dw": tconv_dw64(x, dy, K, s, p, op, flipped)}
