"""CPU reference of the input-gradient Functions of hipops/autograd.py: plain torch / numpy in NCHW, no GPU and no import of the library.
tests/test_tape_reference.py pins it; tests/test_gpu_tape_functions.py compares the Functions with it.

For every conv-like operation (conv, transposed conv, the GDN norm pool, Linear) three things are computed, for the value and again for
the input gradient:
  * `ref`: float64; the input gradient comes from torch autograd of the float64 forward for the given upstream gradient;
  * `S = sum |a| |b|` per output element: the same operation on absolute values (a bias enters as |bias|), float64;
  * `q`: the error of the reference's OWN float32 chain in units of u S, u = 2^-24.  The chain multiplies in float32 and adds the products
    strictly one after the other (numpy.cumsum in float32 over the unfolded products, tap-major and channel-minor, then the bias, then the
    activation's slope).  A transposed conv / an input gradient is unfolded from the zero-inserted tensor with the flipped taps, so the
    structural zeros are added too (exactly).  Where a case has more than 2^26 products the chain is formed for evenly spaced output pixels
    (first and last included), all channels: a maximum over fewer elements is never larger, the bound below never wider.

The bound of an element is  (2 q + d) u S + 2 u |ref|  (`bound`): the factor 2 is the margin for another summation order, d = 0 on the
fp32 / thin kernels, d = 2 on the split-bf16 kernel (its three-way split is exact, the three dropped products are <= 2^-24 |a b| each).
Nothing in it comes from a kernel.

LeakyReLU / ReLU: the derivative jumps at 0, so `mask(d)` marks the elements whose float64 pre-activation is within its own bound of 0.
Outside the mask the kernel must take the reference's branch; the input gradient is the autograd gradient for a given branch tensor
(the reference's own, unless a caller passes the one a kernel took inside the mask)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
F32 = np.float32
F64 = torch.float64
SLOPE = {"none": None, "lrelu": 0.01, "relu": 0.0}
MAX_PRODUCTS = 1 << 26
MASK_CAP = 0.005                     # a case may lose at most this fraction of its elements to the kink mask


def bound(S, ref, q, d):
    return (2.0 * q + d) * U * S + 2.0 * U * ref.abs()


def rows_of(t):
    """[B,C,H,W] -> [B*H*W, C]: the order in which `chain32` numbers output pixels"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def zero_insert(g, stride, q, oph, opw):
    """[B,C,H,W] -> [B,C,(H-1)s+1+2q+oph,(W-1)s+1+2q+opw]: g at (q + h s, q + w s), the output padding below / right"""
    B, C, H, W = g.shape
    out = g.new_zeros(B, C, (H - 1) * stride + 1 + 2 * q + oph, (W - 1) * stride + 1 + 2 * q + opw)
    out[:, :, q:q + (H - 1) * stride + 1:stride, q:q + (W - 1) * stride + 1:stride] = g
    return out


def chain32(a, w, bias, stride, pad, slope=None, max_products=MAX_PRODUCTS):
    """Sequential float32 chain of conv2d(a [B,C,H,W], w [O,C,KH,KW]) + bias: -> (idx, values [len(idx), O]) with idx into `rows_of`.
    `slope` [B,O,Ho,Wo] float32 (or None) multiplies the result last (the activation's branch)."""
    O, C, KH, KW = w.shape
    cols = F.unfold(a.float(), (KH, KW), padding=pad, stride=stride)                  # [B, C*KH*KW, L], channel-major
    B, _, Lp = cols.shape
    wm = w.float().permute(0, 2, 3, 1).reshape(O, -1).numpy()                          # [O, taps * C], tap-major
    n, M = wm.shape[1], B * Lp
    keep = max(1, max_products // (O * n))
    idx = torch.arange(M) if M <= keep else torch.unique(torch.linspace(0, M - 1, keep).round().long())
    A = cols.permute(0, 2, 1)[idx // Lp, idx % Lp].view(-1, C, KH * KW).permute(0, 2, 1).reshape(-1, n).numpy()
    out = np.empty((len(idx), O), F32)
    step = max(1, (1 << 24) // (O * n))
    for i in range(0, len(idx), step):
        out[i:i + step] = np.cumsum(A[i:i + step, None, :] * wm[None], axis=-1, dtype=F32)[..., -1]
    if bias is not None:
        out = out + bias.float().numpy()[None]
    if slope is not None:
        out = out * rows_of(slope)[idx].numpy().astype(F32)
    return idx, torch.from_numpy(out)


def chain_q(chain, ref, S):
    """max |chain32 - ref64| / (u S) over the elements the chain was formed for (0 / 0 counts as 0)"""
    idx, c = chain
    r, s = rows_of(ref)[idx], rows_of(S)[idx]
    err = (c.double() - r).abs()
    assert bool((err[s == 0] == 0).all())
    live = s > 0
    return float((err[live] / (U * s[live])).max()) if bool(live.any()) else 0.0


def tconv_weight_as_conv(w):
    """[O,C,K,K] read by conv_transpose2d(g [B,O,..]) -> the weight [C,O,K,K] of the stride-1 conv over the zero-inserted g"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def tconv_chain32(g, w, bias, stride, pad, opad, slope=None):
    K = w.shape[2]
    return chain32(zero_insert(g.float(), stride, K - 1 - pad, *opad), tconv_weight_as_conv(w), bias, 1, 0, slope)


def conv_out_pad(H, W, K, stride, pad):
    """output_padding (h, w) with which conv_transpose2d returns the conv's input size: the rows / columns the strided conv never reached"""
    return (H + 2 * pad - K) % stride, (W + 2 * pad - K) % stride


def _slopes(pos, act):
    s = SLOPE[act]
    if s is None:
        return None, None
    return torch.where(pos, 1.0, s).double(), torch.where(pos, F32(1.0), F32(s)).float()


class TapeRef:
    """Value and input gradient of y = act(op(x)) for op = conv2d ('conv', w [Cout,Cin,K,K]) or conv_transpose2d ('tconv', w [Cin,Cout,K,K]
    with output_padding `opad`) or a Linear ('conv' with K = 1 on [rows, Cin, 1, 1]).  x, w, b, go: float32 CPU tensors."""

    def __init__(self, kind, x, w, b, stride, pad, opad=0, act="none"):
        self.kind, self.w, self.b, self.stride, self.pad, self.act = kind, w, b, stride, pad, act
        self.opad = (opad, opad) if isinstance(opad, int) else tuple(opad)
        self.x = x
        self.x64 = x.double().requires_grad_(True)
        b64 = None if b is None else b.double()
        babs = None if b is None else b64.abs()
        if kind == "conv":
            self.pre_graph = F.conv2d(self.x64, w.double(), b64, stride, pad)
            self.S_pre = F.conv2d(x.double().abs(), w.double().abs(), babs, stride, pad)
        else:
            self.pre_graph = F.conv_transpose2d(self.x64, w.double(), b64, stride, pad, output_padding=self.opad)
            self.S_pre = F.conv_transpose2d(x.double().abs(), w.double().abs(), babs, stride, pad, output_padding=self.opad)
        self.pre = self.pre_graph.detach()
        self.pos = self.pre > 0
        s64, s32 = _slopes(self.pos, act)
        self.y = self.pre if s64 is None else self.pre * s64
        self.S = self.S_pre if s64 is None else self.S_pre * s64
        chain = self._chain(x, None)
        self.q_pre = chain_q(chain, self.pre, self.S_pre)
        self.q = self.q_pre
        if s64 is not None:
            self.q = max(self.q, chain_q(self._chain(x, s32), self.y, self.S))
        self._bwd = {}

    def _chain(self, x, slope):
        if self.kind == "conv":
            return chain32(x, self.w, self.b, self.stride, self.pad, slope)
        return tconv_chain32(x, self.w, self.b, self.stride, self.pad, self.opad, slope)

    # ---- value ----
    def bound_pre(self, d):
        return bound(self.S_pre, self.pre, self.q_pre, d)

    def mask(self, d):
        """elements whose pre-activation is within its own bound of the kink"""
        if self.act == "none":
            return torch.zeros_like(self.pos)
        return self.pre.abs() <= self.bound_pre(d)

    def bound_y(self, d):
        """outside the mask (the slope scales S; ReLU's dead side is exactly 0); inside it either branch of a pre-activation within
        its bound of 0 is right: twice that bound"""
        return torch.where(self.mask(d), 2.0 * self.bound_pre(d), bound(self.S, self.y, self.q, d))

    # ---- input gradient ----
    def backward(self, go, pos=None):
        """-> dict(dx, S, q) for the upstream gradient `go` and the branch tensor `pos` (default: the reference's own)"""
        own = pos is None
        if own and "own" in self._bwd:
            return self._bwd["own"]
        pos = self.pos if own else pos
        s64, s32 = _slopes(pos, self.act)
        g64 = go.double() if s64 is None else go.double() * s64
        g32 = go.float() if s32 is None else go.float() * s32                         # the product the kernel rounds to fp32 too
        (dx,) = torch.autograd.grad(self.pre_graph, self.x64, g64, retain_graph=True)
        wabs = self.w.double().abs()
        if self.kind == "conv":
            op = conv_out_pad(self.x.shape[2], self.x.shape[3], self.w.shape[2], self.stride, self.pad)
            S = F.conv_transpose2d(g64.abs(), wabs, None, self.stride, self.pad, output_padding=op)
            chain = tconv_chain32(g32, self.w, None, self.stride, self.pad, op)
        else:
            S = F.conv2d(g64.abs(), wabs, None, self.stride, self.pad)
            chain = chain32(g32, self.w, None, self.stride, self.pad)
        out = {"dx": dx, "S": S, "q": chain_q(chain, dx, S)}
        if own:
            self._bwd["own"] = out
        return out


def bound_dx(r, d):
    return bound(r["S"], r["dx"], r["q"], d)


# ---- GDN -----------------------------------------------------------------------------------------------------------------------------------
class GdnRef:
    """y = x n^(-1/2) (GDN) or x n^(1/2) (inverse), n = beta + gamma . x^2 (gamma [C,C] >= 0 over the input channel, beta [C] > 0).
    The norm pool is the conv-like op: S_n, q_n from its chain over the fp32 squares.  The bounds of y and dx follow to first order:
      y :  |dy/dn| B_n + 8 u |y|           (B_n = bound of n; a 2 ulp reciprocal square root, the product, and a factor 2: tail_reference)
      t = dL/dn = g x (-1/2 n^-3/2 | 1/2 n^-1/2):  |dt| <= |t| (k B_n / n + 12 u), k = 3/2 | 1/2   (tail_reference.gdn_bounds)
      acc = t . gamma (1x1 conv with the transposed weight):  B_acc = bound(S_acc, acc, q_acc, d) + |dt| . gamma
      dx = g f + 2 x acc:  |g| |df/dn| B_n + 2 |x| B_acc + 2 u (3 |g f| + 3 |2 x acc| + |dx|)           (tail_reference.gdn_dx64)"""

    def __init__(self, x, gamma, beta, inverse):
        C = x.shape[1]
        self.inverse, self.x, self.gamma = inverse, x, gamma
        self.w = gamma.reshape(C, C, 1, 1)
        x64 = x.double()
        self.x64 = x64.clone().requires_grad_(True)
        n_graph = F.conv2d(self.x64 * self.x64, self.w.double(), beta.double())
        self.y_graph = self.x64 * (n_graph.sqrt() if inverse else n_graph.rsqrt())
        self.n, self.y = n_graph.detach(), self.y_graph.detach()
        self.S_n = F.conv2d(x64 * x64, self.w.double().abs(), beta.double().abs())
        self.q_n = chain_q(chain32(x * x, self.w, beta, 1, 0), self.n, self.S_n)
        self._bwd = {}

    def bound_n(self, d):
        return bound(self.S_n, self.n, self.q_n, d)

    def _dfdn(self):
        return 0.5 * (self.n.rsqrt() if self.inverse else self.n.pow(-1.5))

    def bound_y(self, d):
        return self.x.double().abs() * self._dfdn() * self.bound_n(d) + 8.0 * U * self.y.abs()

    def backward(self, go):
        key = go.data_ptr()
        if key in self._bwd:
            return self._bwd[key]
        (dx,) = torch.autograd.grad(self.y_graph, self.x64, go.double(), retain_graph=True)
        g, x, n = go.double(), self.x.double(), self.n
        t = g * x * (0.5 * n.rsqrt() if self.inverse else -0.5 * n.pow(-1.5))
        wt = self.w.transpose(0, 1).contiguous()
        acc = F.conv2d(t, wt.double())
        S_acc = F.conv2d(t.abs(), wt.double().abs())
        q_acc = chain_q(chain32(t.float(), wt, None, 1, 0), acc, S_acc)
        out = self._bwd[key] = {"dx": dx, "g": g, "t": t, "acc": acc, "S_acc": S_acc, "q_acc": q_acc, "wt": wt}
        return out

    def bound_dx(self, r, d):
        g, x, n = r["g"], self.x.double(), self.n
        k = 0.5 if self.inverse else 1.5
        dt = r["t"].abs() * (k * self.bound_n(d) / n + 12.0 * U)
        b_acc = bound(r["S_acc"], r["acc"], r["q_acc"], d) + F.conv2d(dt, r["wt"].double().abs())
        a = g * (n.sqrt() if self.inverse else n.rsqrt())
        b = 2.0 * x * r["acc"]
        return g.abs() * self._dfdn() * self.bound_n(d) + 2.0 * x.abs() * b_acc + 2.0 * U * (3 * a.abs() + 3 * b.abs() + r["dx"].abs())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def permuted(shape_nchw, gen, scale=1.0):
    """a non-contiguous NCHW tensor: drawn as [B, W, C, H] and permuted (neither NCHW- nor NHWC-contiguous)"""
    B, C, H, W = shape_nchw
    return (torch.randn(B, W, C, H, generator=gen) * scale).permute(0, 2, 3, 1)


def nhwc_view(shape_nchw, gen, scale=1.0):
    """an NCHW view of NHWC storage (the layout tensors have between the package's modules)"""
    B, C, H, W = shape_nchw
    return (torch.randn(B, H, W, C, generator=gen) * scale).permute(0, 3, 1, 2)


# Conv2dFn: name -> (B, H, W, Cin, Cout, K, stride, pad, act, forward kernel, dgrad form, dgrad kernel, flags)
#   forward / dgrad kernel: fp32 | thin | thincout | x6 ;  dgrad form: flip (stride-1 'same') | phase | zi (zero insertion)
#   flags: "raw" = the weight goes in as a tensor, not a WeightPack; "nobias" = bias None
CONV_CASES = {
    "flip_3x3_lrelu": (2, 9, 11, 36, 20, 3, 1, 1, "lrelu", "fp32", "flip", "fp32", ()),
    "flip_5x5": (1, 7, 5, 8, 8, 5, 1, 2, "none", "fp32", "flip", "fp32", ()),
    "flip_1x1_relu": (2, 6, 10, 16, 24, 1, 1, 0, "relu", "fp32", "flip", "fp32", ()),
    "s1_valid": (1, 10, 9, 12, 8, 3, 1, 0, "none", "fp32", "zi", "fp32", ()),
    "s1_pad2": (1, 8, 8, 8, 8, 3, 1, 2, "none", "fp32", "zi", "fp32", ()),
    "phase_3x3_s2": (2, 16, 12, 16, 24, 3, 2, 1, "none", "fp32", "phase", "fp32", ()),
    "phase_4x4_s2": (1, 10, 8, 8, 8, 4, 2, 1, "none", "fp32", "phase", "fp32", ()),
    "phase_3x3_s3": (1, 12, 12, 8, 8, 3, 3, 1, "none", "fp32", "phase", "fp32", ()),
    "zi_3x3_s2_odd": (2, 9, 13, 8, 12, 3, 2, 1, "none", "fp32", "zi", "fp32", ()),
    "zi_5x5_s2_odd": (1, 9, 9, 8, 8, 5, 2, 2, "none", "fp32", "zi", "fp32", ()),
    "zi_3x3_s3_rem1": (1, 11, 11, 8, 8, 3, 3, 1, "none", "fp32", "zi", "fp32", ()),
    "zi_3x3_s3_rem0": (1, 10, 10, 8, 8, 3, 3, 1, "none", "fp32", "zi", "fp32", ()),
    "mixed_9x10": (1, 9, 10, 8, 8, 3, 2, 1, "none", "fp32", "zi", "fp32", ()),
    "mixed_10x9": (1, 10, 9, 8, 8, 3, 2, 1, "none", "fp32", "zi", "fp32", ()),
    "thin_stem_lrelu": (1, 32, 32, 3, 32, 5, 2, 2, "lrelu", "thin", "phase", "thincout", ()),
    "thincout_fwd": (1, 16, 32, 192, 12, 3, 1, 1, "none", "thincout", "flip", "fp32", ()),
    "x6_s1_lrelu": (1, 61, 64, 192, 192, 3, 1, 1, "lrelu", "x6", "flip", "x6", ()),
    "x6_s2_phase": (1, 122, 128, 192, 192, 3, 2, 1, "none", "x6", "phase", "x6", ()),
    "raw_tensor": (2, 9, 11, 36, 20, 3, 1, 1, "none", "fp32", "flip", "fp32", ("raw",)),
    "no_bias": (2, 9, 13, 8, 12, 3, 2, 1, "lrelu", "fp32", "zi", "fp32", ("nobias",)),
}
MIXED_CASES = ("mixed_9x10", "mixed_10x9")

# ConvTranspose2dFn: name -> (B, H, W, Cin, Cout, K, stride, pad, output_padding, act, forward form, forward kernel, backward kernel)
TCONV_CASES = {
    "phase_5x5_lrelu": (2, 9, 7, 12, 20, 5, 2, 2, 1, "lrelu", "phase", "fp32", "fp32"),
    "phase_3x3_relu": (1, 8, 8, 32, 16, 3, 2, 1, 1, "relu", "phase", "fp32", "fp32"),
    "phase_4x4": (2, 6, 5, 8, 8, 4, 2, 1, 0, "none", "phase", "fp32", "fp32"),
    "zi_3x3_s1": (1, 7, 7, 16, 24, 3, 1, 1, 0, "none", "zi", "fp32", "fp32"),
    "zi_3x3_s2_lrelu": (1, 7, 6, 8, 12, 3, 2, 1, 0, "lrelu", "zi", "fp32", "fp32"),
    "zi_3x3_s1_relu": (1, 5, 5, 8, 8, 3, 1, 1, 0, "relu", "zi", "fp32", "fp32"),
    "x6_5x5_s2": (1, 32, 32, 192, 192, 5, 2, 2, 1, "none", "phase", "x6", "fp32"),
}

# GDNFn: name -> (B, H, W, C, inverse, flags); "span" = token magnitudes e^(+-4); "raw" = gamma / beta as tensors, not a pack
GDN_CASES = {f"{'igdn' if inv else 'gdn'}_c{C}_{H}x{W}": (B, H, W, C, inv, ())
             for C in (8, 36, 192) for (B, H, W) in ((2, 7, 9), (1, 16, 16)) for inv in (False, True)}
GDN_CASES.update({"gdn_c36_span": (2, 7, 9, 36, False, ("span",)), "igdn_c36_span": (2, 7, 9, 36, True, ("span",)),
                  "gdn_c36_raw": (2, 7, 9, 36, False, ("raw",)), "igdn_c8_raw": (1, 16, 16, 8, True, ("raw",))})

# LinearFn: name -> (input shape, Cout, forward on linear_h2, backward on linear_h2, flags); "grad" = a gradient-like input (1e-6,
# token magnitudes e^(+-6))
LINEAR_CASES = {
    "3d_conv_path": ((2, 50, 36), 20, False, False, ()),
    "4d_conv_path": ((3, 5, 7, 16), 24, False, False, ()),
    "h2_192_to_96": ((4096, 192), 96, True, True, ()),
    "h2_4160": ((4160, 192), 192, True, True, ()),
    "large_unsupported_4097": ((4097, 192), 192, False, False, ()),
    "below_threshold_4032": ((4032, 192), 192, False, False, ()),
    "h2_grad_like": ((4096, 192), 192, True, True, ("grad",)),
}
H2_TOKEN_TOL = 2e-6                  # test_linear_h2_per_token_scale_matches_float64: of each token's own largest reference output
MAXNORM = {"x6": (2e-6, 1e-7), "fp32": (5e-6, 0.0), "thin": (5e-6, 0.0), "thincout": (5e-6, 0.0)}      # rel of max |ref|, abs
D_OF = {"x6": 2, "fp32": 0, "thin": 0, "thincout": 0}


def _seed(name):
    return 1000 + sum((i + 1) * ord(c) for i, c in enumerate(name))


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """-> dict(x, w [Cout,Cin,K,K], b, go (non-contiguous), ref: TapeRef) of one CONV_CASES entry, built once"""
    B, H, W, Cin, Cout, K, s, p, act, _, _, _, flags = CONV_CASES[name]
    gen = torch.Generator().manual_seed(_seed(name))
    x = nhwc_view((B, Cin, H, W), gen) if len(name) % 2 else torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, K, K, generator=gen) / (Cin * K * K) ** 0.5
    b = None if "nobias" in flags else torch.randn(Cout, generator=gen) * 0.1
    ref = TapeRef("conv", x, w, b, s, p, act=act)
    go = permuted(tuple(ref.pre.shape), gen)
    return {"x": x, "w": w, "b": b, "go": go, "ref": ref}


@functools.lru_cache(maxsize=None)
def tconv_case(name):
    """-> dict(x, w [Cin,Cout,K,K], b, go, ref) of one TCONV_CASES entry"""
    B, H, W, Cin, Cout, K, s, p, op, act, _, _, _ = TCONV_CASES[name]
    gen = torch.Generator().manual_seed(_seed(name))
    x = nhwc_view((B, Cin, H, W), gen) if len(name) % 2 else torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cin, Cout, K, K, generator=gen) / (Cin * K * K / (s * s)) ** 0.5
    b = torch.randn(Cout, generator=gen) * 0.1
    ref = TapeRef("tconv", x, w, b, s, p, op, act)
    go = permuted(tuple(ref.pre.shape), gen)
    return {"x": x, "w": w, "b": b, "go": go, "ref": ref}


@functools.lru_cache(maxsize=None)
def gdn_case(name):
    """-> dict(x, gamma [C,C], beta [C], go, ref: GdnRef).  gamma = 0.1 I + 0.01 rand, beta in [1, 2] (as the 192-channel tape test)"""
    B, H, W, C, inverse, flags = GDN_CASES[name]
    gen = torch.Generator().manual_seed(_seed(name))
    x = nhwc_view((B, C, H, W), gen)
    if "span" in flags:
        x = x * torch.exp(8.0 * torch.rand(B, 1, H, W, generator=gen) - 4.0)
    gamma = 0.1 * torch.eye(C) + 0.01 * torch.rand(C, C, generator=gen)
    beta = 1.0 + torch.rand(C, generator=gen)
    ref = GdnRef(x, gamma, beta, inverse)
    go = permuted((B, C, H, W), gen)
    return {"x": x, "gamma": gamma, "beta": beta, "go": go, "ref": ref}


@functools.lru_cache(maxsize=None)
def linear_case(name):
    """-> dict(x [..., Cin] (non-contiguous), w [Cout,Cin], b, go [..., Cout] (non-contiguous), ref: TapeRef over [rows, Cin, 1, 1])"""
    shape, Cout, _, _, flags = LINEAR_CASES[name]
    Cin = shape[-1]
    gen = torch.Generator().manual_seed(_seed(name))
    lead = tuple(shape[:-1])
    x = torch.randn((Cin,) + lead, generator=gen).permute(*range(1, len(shape)), 0)     # channels-first storage: non-contiguous
    go = torch.randn((Cout,) + lead, generator=gen).permute(*range(1, len(shape)), 0)
    if "grad" in flags:
        go = go * 1e-6 * torch.exp(12.0 * torch.rand(lead + (1,), generator=gen) - 6.0)
        go[3] = 0.0                                                                    # a token of zeros: exact zeros out
    w = torch.randn(Cout, Cin, generator=gen) / Cin ** 0.5
    b = torch.randn(Cout, generator=gen) * 0.1
    ref = TapeRef("conv", x.reshape(-1, Cin, 1, 1), w.reshape(Cout, Cin, 1, 1), b, 1, 0)
    return {"x": x, "w": w, "b": b, "go": go, "ref": ref}
