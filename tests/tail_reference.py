"""CPU reference of the unit-tail kernels (csrc/elementwise.hip: gather_qdrop, lp2_loss_grad, lp_loss_grad; csrc/fused_tail.hip): plain
torch / numpy over NHWC tensors, no GPU and no import of the library.  tests/test_tail_reference.py pins it to float64 autograd of the
oracle; tests/test_gpu_tail_parity.py compares the kernels with it.

Three kinds of function:
  * fp32 op-for-op emulations (`lp2`, `loss_act`, `splitk_pre`): these kernels use only IEEE add, sub, mul and compare and their files
    are built with -ffp-contract=off, so numpy float32 arithmetic in the kernel's order gives the kernel's bits;
  * float64 formulas with first-order error bounds (`loss_gdn64` + `gdn_bounds`, `gdn_dx64`, `lp64`);
  * exact data movement (`gather`, `h2_planes`, `overflow_word`, `pixel_shuffle2`, `pixel_unshuffle2`).

The scalar loss is always a float64 sum (`loss64`) over the fp32 differences d = out - target: those differences are what the kernel
squares (the emulation gives them exactly; for GDN they are the launch's own `out`, itself bounded against float64, minus the target), so
the comparison with the kernel's log row measures the products, the order of the additions and the two scalings, nothing else.

Where the kernel takes `(idx_table, it, B)` so do these: the targets of mini-batch row b are row `idx_table[it, b]` of the cache."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import rdo_oracle as O

U = 2.0 ** -24                       # unit round-off of fp32
F32 = np.float32


def rows(cache, idx, it, B):
    """cache[idx_table[it, :B]]"""
    return cache[idx[it, :B].long()]


def inv_npix(B, ppi):
    """1 / (B * pixels per image) as the host code rounds it to fp32"""
    return F32(1.0 / (float(B) * float(ppi)))


def grad_scale(coef, B, ppi):
    """gs = coef * 2.f * inv_npix, every product rounded to fp32"""
    return F32(F32(coef) * F32(2.0)) * inv_npix(B, ppi)


def loss64(d, coef, B, ppi):
    """coef * sum d^2 / (B * ppi) in float64 over the fp32 differences `d`"""
    return float(coef) * float(d.double().pow(2).sum()) / (float(B) * float(ppi))


# ---- gather + QDrop -----------------------------------------------------------------------------------------------------------------------
def gather(cq, cf, idx, it, B, prob, seed, batch_offset=0):
    """where(keep, cq[rows], cf[rows]) with the oracle's mask.  The counter runs over the GLOBAL mini-batch: the mask is drawn for
    batch_offset + B images and the first batch_offset are sliced off."""
    _, H, W, C = cq.shape
    keep = O.qdrop_keep_mask_nhwc(int(seed), int(it), (batch_offset + B, C, H, W), float(prob))
    keep = keep.permute(0, 2, 3, 1)[batch_offset:]
    return torch.where(keep, rows(cq, idx, it, B), rows(cf, idx, it, B)).contiguous()


# ---- fp32 emulations ----------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().contiguous().numpy().astype(F32, copy=False)


def _ppi(t):
    return t[0].numel() // t.shape[-1]


def lp2(pred, tgt, idx, it, coef):
    """lp2_kernel: d = pred - y ; grad = d * gs.  -> (grad fp32, d fp32)"""
    B = pred.shape[0]
    d = _np(pred) - _np(rows(tgt, idx, it, B))
    return torch.from_numpy(d * grad_scale(coef, B, _ppi(pred))), torch.from_numpy(d)


def loss_act(pre, res, tgt, idx, it, coef, act):
    """loss_act_quad: o = act(pre) (+ res) ; d = o - y ; g = d * gs ; dp = pre > 0 ? g : slope * g   (act 0 none, 1 LeakyReLU(0.01),
    2 ReLU; the selects multiply by the slope, so a negative or zero input keeps its sign bit).  -> dict(out, grad_out, dpre, d)"""
    B = pre.shape[0]
    p = _np(pre)
    gs = grad_scale(coef, B, _ppi(pre))
    slope = F32(0.01) if act == 1 else F32(0.0)
    o = np.where(p > 0, p, slope * p) if act else p.copy()
    if res is not None:
        o = o + _np(res)
    d = o - _np(rows(tgt, idx, it, B))
    g = d * gs
    dp = np.where(p > 0, g, slope * g) if act else g.copy()
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (("out", o), ("grad_out", g), ("dpre", dp), ("d", d))}


def splitk_pre(partials, bias=None):
    """pre-activation from K-split partial sums [ks, B, H, W, C]: ((0 + slab 0) + slab 1 + ...) + bias"""
    p = _np(partials)
    acc = np.zeros_like(p[0])
    for z in range(p.shape[0]):
        acc = acc + p[z]
    if bias is not None:
        acc = acc + _np(bias)
    return torch.from_numpy(acc)


# ---- float64 formulas ---------------------------------------------------------------------------------------------------------------------
def loss_gdn64(x, n, res, tgt, idx, it, coef, inverse):
    """loss_gdn_quad in float64: f = n^(-+1/2) ; o = x f + r ; d = o - y ; g = gs d ; t = dL/dn = g * (1/2 x n^-1/2  |  -1/2 x n^-3/2).
    gs is the kernel's fp32 value.  -> dict(out, grad_out, t) and the magnitudes the bounds need (xf, d, t_over_g, gs)"""
    B = x.shape[0]
    gs = float(grad_scale(coef, B, _ppi(x)))
    x, n = x.double(), n.double()
    f = n.sqrt() if inverse else n.rsqrt()
    o = x * f
    xf = o.abs()
    if res is not None:
        o = o + res.double()
    d = o - rows(tgt, idx, it, B).double()
    g = gs * d
    tg = 0.5 * x * n.rsqrt() if inverse else -0.5 * x * n.pow(-1.5)
    return {"out": o, "grad_out": g, "t": g * tg, "xf": xf, "d": d, "t_over_g": tg.abs(), "gs": gs}


def gdn_bounds(r):
    """Per-element bounds of |fp32 kernel - float64| for out, grad_out, t: first order in u = 2^-24, 1 ulp for the reciprocal square
    root, a correctly rounded sqrt, a factor 2 for the second-order terms.
      o: the factor f (1u; its cube for t below 3u) and the product (1u) -> 4u |x f| covers both forms; the residual add u |o|
      g: the error of o, the subtraction u |d|, times gs; the product 4u |g| (with room for gs itself)
      t: the error of g through t / g, and 12u |t| for 0.5 g x (2 products), rs^3 (3 factors at 1u, 2 products), the last product."""
    e_o = 4 * U * r["xf"] + U * r["out"].abs()
    e_g = r["gs"] * (e_o + U * r["d"].abs()) + 4 * U * r["grad_out"].abs()
    e_t = e_g * r["t_over_g"] + 12 * U * r["t"].abs()
    return {"out": 2 * e_o, "grad_out": 2 * e_g, "t": 2 * e_t}


def loss_gdn32(x, n, res, tgt, idx, it, coef, inverse):
    """The same chain in fp32 on the CPU, in the kernel's order (torch's rsqrt / sqrt in place of the device's): the inputs of a GPU case
    are admissible when THIS chain stays within gdn_bounds."""
    B = x.shape[0]
    gs = torch.tensor(float(grad_scale(coef, B, _ppi(x))), dtype=torch.float32)
    half = torch.tensor(0.5, dtype=torch.float32)
    rs = n.rsqrt()
    o = x * (n.sqrt() if inverse else rs)
    if res is not None:
        o = o + res
    d = o - rows(tgt, idx, it, B)
    g = d * gs
    t = (half * g * x) * rs if inverse else (-half * g * x) * (rs * rs * rs)
    return {"out": o, "grad_out": g, "t": t}


def gdn_dx64(g, x, n, acc, inverse):
    """dx = g n^(-+1/2) + 2 x acc in float64, and the bound 2 * u * (3 |g f| + 3 |2 x acc| + |dx|)"""
    g, x, n, acc = g.double(), x.double(), n.double(), acc.double()
    a = g * (n.sqrt() if inverse else n.rsqrt())
    b = 2.0 * x * acc
    dx = a + b
    return dx, 2 * U * (3 * a.abs() + 3 * b.abs() + dx.abs())


def gdn_dx32(g, x, n, acc, inverse):
    return g * (n.sqrt() if inverse else n.rsqrt()) + (2.0 * x) * acc


def lp64(pred, tgt, idx, it, coef2, coefp, p):
    """lp_kernel in float64: loss = coef2 * sum d^2 / npix + coefp * sum |d|^p / npix and its gradient
    (2 coef2 d + coefp p |d|^(p-1) sign d) * inv_npix, with the kernel's fp32 inv_npix.  The two loss terms come from the fp32
    differences (see the module docstring).  -> (grad float64, loss of the p = 2 term, loss of the |d|^p term)"""
    B = pred.shape[0]
    npix = float(B) * float(_ppi(pred))
    y = rows(tgt, idx, it, B)
    d = pred.double() - y.double()
    grad = (2.0 * coef2 * d + coefp * p * d.abs().pow(p - 1.0) * d.sign()) * float(inv_npix(B, _ppi(pred)))
    d32 = (pred - y).double()
    return grad, coef2 * float(d32.pow(2).sum()) / npix, coefp * float(d32.abs().pow(p).sum()) / npix


# ---- planes -------------------------------------------------------------------------------------------------------------------------------
def h2_planes(x, scale):
    """int16 [2, C/16, pixels, 16] (the layout of ops.h2_empty): h1 = fp16(x s), h2 = fp16(x s - h1), both round-to-nearest-even"""
    C = x.shape[-1]
    xs = x.float().reshape(-1, C) * torch.tensor(float(scale), dtype=torch.float32)
    h1 = xs.half()
    h2 = (xs - h1.float()).half()
    return torch.stack([h.view(torch.int16).reshape(-1, C // 16, 16).permute(1, 0, 2) for h in (h1, h2)]).contiguous()


def overflow_word(x, scale):
    """fp32 bit pattern of max |x s| (what a raised overflow word holds for a finite overflow)"""
    m = (x.float() * torch.tensor(float(scale), dtype=torch.float32)).abs().max()
    return int(m.reshape(1).view(torch.int32).item())


# ---- r = 2 pixel (un)shuffle on NHWC ------------------------------------------------------------------------------------------------------
def pixel_shuffle2(x):
    """[B,H,W,4C] -> [B,2H,2W,C]"""
    return F.pixel_shuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


def pixel_unshuffle2(x):
    """[B,2H,2W,C] -> [B,H,W,4C]"""
    return F.pixel_unshuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


# ---- the inputs both test files use -------------------------------------------------------------------------------------------------------
N_TARGETS = 5        # cached images; every mini-batch is smaller
# three rows, none equal to arange(B); row 2 (it = 2) repeats an index where B allows one
IDX_TABLES = {1: [[4], [2], [3]], 2: [[4, 1], [0, 2], [3, 3]], 3: [[4, 0, 2], [1, 3, 0], [3, 4, 3]]}


def idx_table(B):
    return torch.tensor(IDX_TABLES[B], dtype=torch.int32)


# GDN cases of the GPU test: shape [B,H,W,C] and the magnitude of x (1e-3, 1, 30: norm dominated by beta, mixed, dominated by x^2)
GDN_CASES = [((3, 5, 7, 16), 1e-3), ((3, 5, 7, 48), 1.0), ((3, 5, 7, 64), 30.0), ((2, 8, 8, 192), 1.0), ((1, 2, 2, 16), 30.0),
             ((3, 5, 7, 12), 1.0)]


def gdn_inputs(shape, mag, seed=0):
    """x = randn * mag, n = 0.5 + rand + 0.1 x^2, residual and targets of the size of the output, g / acc for the dx kernels"""
    gen = torch.Generator().manual_seed(1000 + seed + shape[-1] + 7 * shape[0])
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = rn(*shape) * mag
    n = 0.5 + torch.rand(*shape, generator=gen) + 0.1 * x * x
    ysz = max(1.0, mag ** 0.5)
    return {"x": x, "n": n, "res": rn(*shape) * ysz, "tgt": rn(N_TARGETS, *shape[1:]) * ysz, "g": rn(*shape), "acc": rn(*shape) / max(1.0, mag)}
