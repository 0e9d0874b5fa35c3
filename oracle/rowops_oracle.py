"""Float64 references, first-order error units and float32 restatements of the row operations of csrc/swin.hip and the LayerNorm forward
of csrc/elementwise.hip: LayerNorm y, backward dx and dgamma, GELU and its derivative.  Sibling of oracle/attention_oracle.py; the
convention is the same: a unit is what one rounding per operation leaves in an element to first order, formed from float64 reference
quantities only (u = 2^-24), and an implementation is held to a small multiple of it.

LayerNorm of a row x[0..C): m = mean(x), d = x - m, var = mean(d^2), r = (var + eps)^-1/2, xh = d r, y = xh w + b  (two passes, as every
kernel here computes it).
  em     = u mean|x| + u |m|                       the sum (bounded by the absolute terms) and the division
  ed_c   = u |x_c| + em + u |d_c|                  THE CANCELLATION: d is the difference of two numbers of size |x|.  When the mean is far
                                                   larger than the spread (mean 100, spread 0.1), an error of u |x| in either operand is
                                                   1000 u of d, and r = 1 / spread multiplies it.  A unit relative to |d| or |y| would be wrong.
  evar   = 2 mean(|d| ed) + 2u var                 squares, their sum, the division
  erel   = evar / (2 (var + eps)) + 2u             relative error of r (the addition of eps, rsqrt to an ulp)
  exh_c  = r ed_c + |xh_c| (erel + u)
  unit y = |w_c| exh_c + u |xh_c w_c| + u |y_c|
Backward with g = dy w, a = mean(g), b = mean(g xh):  dx = r (g - a - xh b),  dgamma_c = sum over rows of dy xh.
  eg = u |g|;  ea = mean(eg) + u mean|g| + u |a|;  eb = mean(|g| exh + eg |xh| + u |g xh|) + u mean|g xh| + u |b|
  unit dx = r (eg + ea + exh |b| + |xh| eb + u (|g| + |a| + 2 |xh b|)) + |dx| (erel + u)
  dgamma: a term dy xh carries the error |dy| exh of xh and its own rounding; the kernels add the terms of a slab one after the other per
  lane (rows / (slabs x row groups) of them, at most rows / slabs) and fold lanes and waves in a tree of depth <= 4.  As in
  tests/rate_channels_reference.py, a term that passes D additions gathers at most 1.01 D u of the sum of absolute terms:
      bound dgamma_c = 1.01 (ceil(rows / slabs) + 4 + 1) u sum_rows |dy xh| + sum_rows |dy| exh          (the slabs are added in float64)
  It is a bound, not a unit: it is asserted with the factor 1.

GELU(v) = 0.5 v (1 + erf(z)), z = v / sqrt 2.  erf is good to an ulp, u |erf z|, and takes z's rounding through erf'(z) = 2 / sqrt(pi) e^(-z^2);
the sum 1 + erf z then has the ABSOLUTE error u (|erf z| + |z| erf'(z) + |1 + erf z|).  In the negative tail erf z -> -1 and 1 + erf z
cancels: the error stays u while the value goes to 0, so the result's error is 0.5 u |v|, absolute in u |v| -- in torch's float32 kernel as
much as in this one.  A unit relative to |gelu(v)| would be wrong there.
  unit gelu  = 0.5 |v| u (|erf z| + |z| erf'(z) + |1 + erf z|) + 2u |gelu(v)|
GELU'(v) = cdf + v pdf, cdf = 0.5 (1 + erf z), pdf = exp(-v^2 / 2) / sqrt(2 pi): the exponent -0.5 v v is rounded twice (absolute 2u v^2 / 2
each way, so a relative u v^2 of pdf), expf to 2 ulp, the constant, the product:
  unit gelu' = 0.5 u (|erf z| + |z| erf'(z) + |1 + erf z|) + |v| pdf u (4 + v^2) + u |gelu'(v)|
  gelu_bwd   = |dy| unit gelu' + u |dy gelu'(v)|

Float32 restatements (`layer_norm32`, `layer_norm_bwd32`, `gelu32`, `gelu_grad32`): torch on the CPU in float32 in the kernels' order of
operations.  For LayerNorm that includes the ORDER OF THE ROW SUMS (`_rowsum32`): the error of a row is dominated by the rounding of its
mean, one number per row, so a restatement that adds in another order measures another sample of that rounding, not the kernel's
arithmetic (one row of 512 channels around 100: 0.05 units with torch's blocked sum, 0.37 with the 64-lane order)."""
import math

import torch

U = 2.0 ** -24
F64 = torch.float64


def layer_norm64(x, w=None, b=None, eps=1e-5):
    """-> dict of float64 tensors: y, unit_y and the row quantities the backward needs"""
    x = x.detach().to(F64)
    C = x.shape[-1]
    w = torch.ones(C, dtype=F64) if w is None else w.detach().to(F64)
    b = torch.zeros(C, dtype=F64) if b is None else b.detach().to(F64)
    m = x.mean(-1, keepdim=True)
    d = x - m
    var = (d * d).mean(-1, keepdim=True)
    r = (var + eps) ** -0.5
    xh = d * r
    y = xh * w + b
    em = U * x.abs().mean(-1, keepdim=True) + U * m.abs()
    ed = U * x.abs() + em + U * d.abs()
    evar = 2 * (d.abs() * ed).mean(-1, keepdim=True) + 2 * U * var
    erel = evar / (2 * (var + eps)) + 2 * U
    exh = r * ed + xh.abs() * (erel + U)
    unit_y = w.abs() * exh + U * (xh * w).abs() + U * y.abs()
    return {"y": y, "unit_y": unit_y, "xh": xh, "r": r, "exh": exh, "erel": erel, "w": w}


def layer_norm_bwd64(x, w, dy, eps=1e-5, nslabs=1):
    """-> dict: dx, unit_dx [rows, C]; dgamma, bound_dgamma [C]"""
    f = layer_norm64(x, w, None, eps)
    xh, r, exh, erel, w = f["xh"], f["r"], f["exh"], f["erel"], f["w"]
    dy = dy.detach().to(F64)
    rows = xh.numel() // xh.shape[-1]
    g = dy * w
    a = g.mean(-1, keepdim=True)
    b = (g * xh).mean(-1, keepdim=True)
    dx = r * (g - a - xh * b)
    eg = U * g.abs()
    ea = eg.mean(-1, keepdim=True) + U * g.abs().mean(-1, keepdim=True) + U * a.abs()
    eb = (g.abs() * exh + eg * xh.abs() + U * (g * xh).abs()).mean(-1, keepdim=True) + U * (g * xh).abs().mean(-1, keepdim=True) + U * b.abs()
    unit_dx = r * (eg + ea + exh * b.abs() + xh.abs() * eb + U * (g.abs() + a.abs() + 2 * (xh * b).abs())) + dx.abs() * (erel + U)
    C = xh.shape[-1]
    t = (dy * xh).reshape(rows, C)
    depth = -(-rows // nslabs) + 4 + 1
    assert depth * U < 0.01
    bound = 1.01 * depth * U * t.abs().sum(0) + (dy.abs() * exh).reshape(rows, C).sum(0)
    return {"dx": dx, "unit_dx": unit_dx, "dgamma": t.sum(0), "bound_dgamma": bound}


def _rowsum32(t, order):
    """float32 sum over the last dimension in a kernel's own order.  "wave64" (layer_norm_kernel, layer_norm_bwd_kernel): lane l adds its
    channels l, l + 64, .. one after the other, then the xor butterfly 32 .. 1 (a + b == b + a: every lane holds the same sum).  "group16"
    (add_ln_kernel, ln_bwd_add_kernel): lane l of 16 adds (x + y) + (z + w) of its float4 groups l, l + 16, .., then the butterfly 8 .. 1."""
    rows, C = t.shape
    if order == "group16":
        assert C % 4 == 0
        q = t.view(rows, C // 4, 4)
        t, lanes = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]), 16
    else:
        assert order == "wave64"
        lanes = 64
    n = t.shape[1]
    pad = -n % lanes
    if pad:
        t = torch.cat([t, torch.zeros(rows, pad, dtype=t.dtype)], 1)
    t = t.view(rows, -1, lanes)
    acc = torch.zeros(rows, lanes, dtype=t.dtype)
    for k in range(t.shape[1]):
        acc = acc + t[:, k]
    idx = torch.arange(lanes)
    o = lanes // 2
    while o:
        acc = acc + acc[:, idx ^ o]
        o //= 2
    return acc[:, :1]


def layer_norm32(x, w=None, b=None, eps=1e-5, order="wave64"):
    """float32 restatement, two passes, the row sums in the order of the kernel named by `order` (`_rowsum32`): -> (y, xh, r)"""
    x = x.detach().float()
    C = x.shape[-1]
    x = x.reshape(-1, C)
    m = _rowsum32(x, order) / C
    d = x - m
    r = torch.rsqrt(_rowsum32(d * d, order) / C + eps)
    xh = d * r
    y = xh
    if w is not None:
        y = y * w.detach().float()
    if b is not None:
        y = y + b.detach().float()
    return y, xh, r


def layer_norm_bwd32(x, w, dy, eps=1e-5, order="wave64"):
    """float32 restatement of dx = rstd (g - mean g - xh mean(g xh))"""
    _, xh, r = layer_norm32(x, None, None, eps, order)
    C = x.shape[-1]
    g = dy.detach().float().reshape(-1, C) * (w.detach().float() if w is not None else 1.0)
    a = _rowsum32(g, order) / C
    b = _rowsum32(g * xh, order) / C
    return r * (g - a - xh * b)


_RSQRT2 = 0.70710678118654752
_RSQRT2PI = 0.39894228040143268


def _erf_parts(v):
    z = v * _RSQRT2
    erf = torch.erf(z)
    return U * (erf.abs() + z.abs() * (2.0 / math.sqrt(math.pi)) * torch.exp(-z * z) + (1.0 + erf).abs()), erf


def gelu64(v):
    """-> (gelu, unit) float64.  1 + erf(z) is formed as erfc(-z): float64 itself cancels in the tail below -8"""
    v = v.detach().to(F64)
    e_abs, _ = _erf_parts(v)
    y = 0.5 * v * torch.erfc(-v * _RSQRT2)
    return y, 0.5 * v.abs() * e_abs + 2 * U * y.abs()


def gelu_grad64(v):
    """-> (gelu', unit) float64"""
    v = v.detach().to(F64)
    e_abs, _ = _erf_parts(v)
    pdf = _RSQRT2PI * torch.exp(-0.5 * v * v)
    gp = 0.5 * torch.erfc(-v * _RSQRT2) + v * pdf
    return gp, 0.5 * e_abs + v.abs() * pdf * U * (4 + v * v) + U * gp.abs()


def gelu_bwd64(dy, v):
    dy = dy.detach().to(F64)
    gp, unit = gelu_grad64(v)
    return dy * gp, dy.abs() * unit + U * (dy * gp).abs()


def gelu32(v):
    v = v.detach().float()
    return 0.5 * v * (1.0 + torch.erf(v * torch.tensor(_RSQRT2, dtype=torch.float32)))


def gelu_grad32(v):
    v = v.detach().float()
    cdf = 0.5 * (1.0 + torch.erf(v * torch.tensor(_RSQRT2, dtype=torch.float32)))
    pdf = torch.tensor(_RSQRT2PI, dtype=torch.float32) * torch.exp(-0.5 * v * v)
    return cdf + v * pdf
