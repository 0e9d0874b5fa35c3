"""Float64 reference of the window attention core (csrc/swin.hip) on the kernels' own operands, with one first-order error unit per element
of every result, and a float32 restatement in the kernels' order of operations.  Row operations (LayerNorm, GELU): oracle/rowops_oracle.py.

Operands, from the header comment of swin.hip and include/rdo_ptq_hip.h.  qkv [B, H, W, 3C] in natural pixel order, channel
c = which * C + head * hd + d (which: 0 q, 1 k, 2 v); bias [heads, N, N]; scale: the float32 of the descriptor; N = ws * ws tokens per window.
Window (b, wh, ww), numbered (b * H/ws + wh) * W/ws + ww, token (ih, iw) numbered ih * ws + iw, is the pixel
    ((wh ws + ih + shift) % H, (ww ws + iw + shift) % W)
for reading q, k, v and dout and for writing out and dqkv.  With shift > 0 the token lies in band  0 if p < L - ws, 1 if p < L - shift, else 2
of each axis, p = wh ws + ih (axis length L = H) or ww ws + iw (L = W); its region is 3 * band_h + band_w, and the logit of two tokens of
different regions gets -100.  Everything here is index arithmetic on flat pixel numbers: no roll / view / permute of images, so that
tests/test_attention_reference.py can hold it against that composition.

    s_ij = scale * sum_d q_id k_jd + bias_ij + mask_ij        p_ij = exp(s_ij - max_i) / sum_j' exp(s_ij' - max_i)
    out_id = sum_j p_ij v_jd                                  probs [windows, N, N, heads]
    dP = dO V^T;  D_i = sum_j p_ij dP_ij;  dS = P o (dP - D);  dQ = scale dS K;  dK = dS^T (scale Q);  dV = P^T dO

Error units (u = 2^-24, the unit roundoff of float32).  A unit is the first-order size of the error ONE rounding per operation leaves in an
element, formed from float64 reference quantities only; an implementation is held to a small multiple c of it (tests/test_gpu_attention.py:
c = 4 x what the float32 restatement below needs on the same inputs).  Each is a sum of absolute values of the terms an error can enter by.

  score     ds_ij = u (sum_d |scale q_id k_jd| + |bias_ij| + |s_ij|)
            every product and every partial sum is bounded by the sum of the absolute terms; |bias| stands for the starting value (with the
            mask inside |s|: bias - 100 is rounded once), |s| for the result.
  prob      dp_ij = p_ij (ds_ij + sum_j' p_ij' ds_ij' + 2u |s_ij - max_i| + 4u)
            d log p_ij = ds_ij - sum_j' p_ij' ds_ij' (softmax Jacobian), taken with absolute values.  The hardware exponential evaluates
            exp2(x log2 e): the product x log2 e is rounded to float32 (relative u) and log2 e itself is a float32 constant (relative u), an
            absolute error 2u |x| log2 e of the exponent, that is a relative error 2u |x| of e^x, x = s_ij - max_i.  4u: the subtraction of the
            maximum and exp2's own ulp, the row sum (its terms are positive: relative u per level, a shuffle tree), the reciprocal and the product.
  out       do_id = sum_j (dp_ij |v_jd| + u p_ij |v_jd|)
  pv        out from GIVEN float32 probabilities: u sum_j |p_ij v_jd| (the probabilities are data, not results)
  dP        ddP_ij = u sum_d |dO_id v_jd|
  D         dD_i = sum_j (dp_ij |dP_ij| + p_ij ddP_ij + u |p_ij dP_ij|)
  dS        ddS_ij = dp_ij |dP_ij - D_i| + p_ij (ddP_ij + dD_i) + u p_ij (|dP_ij| + |D_i|)
  dQ        scale sum_j (ddS_ij |k_jd| + u |dS_ij k_jd|) + u |dQ_id|          (the trailing u: the multiplication by scale)
  dK        sum_i (ddS_ij |scale q_id| + 2u |dS_ij scale q_id|)                (2u: scale q is itself rounded)
  dV        sum_i (dp_ij |dO_id| + u p_ij |dO_id|)
A probability the float64 reference holds far below float32's normal range (1e-44) may be flushed to zero by a float32 implementation: the
tests give probabilities an additive floor of 2^-126 for that; nothing else has a floor.

Float32 restatement (`restate32`): torch on the CPU in float32, in the kernels' order: q scaled in float32 first, scores accumulated onto
bias + mask, exp of (v - max), multiplication by the reciprocal of the sum, D and dS from float32 P and dP, dQ = scale * (dS K),
dK = dS^T (scale q), dV = P^T dO.  `pv32` adds the terms of a row one after the other, as the pv kernel does.  Its worst err / unit per
result (`worst_ratio`) is what the CPU tests print and the GPU bound is built from."""
import torch

U = 2.0 ** -24
F64 = torch.float64
P_FLOOR = 2.0 ** -126


class Geom:
    def __init__(self, B, H, W, C, heads, window, shift, scale=None):
        if C % heads or H % window or W % window or not 0 <= shift < window:
            raise ValueError("bad attention geometry")
        self.B, self.H, self.W, self.C, self.heads, self.ws, self.shift = B, H, W, C, heads, window, shift
        self.N, self.hd = window * window, C // heads
        self.nwh, self.nww = H // window, W // window
        self.windows = B * self.nwh * self.nww
        s = self.hd ** -0.5 if scale is None else scale
        self.scale = float(torch.tensor(s, dtype=torch.float32))            # the float32 the descriptor carries

    def args(self):
        return (self.B, self.H, self.W, self.C, self.heads, self.ws, self.shift)


def token_pixels(g):
    """-> int64 [windows, N]: flat pixel number (b H + h) W + w of every token"""
    win = torch.arange(g.windows).view(-1, 1)
    tok = torch.arange(g.N).view(1, -1)
    b = win // (g.nwh * g.nww)
    r = win - b * (g.nwh * g.nww)
    wh, ww = r // g.nww, r % g.nww
    ih, iw = tok // g.ws, tok % g.ws
    h = (wh * g.ws + ih + g.shift) % g.H
    w = (ww * g.ws + iw + g.shift) % g.W
    return (b * g.H + h) * g.W + w


def token_regions(g):
    """-> int64 [windows, N]: mask region of every token (all zero without a shift)"""
    if g.shift == 0:
        return torch.zeros(g.windows, g.N, dtype=torch.int64)
    win = torch.arange(g.windows).view(-1, 1)
    tok = torch.arange(g.N).view(1, -1)
    r = win % (g.nwh * g.nww)
    wh, ww = r // g.nww, r % g.nww
    sh, sw = wh * g.ws + tok // g.ws, ww * g.ws + tok % g.ws

    def band(p, L):
        return (p >= L - g.ws).long() + (p >= L - g.shift).long()
    return band(sh, g.H) * 3 + band(sw, g.W)


def mask_of(g, dtype=F64):
    """-> [windows, 1, N, N]: -100 where the regions of two tokens differ, else 0"""
    reg = token_regions(g)
    return ((reg.unsqueeze(2) != reg.unsqueeze(1)).to(dtype) * -100.0).unsqueeze(1)


def gather(g, t, nparts):
    """t [B, H, W, nparts * C] -> nparts tensors [windows, heads, N, hd] (window tokens through `token_pixels`)"""
    rows = t.reshape(g.B * g.H * g.W, nparts, g.heads, g.hd)[token_pixels(g)]          # [windows, N, nparts, heads, hd]
    return [rows[:, :, i].permute(0, 2, 1, 3) for i in range(nparts)]


def scatter(g, parts, dtype):
    """the inverse of `gather`: parts [windows, heads, N, hd] each -> [B, H, W, len(parts) * C] (every pixel is exactly one token)"""
    rows = torch.stack([p.permute(0, 2, 1, 3) for p in parts], dim=2)                   # [windows, N, nparts, heads, hd]
    out = torch.full((g.B * g.H * g.W, len(parts), g.heads, g.hd), float("nan"), dtype=dtype)
    out[token_pixels(g).reshape(-1)] = rows.reshape(-1, len(parts), g.heads, g.hd)
    return out.reshape(g.B, g.H, g.W, len(parts) * g.C)


def _forward64(g, q, k, v, bias):
    s = g.scale * (q @ k.transpose(-1, -2)) + bias.unsqueeze(0) + mask_of(g)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    p = e / e.sum(-1, keepdim=True)
    return s, mx, p, p @ v


def reference(g, qkv, bias, dout=None):
    """float64 results and units.  -> dict: s, p [windows, heads, N, N]; probs, u_probs [windows, N, N, heads]; out, u_out [B, H, W, C];
    with `dout` also dqkv (float64 autograd through this module's own forward), u_dqkv [B, H, W, 3C]"""
    qkv64, bias64 = qkv.detach().to(F64), bias.detach().to(F64)
    with torch.no_grad():
        q, k, v = gather(g, qkv64, 3)
        s, mx, p, o = _forward64(g, q, k, v, bias64)
        ds = U * (g.scale * (q.abs() @ k.abs().transpose(-1, -2)) + bias64.abs().unsqueeze(0) + s.abs())
        dp = p * (ds + (p * ds).sum(-1, keepdim=True) + 2 * U * (s - mx).abs() + 4 * U)
        r = {"s": s, "p": p, "u_s": ds, "probs": p.permute(0, 2, 3, 1).contiguous(), "u_probs": dp.permute(0, 2, 3, 1).contiguous(),
             "out": scatter(g, [o], F64), "u_out": scatter(g, [(dp + U * p) @ v.abs()], F64)}
    if dout is None:
        return r
    leaf = qkv64.clone().requires_grad_(True)
    q_, k_, v_ = gather(g, leaf, 3)
    out_ = scatter(g, [_forward64(g, q_, k_, v_, bias64)[3]], F64)
    (r["dqkv"],) = torch.autograd.grad(out_, leaf, dout.detach().to(F64))
    with torch.no_grad():
        (dO,) = gather(g, dout.detach().to(F64), 1)
        dP = dO @ v.transpose(-1, -2)
        ddP = U * (dO.abs() @ v.abs().transpose(-1, -2))
        D = (p * dP).sum(-1, keepdim=True)
        dD = (dp * dP.abs() + p * ddP + U * (p * dP).abs()).sum(-1, keepdim=True)
        dS = p * (dP - D)
        ddS = dp * (dP - D).abs() + p * (ddP + dD) + U * p * (dP.abs() + D.abs())
        u_dq = g.scale * (ddS @ k.abs() + U * (dS.abs() @ k.abs())) + U * (g.scale * (dS @ k)).abs()
        u_dk = g.scale * (ddS.transpose(-1, -2) @ q.abs() + 2 * U * (dS.abs().transpose(-1, -2) @ q.abs()))
        u_dv = (dp + U * p).transpose(-1, -2) @ dO.abs()
        r["u_dqkv"] = scatter(g, [u_dq, u_dk, u_dv], F64)
        r["dqkv_analytic"] = scatter(g, [g.scale * (dS @ k), g.scale * (dS.transpose(-1, -2) @ q), p.transpose(-1, -2) @ dO], F64)
    return r


def pv_reference(g, qkv, probs):
    """out from given probabilities [windows, N, N, heads] -> (out, unit) float64 [B, H, W, C]"""
    with torch.no_grad():
        v = gather(g, qkv.detach().to(F64), 3)[2]
        p = probs.detach().to(F64).permute(0, 3, 1, 2)
        return scatter(g, [p @ v], F64), scatter(g, [U * (p.abs() @ v.abs())], F64)


def restate32(g, qkv, bias, dout=None):
    """float32 on the CPU in the kernels' order of operations -> dict: probs, out (and dqkv with `dout`)"""
    f32 = torch.float32
    with torch.no_grad():
        qkv, bias = qkv.detach().to(f32).cpu(), bias.detach().to(f32).cpu()
        q, k, v = gather(g, qkv, 3)
        scale = torch.tensor(g.scale, dtype=f32)
        qs = q * scale
        start = (bias.unsqueeze(0) + mask_of(g, f32)).expand(g.windows, g.heads, g.N, g.N).reshape(-1, g.N, g.N)
        s = torch.baddbmm(start, qs.reshape(-1, g.N, g.hd), k.reshape(-1, g.N, g.hd).transpose(-1, -2)).view(g.windows, g.heads, g.N, g.N)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        p = e * (1.0 / e.sum(-1, keepdim=True))
        r = {"probs": p.permute(0, 2, 3, 1).contiguous(), "out": scatter(g, [p @ v], f32)}
        if dout is not None:
            (dO,) = gather(g, dout.detach().to(f32).cpu(), 1)
            dP = dO @ v.transpose(-1, -2)
            D = (p * dP).sum(-1, keepdim=True)
            dS = p * (dP - D)
            r["dqkv"] = scatter(g, [scale * (dS @ k), dS.transpose(-1, -2) @ qs, p.transpose(-1, -2) @ dO], f32)
    return r


def pv32(g, qkv, probs):
    """float32 restatement of the pv entry: a row's terms added one after the other"""
    f32 = torch.float32
    with torch.no_grad():
        v = gather(g, qkv.detach().to(f32).cpu(), 3)[2]                                 # [windows, heads, N, hd]
        p = probs.detach().to(f32).cpu().permute(0, 3, 1, 2)                            # [windows, heads, N(i), N(j)]
        acc = torch.zeros(g.windows, g.heads, g.N, g.hd, dtype=f32)
        for j in range(g.N):
            acc = acc + p[..., j:j + 1] * v[:, :, j:j + 1, :]
        return scatter(g, [acc], f32)


def worst_ratio(got, ref, unit, floor=0.0):
    """max over ALL elements of |got - ref| / (unit + floor); an element with a zero unit must be exact (0 / 0 counts as 0), a non-finite
    value anywhere gives inf"""
    got = got.detach().cpu().to(F64)
    if not bool(torch.isfinite(got).all()) or not bool(torch.isfinite(ref).all()) or not bool(torch.isfinite(unit).all()):
        return float("inf")
    err = (got - ref).abs()
    den = unit + floor
    ratio = torch.where(err == 0, torch.zeros_like(err), err / den)                     # err > 0 over a zero unit -> inf
    return float(ratio.max())
