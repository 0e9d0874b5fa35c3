"""Float64 reference of the entropy-model kernels (csrc/entropy.hip, K12) on the kernels' own operands: flat NHWC arrays (channel =
index mod C), `params` [C][58] = [33 softplus(matrix) | 13 bias | 12 tanh(factor)] per channel, `medians` [C], and the scale bound as
the float32 value the kernel receives.  Only the rounding z^ = rint(z - med) + med is done in float32 (bit-equal to the kernel);
everything behind it is float64 torch, gradients by float64 autograd of the value functions.

Conventions (include/rdo_ptq_hip.h): the likelihood floor is 1e-9f and carries no gradient (p <= 1e-9f: gradient 0); a scale below
the bound carries no gradient, a scale equal to the bound does; dmeans is 0 at y^ == mu.

Every function also returns a per-element ERROR UNIT: a first-order bound of what float32 evaluation of the same expression may be
off by, formed from reference quantities only.  With u = 2^-24, L = 1 / ln 2:

  Gaussian forward      e_p    = u (P(a) + P(b) + 2 (|a| phi(a) + |b| phi(b))),   a = (.5 - v) / s, b = (-.5 - v) / s, P = Phi
  Gaussian backward     unit_s = |gs| L / (p s) (4 u (|a| phi(a) + |b| phi(b)) (1 + a^2 + b^2) + |a phi(a) - b phi(b)| e_p / p)
                        unit_m = |gs| L / (p s) (4 u (phi(a) + phi(b)) (1 + a^2 + b^2) + |phi(a) - phi(b)| e_p / p)
  factorised forward    e_p    = u (S_hi + S_lo + 8 (S_hi (1 - S_hi) A_hi + S_lo (1 - S_lo) A_lo))
        S = the two sigmoids (of sgn * logit), A = the running magnitude of the logit: the same net with |.| at every product and bias
        (|tanh| <= 1 taken at its value)
  factorised backward   g = -gs L dp / p,  dp = +-(S'_hi D_hi - S'_lo D_lo),  S' = S (1 - S),  D = F'(x) by forward mode
        unit = |gs| L / p ( |dp| e_p / p                                     the unit of p, through 1 / p
                            + u sum_{e in hi, lo} ( 8 S'_e (Dm_e + Q_e)      error of F': its magnitude pass Dm (every layer factor
                                                                             1 + |f| (1 - th^2): no cancellation, softplus(M) > 0 and
                                                                             |tanh f| < 1) and Q, the first-order effect of the
                                                                             pre-activations' error A_v on the factors, 2 |f th| (1 - th^2) A_v,
                                                                             carried through the remaining layers
                                    + 8 |S''_e| A_e D_e                      error of the logit through S'' = S' (1 - 2 S)
                                    + 2 S'_e D_e ) )                         the roundings of S (1 - S) D itself
  sums                  the float64 total and sum |t_i| of its terms (the bounds are derived in tests/test_gpu_entropy.py)
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
INV_LN2 = 1.0 / math.log(2.0)
FLOOR = float(np.float32(1e-9))           # 1e-9f
F64 = torch.float64


def _d(t):
    return torch.as_tensor(t).detach().to(F64)


def _std_cum(x):
    return 0.5 * torch.erfc(-x * (2.0 ** -0.5))


def _phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def round_about(x32, c32):
    """rint(x - c) + c in float32, half to even: the kernels' rounding, bit for bit"""
    assert x32.dtype == torch.float32 and c32.dtype == torch.float32
    return torch.round(x32 - c32) + c32


# ---- factorised prior ----------------------------------------------------------------------------------------------------------------

def eb_logits(params, x, detail=False):
    """F(x) of every channel: x [N, C] float64, params [C, 58] -> logits [N, C].  `detail`: -> (F, A, D, Dm, Q) with A the running
    magnitude, D = dF/dx, Dm its magnitude pass and Q the propagated sensitivity of D to the pre-activations' error (module docstring)."""
    P = _d(params)
    C = P.shape[0]
    assert P.shape == (C, 58) and x.shape[-1] == C
    M, B, Fv = P[:, :33], P[:, 33:46], P[:, 46:58]
    mats = [M[:, 0:3].reshape(C, 3, 1)] + [M[:, 3 + 9 * l:12 + 9 * l].reshape(C, 3, 3) for l in range(3)] + [M[:, 30:33].reshape(C, 1, 3)]
    bias = [B[:, 0:3]] + [B[:, 3 + 3 * l:6 + 3 * l] for l in range(3)] + [B[:, 12:13]]
    fac = [Fv[:, 3 * l:3 * l + 3] for l in range(4)]
    h = x.unsqueeze(-1)                                  # [N, C, 1]
    if detail:
        ah, dh, dmh, qh = h.abs(), torch.ones_like(h), torch.ones_like(h), torch.zeros_like(h)
    for l in range(5):
        v = torch.einsum("coi,nci->nco", mats[l], h) + bias[l]
        if detail:
            av = torch.einsum("coi,nci->nco", mats[l].abs(), ah) + bias[l].abs()
            dv = torch.einsum("coi,nci->nco", mats[l], dh)
            dmv = torch.einsum("coi,nci->nco", mats[l].abs(), dmh)
            qv = torch.einsum("coi,nci->nco", mats[l].abs(), qh)
        if l < 4:
            th = torch.tanh(v)
            h = v + fac[l] * th
            if detail:
                sech2 = 1.0 - th * th
                ah = av + fac[l].abs() * th.abs()
                dh = dv * (1.0 + fac[l] * sech2)
                tm = 1.0 + fac[l].abs() * sech2
                dmh = dmv * tm
                qh = qv * tm + dv.abs() * fac[l].abs() * 2.0 * th.abs() * sech2 * av
        else:
            h = v
            if detail:
                ah, dh, dmh, qh = av, dv, dmv, qv
    if detail:
        return h[..., 0], ah[..., 0], dh[..., 0], dmh[..., 0], qh[..., 0]
    return h[..., 0]


def _eb_p(params, q):
    """raw |sigmoid(s hi) - sigmoid(s lo)| (no floor) of q [N, C] float64, differentiable in q"""
    lo, hi = eb_logits(params, q - 0.5), eb_logits(params, q + 0.5)
    sgn = -torch.sign(lo + hi).detach()
    return (torch.sigmoid(sgn * hi) - torch.sigmoid(sgn * lo)).abs()


def _eb_detail(params, q):
    lo, alo, dlo, dmlo, qlo = eb_logits(params, q - 0.5, detail=True)
    hi, ahi, dhi, dmhi, qhi = eb_logits(params, q + 0.5, detail=True)
    sgn = -torch.sign(lo + hi)
    sh, sl = torch.sigmoid(sgn * hi), torch.sigmoid(sgn * lo)
    e_p = U * (sh + sl + 8.0 * (sh * (1 - sh) * ahi + sl * (1 - sl) * alo))
    return dict(sh=sh, sl=sl, sgn=sgn, p=(sh - sl).abs(), e_p=e_p, ahi=ahi, alo=alo, dhi=dhi, dlo=dlo, dmhi=dmhi, dmlo=dmlo, qhi=qhi, qlo=qlo)


def factorized(z32, params, medians):
    """z32: float32, numel a multiple of C, channel fastest.  -> (zhat float32 in z32's shape, lik float64, unit float64)"""
    C = params.shape[0]
    z = z32.detach().reshape(-1, C)
    zhat = round_about(z, medians.detach().to(torch.float32).reshape(1, C).expand_as(z).contiguous())
    d = _eb_detail(params, zhat.to(F64))
    lik = torch.clamp(d["p"], min=FLOOR)
    return zhat.reshape(z32.shape), lik.reshape(z32.shape), d["e_p"].reshape(z32.shape)


def factorized_value(zhat, params):
    """likelihood (floored, no gradient at or below the floor) of zhat [..., C] float64; differentiable in zhat"""
    C = params.shape[0]
    p = _eb_p(params, zhat.reshape(-1, C))
    return torch.where(p > FLOOR, p, torch.full_like(p, FLOOR)).reshape(zhat.shape)


def factorized_grad(zhat, params, grad_scale=1.0):
    """d(grad_scale * sum -log2 p) / dzhat by float64 autograd.  -> (dz, unit)"""
    C = params.shape[0]
    q = _d(zhat).reshape(-1, C).requires_grad_(True)
    lik = factorized_value(q, params)
    (dz,) = torch.autograd.grad((-torch.log2(lik)).sum() * float(grad_scale), q)
    with torch.no_grad():
        d = _eb_detail(params, q.detach())
        sph, spl = d["sh"] * (1 - d["sh"]), d["sl"] * (1 - d["sl"])
        dp = (sph * d["dhi"] - spl * d["dlo"]).abs()
        p = torch.clamp(d["p"], min=FLOOR)
        per = lambda sp, s, a, dd, dm, qq: 8.0 * sp * (dm + qq) + 8.0 * (sp * (1 - 2 * s)).abs() * a * dd.abs() + 2.0 * sp * dd.abs()
        unit = abs(float(grad_scale)) * INV_LN2 / p * (dp * d["e_p"] / p + U * (per(sph, d["sh"], d["ahi"], d["dhi"], d["dmhi"], d["qhi"])
                                                                                  + per(spl, d["sl"], d["alo"], d["dlo"], d["dmlo"], d["qlo"])))
    return dz.reshape(zhat.shape), unit.reshape(zhat.shape)


# ---- Gaussian conditional ------------------------------------------------------------------------------------------------------------

def _gc_terms(yhat, scales, means, bound):
    mu = torch.zeros_like(yhat) if means is None else means
    s = torch.where(scales >= bound, scales, torch.full_like(scales, bound))        # the gradient passes at sigma == bound
    v = (yhat - mu).abs()                                                           # d|.|/d. = 0 at 0
    return (0.5 - v) / s, (-0.5 - v) / s, s


def gaussian_value(yhat, scales, means, bound):
    """likelihood (floored; no gradient at or below the floor, none to a scale below the bound) in float64; differentiable"""
    a, b, _ = _gc_terms(yhat, scales, means, float(bound))
    p = _std_cum(a) - _std_cum(b)
    return torch.where(p > FLOOR, p, torch.full_like(p, FLOOR))


def _gc_units(a, b, s, p):
    pa, pb = _phi(a), _phi(b)
    e_p = U * (_std_cum(a) + _std_cum(b) + 2.0 * (a.abs() * pa + b.abs() * pb))
    k = 4.0 * U * (1.0 + a * a + b * b)
    unit_s = INV_LN2 / (p * s) * (k * (a.abs() * pa + b.abs() * pb) + (a * pa - b * pb).abs() * e_p / p)
    unit_m = INV_LN2 / (p * s) * (k * (pa + pb) + (pa - pb).abs() * e_p / p)
    return e_p, unit_s, unit_m


def gaussian(y32, scales, means, bound):
    """-> (yhat float32, lik float64, unit float64); means may be None"""
    mu32 = torch.zeros_like(y32) if means is None else means.detach().to(torch.float32)
    yhat = round_about(y32.detach(), mu32)
    with torch.no_grad():
        a, b, s = _gc_terms(yhat.to(F64), _d(scales), mu32.to(F64), float(bound))
        lik = gaussian_value(yhat.to(F64), _d(scales), mu32.to(F64), bound)
        e_p, _, _ = _gc_units(a, b, s, lik)
    return yhat, lik, e_p


def gaussian_grad(yhat, scales, means, bound, grad_scale=1.0):
    """d(grad_scale * sum -log2 p) / d(scales, means) by float64 autograd, y^ constant.  -> (dscales, dmeans, unit_s, unit_m)"""
    yh = _d(yhat)
    sc = _d(scales).requires_grad_(True)
    mu = (torch.zeros_like(yh) if means is None else _d(means)).requires_grad_(True)
    lik = gaussian_value(yh, sc, mu, bound)
    ds, dm = torch.autograd.grad((-torch.log2(lik)).sum() * float(grad_scale), (sc, mu))
    with torch.no_grad():
        a, b, s = _gc_terms(yh, sc, mu, float(bound))
        _, unit_s, unit_m = _gc_units(a, b, s, lik)
    g = abs(float(grad_scale))
    return ds, dm, g * unit_s, g * unit_m


# ---- sums ----------------------------------------------------------------------------------------------------------------------------

def neg_log2_sum(lik, scale=1.0):
    """-> (scale * sum -log2 lik, sum |terms|) in float64"""
    t = -torch.log2(_d(lik)) * float(scale)
    return float(t.sum()), float(t.abs().sum())


def sq_diff_sum(a, b, scale=1.0, clamp01=False):
    """-> (scale * sum (clamp01(a) - b)^2, sum |terms|) in float64"""
    x = _d(a)
    if clamp01:
        x = x.clamp(0.0, 1.0)
    t = (x - _d(b)) ** 2 * float(scale)
    return float(t.sum()), float(t.abs().sum())
