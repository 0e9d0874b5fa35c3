"""CPU anchor of `oracle.entropy_oracle`, the float64 reference that tests/test_gpu_entropy.py holds the kernels of csrc/entropy.hip
against: the reference against mpmath at 50 digits, against the two EntropyBottleneck restatements (which pins the 33 | 13 | 12 packing
of `kernel_params`), its floor / bound conventions on planted elements, and a float32 restatement of every kernel (same expression order
as entropy.hip, libm functions) whose error stays within the reference's per-element units.  The input generators and the restatements
are shared with the GPU tests: a kernel is allowed 4 x the restatement's worst err / unit on the same inputs."""
import math

import numpy as np
import pytest
import torch

from oracle import entropy_oracle as E

F32, F64 = torch.float32, torch.float64
BOUND = float(np.float32(0.11))                 # the scale bound as the kernels receive it
f32 = np.float32


# ---- inputs shared with the GPU tests ------------------------------------------------------------------------------------------------

def make_eb(C, seed):
    """lic.EntropyBottleneck with distinct random values in every entry: pre-softplus matrices ~ N(-1, 0.5), biases wide ~ N(0, 4), factors
    uniform in +-0.8 (tanh'ed by kernel_params), medians ~ 0.7 N(0, 1).  -> (module, params [C, 58], medians [C])"""
    from lic.entropy import EntropyBottleneck
    g = torch.Generator().manual_seed(seed)
    eb = EntropyBottleneck(C).eval()
    with torch.no_grad():
        for n, p in eb.named_parameters():
            if n.startswith("_matrix"):
                p.copy_(-1.0 + 0.5 * torch.randn(p.shape, generator=g))
            elif n.startswith("_bias"):
                p.copy_(4.0 * torch.randn(p.shape, generator=g))
            elif n.startswith("_factor"):
                p.copy_(1.6 * torch.rand(p.shape, generator=g) - 0.8)
            elif n == "quantiles":
                p[:, 0, 1] = 0.7 * torch.randn(C, generator=g)
    return eb, eb.kernel_params().detach().contiguous(), eb.quantiles[:, 0, 1].detach().contiguous()


def factorized_case(C, npix, seed):
    """-> (z [npix, C] ~ 6 N(0, 1), params, medians); planted in channel 0 and C - 1: z = +-60 (rows 0, 1: far tail, on the floor in most
    channels) and z = +-2000 (rows 2, 3: on the floor in every channel, expf of the logit overflows)"""
    _, params, med = make_eb(C, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    z = 6.0 * torch.randn(npix, C, generator=g)
    if npix >= 4:
        z[0, 0], z[1, 0], z[0, C - 1], z[1, C - 1] = 60.0, -60.0, -60.0, 60.0
        z[2, 0], z[3, 0], z[2, C - 1], z[3, C - 1] = 2000.0, -2000.0, -2000.0, 2000.0
    return z.contiguous(), params, med


GC_PLANTED = 40


def gaussian_case(n=200003, seed=11, with_means=True):
    """sigma log-uniform in [0.05, 256], mu ~ N(0, 3), y = mu + 1.5 sigma N(0, 1); the first GC_PLANTED elements are planted (their mu on a
    grid of 1/8 so that y - mu is exact).  -> (y, scales, means or None, names of the planted elements)"""
    g = torch.Generator().manual_seed(seed)
    scales = torch.exp(torch.empty(n).uniform_(math.log(0.05), math.log(256.0), generator=g))
    means = 3.0 * torch.randn(n, generator=g)
    y = means + 1.5 * scales * torch.randn(n, generator=g)
    b = f32(BOUND)
    plant = []
    for s in (0.0, -1.0, float(np.nextafter(b, f32(0))), float(b), float(np.nextafter(b, f32(1)))):       # around the scale bound, off centre
        plant.append((f"sigma={s!r}", 1.0, s, 0.375))
    for d in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5):                                                              # half-to-even ties
        plant.append((f"tie{d:+}", d, 1.7, -2.125))
    for s in (0.05, BOUND, 0.7, 40.0, 256.0):                                                                # y^ == mu
        plant.append((f"centre s={s}", 0.0, s, 1.25))
    for v, s in ((11.0, 2.0), (-11.0, 2.0), (1.0, 1 / 5.5), (13.0, 2.0), (1.0, 1 / 6.5), (-13.0, 2.0), (12.0, 1.0), (-24.0, 2.0), (6.0, 0.5)):
        plant.append((f"tail v={v} s={s:.4f}", v, s, 0.625))                                                 # |y^ - mu| / sigma = 5.5, 6.5, 12
    assert len(plant) <= GC_PLANTED
    for k, (_, d, s, m) in enumerate(plant):
        means[k], scales[k], y[k] = m, s, m + d
    if not with_means:
        y = y - means
        means = None
    return y.contiguous(), scales.contiguous(), means, [p[0] for p in plant]


# ---- float32 restatements of the kernels (expression order of csrc/entropy.hip) --------------------------------------------------------

def _sigm32(x):
    return 1.0 / (1.0 + torch.exp(-x))


def eb_logits32(P, x, deriv=False):
    """eb_logits / eb_logits_d: P [C, 58] float32, x [N, C] float32"""
    M, Bv, Fv = [P[:, k] for k in range(33)], [P[:, 33 + k] for k in range(13)], [P[:, 46 + k] for k in range(12)]
    h, dh = [], []
    for o in range(3):
        v = M[o] * x + Bv[o]
        th = torch.tanh(v)
        h.append(v + Fv[o] * th)
        dh.append(M[o] * (1.0 + Fv[o] * (1.0 - th * th)))
    for l in range(3):
        g, dg = [], []
        for o in range(3):
            v, dv = Bv[3 + 3 * l + o].expand_as(x), torch.zeros_like(x)
            for i in range(3):
                v = v + M[3 + 9 * l + 3 * o + i] * h[i]
                dv = dv + M[3 + 9 * l + 3 * o + i] * dh[i]
            th = torch.tanh(v)
            g.append(v + Fv[3 + 3 * l + o] * th)
            dg.append(dv * (1.0 + Fv[3 + 3 * l + o] * (1.0 - th * th)))
        h, dh = g, dg
    v, dv = Bv[12].expand_as(x), torch.zeros_like(x)
    for i in range(3):
        v = v + M[30 + i] * h[i]
        dv = dv + M[30 + i] * dh[i]
    return (v, dv) if deriv else v


def eb_fwd32(z, params, med):
    C = params.shape[0]
    zz = z.reshape(-1, C)
    q = torch.round(zz - med) + med
    lo, hi = eb_logits32(params, q - 0.5), eb_logits32(params, q + 0.5)
    sgn = -torch.sign(lo + hi)
    lik = torch.clamp((_sigm32(sgn * hi) - _sigm32(sgn * lo)).abs(), min=1e-9)
    return q.reshape(z.shape), lik.reshape(z.shape)


def eb_bwd32(zhat, params, gscale):
    C = params.shape[0]
    q = zhat.reshape(-1, C)
    lo, dlo = eb_logits32(params, q - 0.5, True)
    hi, dhi = eb_logits32(params, q + 0.5, True)
    sgn = -torch.sign(lo + hi)
    sh, sl = _sigm32(sgn * hi), _sigm32(sgn * lo)
    diff = sh - sl
    pr = diff.abs()
    dp = torch.where(diff > 0, 1.0, -1.0) * sgn * (sh * (1.0 - sh) * dhi - sl * (1.0 - sl) * dlo)
    coef = float(f32(-gscale) * f32(1.4426950408889634))
    g = coef / pr * dp
    return torch.where(pr > 1e-9, g, torch.zeros_like(g)).reshape(zhat.shape)


def _std_cum32(x):
    return 0.5 * torch.erfc(-0.70710678118654752440 * x)


def gc_fwd32(y, scales, means, bound):
    mu = torch.zeros_like(y) if means is None else means
    q = torch.round(y - mu) + mu
    v = (q - mu).abs()
    s = torch.clamp(scales, min=bound)
    return q, torch.clamp(_std_cum32((0.5 - v) / s) - _std_cum32((-0.5 - v) / s), min=1e-9)


def gc_bwd32(yhat, scales, means, bound, gscale):
    mu = torch.zeros_like(yhat) if means is None else means
    d = yhat - mu
    v = d.abs()
    s = torch.clamp(scales, min=bound)
    a, b = (0.5 - v) / s, (-0.5 - v) / s
    p = _std_cum32(a) - _std_cum32(b)
    pa, pb = 0.3989422804014327 * torch.exp(-0.5 * a * a), 0.3989422804014327 * torch.exp(-0.5 * b * b)
    coef = float(f32(-gscale) * f32(1.4426950408889634)) / p
    ds = coef * (-(pa * a - pb * b) / s)
    dm = coef * (-(pa - pb) / s) * (-torch.sign(d))
    live = p > 1e-9
    return torch.where(live & (scales >= bound), ds, torch.zeros_like(ds)), torch.where(live, dm, torch.zeros_like(dm))


def sum_grid(n):
    return min(-(-n // 256), 2048)


def _tree32(v):
    """block_sum of [..., 256] float32: per wave the shuffle steps 32 .. 1, then ((w0 + w1) + w2) + w3"""
    w = v.reshape(v.shape[:-1] + (4, 64))
    for o in (32, 16, 8, 4, 2, 1):
        w = w[..., :o] + w[..., o:2 * o]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def ordered_sum32(terms, scale, out0=0.0):
    """The ordered sums' order on float32 `terms` (numpy): per-thread chain over the grid-stride laps, block tree, * scale, fold chain, fold tree, +="""
    n = terms.size
    g = sum_grid(n)
    laps = -(-n // (256 * g))
    t = np.zeros(laps * 256 * g, f32)
    t[:n] = terms
    acc = np.zeros(256 * g, f32)
    for row in t.reshape(laps, 256 * g):
        acc = acc + row
    part = _tree32(acc.reshape(g, 256)) * f32(scale)
    p = np.zeros(256 * (-(-g // 256)), f32)
    p[:g] = part
    acc = np.zeros(256, f32)
    for row in p.reshape(-1, 256):
        acc = acc + row
    return f32(out0) + _tree32(acc)


def ratio(got, ref, unit, keep=None):
    """worst |got - ref| / unit over the kept elements"""
    err = (got.to(F64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / unit)         # an exact element needs no unit (on the floor the unit may be 0)
    if keep is not None:
        r = r[keep]
    return float(r.max()) if r.numel() else 0.0


def near_floor(p_ref):
    """elements whose float64 p lies within 1e-3 relative of the floor: the two precisions may land on different sides"""
    return (p_ref - E.FLOOR).abs() <= 1e-3 * E.FLOOR


def gc_raw_p(yhat, scales, means, bound=BOUND):
    """unfloored float64 p of the Gaussian conditional (to decide which elements the floor rule excludes)"""
    a, b, _ = E._gc_terms(yhat.to(F64), scales.to(F64), None if means is None else means.to(F64), bound)
    return E._std_cum(a) - E._std_cum(b)


def eb_raw_p(zhat, params):
    return E._eb_p(params, zhat.to(F64).reshape(-1, params.shape[0])).reshape(zhat.shape)


# ---- the reference against mpmath ----------------------------------------------------------------------------------------------------

def test_gaussian_reference_matches_mpmath():
    import mpmath as mp
    mp.mp.dps = 50
    pts = [(0.0, 0.05), (0.0, 0.11), (0.0, 2.3), (0.0, 256.0), (1.0, 0.11), (1.0, 0.3), (2.0, 0.5), (3.0, 1.0), (7.0, 2.3), (11.0, 2.0),
           (13.0, 2.5), (-5.0, 1.0), (6.0, 1.1), (40.0, 40.0), (120.0, 40.0), (200.0, 40.0), (256.0, 256.0), (700.0, 256.0), (1100.0, 256.0),
           (1240.0, 256.0), (1.0, 0.19), (5.0, 0.9), (28.0, 5.0), (-57.0, 10.0), (1.0, 256.0), (3.0, 100.0), (17.0, 3.0), (560.0, 100.0)]
    mu = 0.625
    y = torch.tensor([mu + v for v, _ in pts], dtype=F32)
    s = torch.tensor([sg for _, sg in pts], dtype=F32)
    m = torch.full_like(y, mu)
    yhat, lik, unit = E.gaussian(y, s, m, BOUND)
    assert torch.equal(yhat, y)
    tails = 0
    for k, (v, _) in enumerate(pts):
        sg = mp.mpf(max(float(s[k]), BOUND))
        P = lambda t: mp.erfc(-t / mp.sqrt(2)) / 2
        want = P((mp.mpf(0.5) - abs(v)) / sg) - P((mp.mpf(-0.5) - abs(v)) / sg)
        want = max(want, mp.mpf(E.FLOOR))
        assert abs(mp.mpf(float(lik[k])) - want) <= 1e-5 * float(unit[k]), (pts[k], float(lik[k]), want)
        tails += 1e-9 < want < 1e-7
    assert tails >= 4


def test_factorized_reference_matches_mpmath():
    import mpmath as mp
    mp.mp.dps = 50
    C = 3
    _, params, med = make_eb(C, 5)
    zs = [-80.0, -60.0, -40.0, -25.0, -18.0, -12.0, -7.0, -3.0, -1.0, 0.0, 1.0, 2.0, 5.0, 9.0, 14.0, 19.0, 26.0, 40.0, 60.0, 80.0]
    z = torch.tensor(zs, dtype=F32).reshape(-1, 1).repeat(1, C).contiguous()
    zhat, lik, unit = E.factorized(z, params, med)
    P = [[mp.mpf(float(v)) for v in row] for row in params]

    def net(p, x):
        M, B, Fv = p[:33], p[33:46], p[46:]
        h = [M[o] * x + B[o] for o in range(3)]
        h = [h[o] + Fv[o] * mp.tanh(h[o]) for o in range(3)]
        for l in range(3):
            v = [B[3 + 3 * l + o] + sum(M[3 + 9 * l + 3 * o + i] * h[i] for i in range(3)) for o in range(3)]
            h = [v[o] + Fv[3 + 3 * l + o] * mp.tanh(v[o]) for o in range(3)]
        return B[12] + sum(M[30 + i] * h[i] for i in range(3))

    sig = lambda t: 1 / (1 + mp.exp(-t))
    small = 0
    for n in range(len(zs)):
        for c in range(C):
            q = mp.mpf(float(zhat[n, c]))
            lo, hi = net(P[c], q - mp.mpf(0.5)), net(P[c], q + mp.mpf(0.5))
            sg = -mp.sign(lo + hi)
            want = max(abs(sig(sg * hi) - sig(sg * lo)), mp.mpf(E.FLOOR))
            assert abs(mp.mpf(float(lik[n, c])) - want) <= 1e-5 * float(unit[n, c]), (zs[n], c, float(lik[n, c]), want)
            small += E.FLOOR < want < 1e-6
    assert small >= 4


# ---- the packing of kernel_params ------------------------------------------------------------------------------------------------------

def test_kernel_params_packing_matches_both_entropy_bottlenecks():
    import copy
    from oracle import lic_oracle
    C = 5
    eb, params, med = make_eb(C, 21)
    vals = torch.cat([p.detach().reshape(-1) for n, p in eb.named_parameters() if n != "quantiles"])
    assert vals.unique().numel() == vals.numel() == C * 58
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():
        eb.quantiles[:, 0, 1] = torch.round(eb.quantiles[:, 0, 1] * 64) / 64        # medians and z on a grid of 1/64: the float32 rounding
    med = eb.quantiles[:, 0, 1].detach().contiguous()                               # is then exact, and equal to the modules' float64 one
    z = torch.round(6.0 * torch.randn(2, C, 4, 3, generator=g) * 64) / 64
    params64 = copy.deepcopy(eb).double().kernel_params().detach()           # softplus / tanh of the packing in float64, as the modules do
    zhat, lik, _ = E.factorized(z.permute(0, 2, 3, 1).contiguous(), params64, med)
    ref = lic_oracle.EntropyBottleneck(C).eval()
    ref.load_state_dict(eb.state_dict())
    with torch.no_grad():
        for module in (ref.double(), copy.deepcopy(eb).double()):
            zr, lr = module(z.double())
            assert torch.equal(zr, zhat.permute(0, 3, 1, 2).double())
            torch.testing.assert_close(lr, lik.permute(0, 3, 1, 2), rtol=1e-11, atol=0)
    # the float32 packing carries the same values
    _, lik32, unit = E.factorized(z.permute(0, 2, 3, 1).contiguous(), params, med)
    assert float(((lik32 - lik).abs() / unit).max()) < 16


# ---- the conventions on planted elements -----------------------------------------------------------------------------------------------

def test_gaussian_conventions_on_planted_elements():
    y, scales, means, names = gaussian_case(n=GC_PLANTED + 5)
    yhat, lik, unit = E.gaussian(y, scales, means, BOUND)
    ds, dm, us, um = E.gaussian_grad(yhat, scales, means, BOUND, 1.0)
    at = {n: k for k, n in enumerate(names)}
    b = f32(BOUND)
    below, on, above = at[f"sigma={float(np.nextafter(b, f32(0)))!r}"], at[f"sigma={float(b)!r}"], at[f"sigma={float(np.nextafter(b, f32(1)))!r}"]
    for k in (at["sigma=0.0"], at["sigma=-1.0"], below):
        assert float(ds[k]) == 0.0 and float(dm[k]) != 0.0 and float(lik[k]) == float(lik[on])
    assert float(ds[on]) != 0.0 and abs(float(ds[on]) - float(ds[above])) < 1e-5 * abs(float(ds[on]))
    want = {0.5: 0.0, -0.5: -0.0, 1.5: 2.0, -1.5: -2.0, 2.5: 2.0, -2.5: -2.0}                               # half to even
    for d, r in want.items():
        assert float(yhat[at[f"tie{d:+}"]]) == -2.125 + r
    for n, k in at.items():
        if n.startswith("centre"):
            assert float(yhat[k]) == float(means[k]) and float(dm[k]) == 0.0
            assert float(ds[k]) > 0.0 if float(scales[k]) >= BOUND else float(ds[k]) == 0.0        # a wider sigma lowers the central mass
    floor = [at["tail v=12.0 s=1.0000"], at["tail v=-24.0 s=2.0000"], at["tail v=6.0 s=0.5000"]]
    for k in floor:
        assert float(lik[k]) == E.FLOOR and float(ds[k]) == 0.0 and float(dm[k]) == 0.0
    k = at["tail v=11.0 s=2.0000"]
    assert float(lik[k]) > E.FLOOR and float(ds[k]) != 0.0 and float(dm[k]) != 0.0
    # closed form of the header against autograd: d(-log2 p)/ds = (phi(a) a - phi(b) b) / (s p ln 2), d/dmu = -sign(y^ - mu) (phi(a) - phi(b)) / (s p ln 2)
    live = [k for k in range(len(names)) if k not in floor and float(lik[k]) > E.FLOOR and float(scales[k]) >= BOUND]
    a, bb, s = E._gc_terms(yhat.double(), scales.double(), means.double(), BOUND)
    cs = (E._phi(a) * a - E._phi(bb) * bb) / (s * lik) * E.INV_LN2
    cm = -torch.sign(yhat.double() - means.double()) * (E._phi(a) - E._phi(bb)) / (s * lik) * E.INV_LN2
    torch.testing.assert_close(ds[live], cs[live], rtol=1e-10, atol=0)
    torch.testing.assert_close(dm[live], cm[live], rtol=1e-10, atol=1e-300)
    # grad_scale is linear
    ds2, dm2, us2, _ = E.gaussian_grad(yhat, scales, means, BOUND, 0.37)
    torch.testing.assert_close(ds2, 0.37 * ds, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(us2, 0.37 * us, rtol=1e-14, atol=0)


def test_factorized_conventions_on_planted_elements():
    z, params, med = factorized_case(3, 50, 31)
    zhat, lik, unit = E.factorized(z, params, med)
    dz, udz = E.factorized_grad(zhat, params, 1.0)
    for r, c in ((2, 0), (3, 0), (2, 2), (3, 2)):                  # z = +-2000: on the floor
        assert float(lik[r, c]) == E.FLOOR and float(dz[r, c]) == 0.0
    live = lik > E.FLOOR
    assert int(live.sum()) >= 100 and bool((dz[live] != 0).all())
    assert torch.equal(zhat, torch.round(z - med) + med)
    # central finite difference of the value function (h = 1e-6 in float64) agrees with autograd
    q = zhat.double()
    h = 1e-6
    fd = (-torch.log2(E.factorized_value(q + h, params)) + torch.log2(E.factorized_value(q - h, params))) / (2 * h)
    torch.testing.assert_close(dz[live], fd[live], rtol=1e-5, atol=1e-7)
    dz2, _ = E.factorized_grad(zhat, params, 0.37)
    torch.testing.assert_close(dz2, 0.37 * dz, rtol=1e-14, atol=0)


# ---- the float32 restatements stay within the units ------------------------------------------------------------------------------------

def gaussian_restatement_ratios(y, scales, means, gscale=1.0):
    """-> dict of the float32 restatement's worst err / unit: 'fwd', 'ds', 'dm' (and the excluded count)"""
    yhat, lik, unit = E.gaussian(y, scales, means, BOUND)
    keep = ~near_floor(gc_raw_p(yhat, scales, means))
    q32, l32 = gc_fwd32(y, scales, means, BOUND)
    assert torch.equal(q32, yhat)
    ds, dm, us, um = E.gaussian_grad(yhat, scales, means, BOUND, gscale)
    ds32, dm32 = gc_bwd32(yhat, scales, means, BOUND, gscale)
    return {"fwd": ratio(l32, lik, unit, keep), "ds": ratio(ds32, ds, us, keep), "dm": ratio(dm32, dm, um, keep), "excluded": int((~keep).sum())}


def factorized_restatement_ratios(z, params, med, gscale=1.0):
    zhat, lik, unit = E.factorized(z, params, med)
    keep = ~near_floor(eb_raw_p(zhat, params))
    q32, l32 = eb_fwd32(z, params, med)
    assert torch.equal(q32, zhat)
    dz, udz = E.factorized_grad(zhat, params, gscale)
    return {"fwd": ratio(l32, lik, unit, keep), "dz": ratio(eb_bwd32(zhat, params, gscale), dz, udz, keep), "excluded": int((~keep).sum())}


# What the restatements may reach.  The units are first-order bounds of the roundings of +, *, / alone; libm's erfcf, expf and tanhf add up
# to 1 ulp each on top (erfcf twice in p: <= 2 units of p at |a| ~ |b|), which the forward unit of the Gaussian does not count -- hence 2
# there; everywhere else the restatement stays within one unit.
RESTATEMENT_LIMIT = {"gc fwd": 2.0, "gc ds": 1.0, "gc dm": 1.0, "eb fwd": 1.0, "eb dz": 1.0}


@pytest.mark.parametrize("with_means", [True, False])
def test_gaussian_restatement_within_units(with_means):
    y, scales, means, _ = gaussian_case(with_means=with_means)
    r = gaussian_restatement_ratios(y, scales, means, 0.37)
    print(f"gaussian restatement (means={with_means}): worst err/unit fwd {r['fwd']:.3f} dscales {r['ds']:.3f} dmeans {r['dm']:.3f} "
          f"excluded {r['excluded']}")
    assert r["excluded"] == 0
    assert r["fwd"] <= RESTATEMENT_LIMIT["gc fwd"] and r["ds"] <= RESTATEMENT_LIMIT["gc ds"] and r["dm"] <= RESTATEMENT_LIMIT["gc dm"]


@pytest.mark.parametrize("C,npix", [(1, 4099), (3, 2731), (24, 683), (192, 171), (7, 75011)])
def test_factorized_restatement_within_units(C, npix):
    z, params, med = factorized_case(C, npix, 40 + C)
    zhat, lik, _ = E.factorized(z, params, med)
    r = factorized_restatement_ratios(z, params, med, 0.37)
    live = lik[lik > E.FLOOR]
    print(f"factorised restatement C={C} n={z.numel()}: worst err/unit fwd {r['fwd']:.3f} dz {r['dz']:.3f} excluded {r['excluded']} "
          f"min live p {float(live.min()):.2e} on floor {int((lik == E.FLOOR).sum())}")
    assert r["excluded"] <= 0.005 * z.numel()
    assert r["fwd"] <= RESTATEMENT_LIMIT["eb fwd"] and r["dz"] <= RESTATEMENT_LIMIT["eb dz"]


SUM_SIZES = [1, 255, 256, 257, 65539, 524288, 524289, 3 * 524288 + 77]


def ordered_bound(n, abs_total):
    """(k1 + 31) u sum |t_i|: per-thread chain of k1 = ceil(n / (256 g)) terms, block tree (9), fold chain of ceil(g / 256) <= 8, fold tree
    (9), the +=, 4 for log2f / the square and the scale"""
    k1 = -(-n // (256 * sum_grid(n)))
    return (k1 + 31) * E.U * abs_total


def atomic_bound(n, abs_total):
    """worst case of the atomic forms: the g block sums arrive in any order, (k1 + g + 14) u sum |t_i|"""
    g = sum_grid(n)
    k1 = -(-n // (256 * g))
    return (k1 + g + 14) * E.U * abs_total


def sum_case(n, seed=7):
    g = torch.Generator().manual_seed(seed + n % 1000)
    lik = torch.exp(-torch.rand(n, generator=g) * 12.0).clamp_min(1e-9)
    a = torch.rand(n, generator=g) * 1.6 - 0.3
    b = torch.rand(n, generator=g)
    return lik, a, b


@pytest.mark.parametrize("n", SUM_SIZES)
def test_ordered_sum_restatement_within_the_derived_bound(n):
    lik, a, b = sum_case(n)
    want, tot = E.neg_log2_sum(lik, 0.25)
    got = float(ordered_sum32((-torch.log2(lik)).numpy(), 0.25, 1.5))
    assert abs(got - (want + 1.5)) <= ordered_bound(n, tot + 1.5), (n, got, want)
    for clamp in (False, True):
        want, tot = E.sq_diff_sum(a, b, 3.0, clamp)
        x = a.clamp(0, 1) if clamp else a
        got = float(ordered_sum32(((x - b) * (x - b)).numpy(), 3.0, 0.0))
        assert abs(got - want) <= ordered_bound(n, tot), (n, clamp, got, want)
    # an exact case: integer terms, any order gives the same bits
    i = torch.arange(n)
    exact = (1 + i % 7).to(F32).numpy()
    assert float(ordered_sum32(exact, 0.5, 3.0)) == 3.0 + 0.5 * float((1 + i % 7).sum())
