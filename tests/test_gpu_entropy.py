"""Float64 parity of csrc/entropy.hip (K12) at the scales models use: every likelihood, gradient and sum against
`oracle.entropy_oracle`, per element, with |got - ref| <= c * unit_i.  The units are the reference's own first-order float32 bounds;
c = 4 x the worst err / unit of the float32 CPU restatement (tests/test_entropy_reference.py) on the SAME inputs -- device erfcf / expf /
tanhf are few-ulp routines where libm's are <= 1 ulp, and the compiler may contract multiplies and adds.  Elements on the 1e-9f floor are
compared exactly; an element is left out only when its float64 p lies within 1e-3 relative of the floor (at most 0.5 % of a case).
Measured ratios: DESIGN.md, "Entropy kernels: float64 parity"."""
import functools
import math

import numpy as np
import pytest
import torch

import test_entropy_reference as R
from oracle import entropy_oracle as E

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
FLOOR32 = float(np.float32(1e-9))
BOUND = R.BOUND
U = E.U


def _compare(what, got, ref, unit, c, p_raw):
    """per-element |got - ref| <= c unit off the floor; on the floor (float64 p below it) the exact floor value: `ref` there"""
    got = got.detach().cpu().reshape(ref.shape)
    near = R.near_floor(p_raw)
    assert int(near.sum()) <= 0.005 * ref.numel(), (what, int(near.sum()))
    on_floor = (p_raw < E.FLOOR) & ~near
    assert torch.equal(got[on_floor].to(F64), ref[on_floor]), (what, "floor elements differ")
    r = R.ratio(got, ref, unit, ~near)
    print(f"[entropy parity] {what}: kernel worst err/unit {r:.3f}, allowed {c:.3f} (= 4 x restatement {c / 4:.3f}); "
          f"on floor {int(on_floor.sum())}, left out {int(near.sum())} of {ref.numel()}")
    assert r <= c, (what, r, c)


# ---- Gaussian conditional ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gaussian_ref(with_means):
    y, s, m, names = R.gaussian_case(with_means=with_means)
    yhat, lik, unit = E.gaussian(y, s, m, BOUND)
    ds, dm, us, um = E.gaussian_grad(yhat, s, m, BOUND, 0.37)
    return dict(y=y, s=s, m=m, names=names, yhat=yhat, lik=lik, unit=unit, ds=ds, dm=dm, us=us, um=um, p_raw=R.gc_raw_p(yhat, s, m),
                rest=R.gaussian_restatement_ratios(y, s, m, 0.37))


@pytest.mark.parametrize("with_means", [True, False])
def test_gaussian_forward_and_backward_match_float64(with_means):
    from hipops import _lib as L
    from hipops import ops
    d = _gaussian_ref(with_means)
    n = d["y"].numel()
    assert n == 200003
    y, s, m = d["y"].cuda(), d["s"].cuda(), None if d["m"] is None else d["m"].cuda()
    yhat, lik = ops.gaussian_likelihood(y, s, m, BOUND)
    assert torch.equal(yhat.cpu(), d["yhat"])                                       # half to even, bit-equal
    tag = f"gaussian means={with_means}"
    _compare(f"{tag} fwd", lik, d["lik"], d["unit"], 4 * d["rest"]["fwd"], d["p_raw"])
    # yhat = NULL: the same likelihoods
    lik2 = torch.full_like(lik, float("nan"))
    L.check(L.lib().rdo_gaussian_likelihood_fwd(ops._ptr(y), ops._ptr(s), ops._ptr(m), n, BOUND, None, ops._ptr(lik2), ops._stream()))
    assert torch.equal(lik2, lik)
    ds, dm = ops.gaussian_likelihood_bwd(yhat, s, m, 0.37, BOUND)
    _compare(f"{tag} dscales", ds, d["ds"], d["us"], 4 * d["rest"]["ds"], d["p_raw"])
    _compare(f"{tag} dmeans", dm, d["dm"], d["um"], 4 * d["rest"]["dm"], d["p_raw"])
    # one output only: the same bits
    for which in (0, 1):
        one = torch.full_like(ds, float("nan"))
        L.check(L.lib().rdo_gaussian_likelihood_bwd(ops._ptr(yhat), ops._ptr(s), ops._ptr(m), n, BOUND, 0.37, ops._ptr(one) if which == 0 else None,
                                                    ops._ptr(one) if which == 1 else None, ops._stream()))
        assert torch.equal(one, (ds, dm)[which])
    # grad_scale is linear: -gs / ln2 is rounded once more than 1 / ln2, then the same two operations; float32(0.37) is 0.37 within u / 2
    ds1, dm1 = ops.gaussian_likelihood_bwd(yhat, s, m, 1.0, BOUND)
    for a, b in ((ds, ds1), (dm, dm1)):
        assert torch.equal(a == 0, b == 0)
        assert bool(((a.double() - 0.37 * b.double()).abs() <= 8 * U * (0.37 * b.double()).abs()).all())
    # the planted elements, on the kernel's own output
    at = {k: i for i, k in enumerate(d["names"])}
    lik_c, ds_c, dm_c = lik.cpu(), ds.cpu(), dm.cpu()
    b32 = np.float32(BOUND)
    on = at[f"sigma={float(b32)!r}"]
    for k in (at["sigma=0.0"], at["sigma=-1.0"], at[f"sigma={float(np.nextafter(b32, np.float32(0)))!r}"]):
        assert float(ds_c[k]) == 0.0 and float(dm_c[k]) != 0.0 and float(lik_c[k]) == float(lik_c[on])
    assert float(ds_c[on]) != 0.0 and float(ds_c[at[f"sigma={float(np.nextafter(b32, np.float32(1)))!r}"]]) != 0.0
    for name, k in at.items():
        if name.startswith("centre"):
            assert float(dm_c[k]) == 0.0 and float(yhat[k]) == (float(d["m"][k]) if with_means else 0.0)
    for name in ("tail v=12.0 s=1.0000", "tail v=-24.0 s=2.0000", "tail v=6.0 s=0.5000"):
        k = at[name]
        assert float(lik_c[k]) == FLOOR32 and float(ds_c[k]) == 0.0 and float(dm_c[k]) == 0.0
    k = at["tail v=11.0 s=2.0000"]
    assert float(lik_c[k]) > FLOOR32 and float(ds_c[k]) != 0.0 and float(dm_c[k]) != 0.0


def test_gaussian_bin_masses_sum_to_one():
    """sum_k of the bin masses over k = -K..K, K = 6 sigma, is 1 - 2 Phi(-(K + .5) / sigma): no reference needed for the value; the
    tolerance is the sum of the allowed per-element errors"""
    from hipops import ops
    d = _gaussian_ref(True)
    c = 4 * d["rest"]["fwd"]
    for sigma in (BOUND, 0.5, 2.3, 40.0, 256.0):
        K = math.ceil(6 * sigma)
        k = torch.arange(-K, K + 1, dtype=F32)
        mu = torch.full_like(k, 0.25)
        s = torch.full_like(k, sigma)
        yhat, lik = ops.gaussian_likelihood((k + mu).cuda(), s.cuda(), mu.cuda(), BOUND)
        assert torch.equal(yhat.cpu(), k + mu)
        _, ref, unit = E.gaussian(k + mu, s, mu, BOUND)
        tails = 2 * 0.5 * math.erfc((K + 0.5) / max(sigma, BOUND) / math.sqrt(2))
        floors = int((lik.cpu() == FLOOR32).sum())
        total = float(lik.double().sum())
        tol = c * float(unit.sum()) + floors * 1e-9
        print(f"[entropy parity] gaussian telescoping sigma={sigma}: |sum - (1 - tails)| = {abs(total - (1 - tails)):.3e}, allowed {tol:.3e}")
        assert abs(total - (1 - tails)) <= tol, (sigma, total, tails, tol)


# ---- factorised prior ----------------------------------------------------------------------------------------------------------------

FACTORIZED_CASES = [(1, 4099), (3, 2731), (24, 683), (192, 171), (7, 75011)]     # the last: 525 077 elements > 2048 * 256, 7 coprime to the stride


@functools.lru_cache(maxsize=None)
def _factorized_ref(C, npix):
    z, params, med = R.factorized_case(C, npix, 40 + C)
    zhat, lik, unit = E.factorized(z, params, med)
    dz, udz = E.factorized_grad(zhat, params, 0.37)
    return dict(z=z, params=params, med=med, zhat=zhat, lik=lik, unit=unit, dz=dz, udz=udz, p_raw=R.eb_raw_p(zhat, params),
                rest=R.factorized_restatement_ratios(z, params, med, 0.37))


@pytest.mark.parametrize("C,npix", FACTORIZED_CASES)
def test_factorized_forward_and_backward_match_float64(C, npix):
    from hipops import ops
    d = _factorized_ref(C, npix)
    if (C, npix) == (7, 75011):
        assert d["z"].numel() == 525077 > 2048 * 256
    assert int((d["p_raw"] < E.FLOOR).sum()) >= 2                                   # the planted z = +-2000
    params, med = d["params"].cuda(), d["med"].cuda()
    zhat, lik = ops.factorized_likelihood(d["z"].cuda(), params, med)
    assert torch.equal(zhat.cpu(), d["zhat"])
    tag = f"factorised C={C} n={d['z'].numel()}"
    _compare(f"{tag} fwd", lik, d["lik"], d["unit"], 4 * d["rest"]["fwd"], d["p_raw"])
    dz = ops.factorized_likelihood_bwd(zhat, params, 0.37)
    _compare(f"{tag} dz", dz, d["dz"], d["udz"], 4 * d["rest"]["dz"], d["p_raw"])
    dz1 = ops.factorized_likelihood_bwd(zhat, params, 1.0)
    assert torch.equal(dz == 0, dz1 == 0)
    assert bool(((dz.double() - 0.37 * dz1.double()).abs() <= 8 * U * (0.37 * dz1.double()).abs()).all())


def test_factorized_likelihoods_telescope():
    """sum_k lik(k + med), k = -K..K, equals sigmoid(F(K + .5 + med)) - sigmoid(F(-K - .5 + med)) per channel (medians on a grid of 1/64:
    the bin edges then meet exactly); evaluated in float64, tolerance = the sum of the allowed per-element errors"""
    from hipops import ops
    C, K = 24, 48
    _, params, med = R.make_eb(C, 77)
    med = torch.round(med * 64) / 64
    k = torch.arange(-K, K + 1, dtype=F32).reshape(-1, 1)
    z = (k + med).contiguous()
    zhat, lik = ops.factorized_likelihood(z.cuda(), params.cuda(), med.cuda())
    assert torch.equal(zhat.cpu(), z)
    _, ref, unit = E.factorized(z, params, med)
    c = 4 * R.factorized_restatement_ratios(z, params, med)["fwd"]
    top = E.eb_logits(params, (med.double() + K + 0.5).reshape(1, C))[0]
    bot = E.eb_logits(params, (med.double() - K - 0.5).reshape(1, C))[0]
    want = torch.sigmoid(top) - torch.sigmoid(bot)
    got = lik.double().sum(0).cpu()
    floors = (lik.cpu() == FLOOR32).sum(0)
    tol = c * unit.sum(0) + floors * 1e-9
    print(f"[entropy parity] factorised telescoping: worst |sum - want| / allowed {float(((got - want).abs() / tol).max()):.3f}, "
          f"masses {float(want.min()):.4f} .. {float(want.max()):.4f}")
    assert bool(((got - want).abs() <= tol).all()), ((got - want).abs() / tol)


# ---- rate / distortion sums ------------------------------------------------------------------------------------------------------------

def _forms():
    from hipops import ops
    return {"atomic": (ops.neg_log2_sum, ops.sq_diff_sum), "ordered": (ops.neg_log2_sum_ordered, ops.sq_diff_sum_ordered)}


def _out(v):
    return torch.full((1,), v, device="cuda", dtype=F32)


@pytest.mark.parametrize("n", R.SUM_SIZES)
def test_sums_exact_cases_are_bit_equal(n):
    """terms whose every partial sum is exact in float32: any summation order gives the same bits, a dropped or doubled element shows"""
    i = torch.arange(n)
    lik = torch.pow(2.0, -(1 + i % 7).to(F32)).cuda()
    want_log = 3.0 + 0.5 * float((1 + i % 7).sum())
    dd = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[i % 7]
    b = (i % 3).to(F32) * 0.25
    a = (b + dd).cuda()
    want_sq = 5.0 + 0.25 * float((dd.double() ** 2).sum())
    assert want_log < 2 ** 24 and 4 * want_sq < 2 ** 24
    for form, (log_sum, sq_sum) in _forms().items():
        assert float(log_sum(lik, 0.5, out=_out(3.0))) == want_log, (form, n)                   # out is accumulated into
        assert float(sq_sum(a, b.cuda(), 0.25, out=_out(5.0))) == want_sq, (form, n)
        assert float(sq_sum(a, b.cuda(), 0.25)) == want_sq - 5.0, (form, n)
    # clamp01_a: a in {-0.5, 0, 1, 1.5} clamps to {0, 0, 1, 1}
    a = torch.tensor([-0.5, 0.0, 1.0, 1.5])[i % 4]
    b = torch.full((n,), 0.5)                      # (a - b)^2 in {1/4, 1}: sums of quarters
    for form, (_, sq_sum) in _forms().items():
        for clamp in (True, False):
            want, _ = E.sq_diff_sum(a, b, 2.0, clamp)
            assert 4 * want / 2.0 < 2 ** 24
            assert float(sq_sum(a.cuda(), b.cuda(), 2.0, clamp)) == want, (form, n, clamp)


@pytest.mark.parametrize("n", R.SUM_SIZES)
def test_sums_random_cases_within_the_derived_bounds(n):
    from hipops import ops
    lik, a, b = R.sum_case(n)
    cases = [("log2", lambda f, out: f[0](lik.cuda(), 0.25, out=out), E.neg_log2_sum(lik, 0.25))]
    for clamp in (False, True):
        cases.append((f"sq clamp={clamp}", lambda f, out, clamp=clamp: f[1](a.cuda(), b.cuda(), 3.0, clamp, out=out), E.sq_diff_sum(a, b, 3.0, clamp)))
    for what, run, (want, tot) in cases:
        for form, fns in _forms().items():
            bound = (R.ordered_bound if form == "ordered" else R.atomic_bound)(n, tot + 1.5)
            got = float(run(fns, _out(1.5)))
            print(f"[entropy parity] sum {what} {form} n={n}: err {abs(got - (want + 1.5)):.3e}, bound {bound:.3e} "
                  f"({abs(got - (want + 1.5)) / bound:.4f} of it)")
            assert abs(got - (want + 1.5)) <= bound, (what, form, n, got, want + 1.5)
        # the ordered form: the same bits on every launch, whatever the workspace held
        bits = []
        for _ in range(3):
            for ws in ops._workspaces("ordered_sum"):
                ws.fill_(float("nan"))
            bits.append(float(run(_forms()["ordered"], _out(1.5))))
        assert bits[0] == bits[1] == bits[2] and math.isfinite(bits[0]), (what, n, bits)


# ---- the autograd Functions of the R + lambda D task loss --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 5, 3, 7), (1, 192, 4, 6)])
def test_autograd_functions_match_float64_autograd(shape):
    """loss = NegLog2SumFn(lik_y, s1) + NegLog2SumFn(lik_z, s1) + SqDiffSumFn(y^, t_y, s2) + SqDiffSumFn(z^, t_z, s2) on NCHW tensors through
    GaussianLikelihoodFn / FactorizedLikelihoodFn: gradients to y, scales, means and z against float64 autograd of the reference composed
    the same way (straight-through rounding).  On top of the kernels' c * unit the hand-back f = g * lik * (-ln 2), g = -s1 / (ln 2 lik),
    and the products with it are <= 8 float32 roundings of each gradient term."""
    from hipops import autograd as A
    Cc = shape[1]
    g = torch.Generator().manual_seed(100 + Cc)
    _, params, med = R.make_eb(Cc, 60 + Cc)
    s = torch.exp(torch.empty(shape).uniform_(math.log(0.05), math.log(30.0), generator=g))
    m = 3.0 * torch.randn(shape, generator=g)
    y = m + 1.5 * s * torch.randn(shape, generator=g)
    z = 6.0 * torch.randn(shape, generator=g)
    t_y, t_z = y + torch.randn(shape, generator=g), z + torch.randn(shape, generator=g)
    s1, s2 = 1.0 / 64, 0.01
    leaf = lambda t: t.cuda().requires_grad_(True)
    yg, sg, mg, zg = leaf(y), leaf(s), leaf(m), leaf(z)
    yhat = A.round_ste(yg - mg) + mg
    lik_y = A.GaussianLikelihoodFn.apply(yhat, sg, mg, BOUND)
    zhat, lik_z = A.FactorizedLikelihoodFn.apply(zg, params.cuda(), med.cuda())
    loss = A.NegLog2SumFn.apply(lik_y, s1) + A.NegLog2SumFn.apply(lik_z, s1) + A.SqDiffSumFn.apply(yhat, t_y.cuda(), s2) \
        + A.SqDiffSumFn.apply(zhat, t_z.cuda(), s2)
    loss.backward()
    # reference: the float32 rounded values, gradient 1 to y / z through the rounding, float64 behind it
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    yhat_r = E.round_about(y, m)
    zhat_r = E.factorized(nhwc(z).contiguous(), params, med)[0].permute(0, 3, 1, 2)
    assert torch.equal(yhat.detach().cpu(), yhat_r) and torch.equal(zhat.detach().cpu(), zhat_r)
    y64, s64, m64, z64 = (t.double().requires_grad_(True) for t in (y, s, m, z))
    yh64 = yhat_r.double() + (y64 - y64.detach())
    zh64 = zhat_r.double() + (z64 - z64.detach())
    ly = E.gaussian_value(yh64, s64, m64, BOUND)
    lz = E.factorized_value(nhwc(zh64), params)
    dist_y, dist_z = s2 * ((yh64 - t_y.double()) ** 2).sum(), s2 * ((zh64 - t_z.double()) ** 2).sum()
    loss64 = s1 * (-torch.log2(ly)).sum() + s1 * (-torch.log2(lz)).sum() + dist_y + dist_z
    loss64.backward()
    # units and c of the four kernels on these inputs
    rg = R.gaussian_restatement_ratios(y.reshape(-1), s.reshape(-1), m.reshape(-1))
    rf = R.factorized_restatement_ratios(nhwc(z).contiguous(), params, med)
    _, _, us, um = E.gaussian_grad(yhat_r, s, m, BOUND, s1)
    _, udz = E.factorized_grad(nhwc(zhat_r).contiguous(), params, s1)
    udz = udz.permute(0, 3, 1, 2)
    keep_y = ~R.near_floor(R.gc_raw_p(yhat_r, s, m))
    keep_z = ~R.near_floor(R.eb_raw_p(nhwc(zhat_r).contiguous(), params)).permute(0, 3, 1, 2)
    assert int((~keep_y).sum()) <= 0.005 * y.numel() and int((~keep_z).sum()) <= 0.005 * z.numel()
    dy_d = 2 * s2 * (yhat_r.double() - t_y.double())                                 # the distortion's share of dL/dy, dL/dz
    dz_d = 2 * s2 * (zhat_r.double() - t_z.double())
    checks = [("scales", sg.grad, s64.grad, 4 * rg["ds"] * us + 8 * U * s64.grad.abs(), keep_y),
              ("means", mg.grad, m64.grad, 4 * rg["dm"] * um + 8 * U * m64.grad.abs(), keep_y),
              ("y", yg.grad, y64.grad, 4 * rg["dm"] * um + 8 * U * ((y64.grad - dy_d).abs() + dy_d.abs()), keep_y),
              ("z", zg.grad, z64.grad, 4 * rf["dz"] * udz + 8 * U * ((z64.grad - dz_d).abs() + dz_d.abs()), keep_z)]
    for what, got, want, tol, keep in checks:
        err = (got.cpu().double() - want).abs()
        worst = float(torch.where(err == 0, torch.zeros_like(err), err / tol)[keep].max())
        print(f"[entropy parity] autograd {shape} d/d{what}: worst err / allowed {worst:.3f}")
        assert worst <= 1.0, (what, worst)
    assert int((s64.grad == 0).sum()) > 0 and torch.equal(sg.grad.cpu() == 0, s64.grad == 0)          # scales below the bound
    # the loss value: the four atomic sums' worst-case bounds plus the likelihoods' own allowed error through -log2
    n = y.numel()
    _, _, ely = E.gaussian(y, s, m, BOUND)
    _, _, elz = E.factorized(nhwc(z).contiguous(), params, med)
    tol = sum(R.atomic_bound(n, float(t.detach())) for t in (s1 * (-torch.log2(ly)).sum(), s1 * (-torch.log2(lz)).sum(), dist_y, dist_z)) \
        + s1 * E.INV_LN2 * (4 * rg["fwd"] * float((ely / ly.detach()).sum()) + 4 * rf["fwd"] * float((elz / lz.detach()).sum()))
    assert abs(float(loss.detach()) - float(loss64.detach())) <= tol, (float(loss.detach()), float(loss64.detach()), tol)
