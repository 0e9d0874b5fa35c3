"""Learned rounding on the MX grids (csrc/mx_round.hip, include/rdo_ptq_mxround.h) on the GPU against tests/mx_round_reference.py.

  * neighbours, init, forward: lo, gap, the scale bytes, the hard weight and its codes bit for bit; alpha0 to the bound of the integer-grid
    init test (rtol = atol = 2e-6 against the oracle's fp32 formula); the soft weight to 4 ulp of h times gap.
  * one step against float64: the cases and the tolerance formulas of tests/test_gpu_adaround_step.py's docstring with delta -> gap per
    element (so wq: gap 1e-4 + 0.3 gap tol_alpha, per element) and the xint kink dropped (there is no level clamp).  Elements at a kink,
    judged on the float64 reference alone, are left out and must be finite: hraw within 1e-5 of 0 or 1, h within 1e-6 of 1/2 apart from
    the planted alpha = 0, q within 1e-6 gap of the reparam bound; at most 0.1 % of the drawn non-pinned elements.  Pinned elements keep
    alpha, m and v bit for bit and have wq = lo.
  * the engine against the oracle's unmodified loop on `MxQOp`s: the bounds of test_gpu_engine.py::test_engine_matches_oracle.
  * the public path: set_weight_format(..., rounding='learned'), block_ / layer_reconstruction, the stored form.

Measured on an MI355X (largest over the cases; `python -m pytest tests/test_gpu_mx_round.py -s` prints them per case):
  largest share of a bound used       m 0.98   v 0.73   alpha 0.73   wq 0.0097    (1.0 = the bound; no case needed the 2 x restatement rule)
  kernel error / fp32-restatement     m 1.22   v 1.36   alpha 1.03               (largest |kernel - f64| over largest |fp32 CPU - f64|)
  largest share of drawn non-pinned elements left out as kinks: 8.0e-4 (G36 mxfp4); 75 step cases in 1.2 s
  engine against the oracle loop: 0 of 523 .. 5243 decisions differ in every unit, hand-back forward error 1.2e-7 .. 3.4e-7: the bounds
  taken from the integer-grid test hold as they are
(first run of the file on the MI355X)
"""
import functools
import os
import types

import numpy as np
import pytest
import torch

import mx_reference as R
import mx_round_reference as RR
from helpers import T, nhwc, oracle_ops, product_unit
from oracle import rdo_oracle as O
from test_gpu_adaround_step import (P24, PLANTS, REPARAM, ROUND_WEIGHT, _counter, _dev_sched, _gamma_like, _guarded, _log, _ulp32, guards_intact,
                                    sched_table, state_of)

pytestmark = pytest.mark.gpu
SEED = 1005
KEYS = ("alpha", "m", "v", "wq")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------- neighbours, init, forward
SHAPES_NB = [(12, 63), (5, 27), (40, 216), (32, 96), (36, 36)]


@functools.lru_cache(maxsize=None)
def nb_case(shape, fmt):
    """a weight-row matrix with planted zeros, an all-zero block, elements on the grid, exact ties, +max X (pinned), -max X (not pinned), a
    tiny negative and -0 -> (w, reference neighbours)"""
    rows, inner = shape
    g = torch.Generator().manual_seed(rows * 1000 + inner)
    w = torch.randn(rows, inner, generator=g) * torch.pow(10.0, torch.linspace(-2, 0, rows))[:, None]
    w[0, :min(32, inner)] = 0.0                                            # an all-zero block
    w[1, ::5] = 0.0
    q, nb = R.quantize(w, fmt), RR.neighbours(w, fmt)
    w[2, :inner // 2] = q["wq"][2, :inner // 2]                            # on the grid
    live = nb["gap"][3] > 0
    w[3] = torch.where(live, nb["lo"][3] + 0.5 * nb["gap"][3], w[3])      # exact ties
    X = float(torch.ldexp(torch.ones(()), q["scales"][4, 0].int() - 127))
    vmax = R.FORMATS[fmt][5]
    w[4, 1], w[4, 2], w[4, 3], w[4, 4] = vmax * X, -vmax * X, -1e-30, -0.0
    nb = RR.neighbours(w, fmt)
    assert bool(nb["pinned"][4, 1]) and not bool(nb["pinned"][4, 2]) and torch.equal(nb["scales"], q["scales"])
    return w, nb


@pytest.mark.parametrize("fmt", R.NAMES)
@pytest.mark.parametrize("shape", SHAPES_NB)
def test_neighbours_init_and_forward_match_the_reference(shape, fmt):
    from hipops import ops
    w, nb = nb_case(shape, fmt)
    rows, inner = shape
    wd_ = w.cuda()
    lo, gap, scales = ops.mx_neighbours(wd_, fmt, want_scales=True)
    assert _same_bits(lo.cpu(), nb["lo"]) and _same_bits(gap.cpu(), nb["gap"])
    assert torch.equal(scales, ops.mx_fakequant(wd_, fmt, want=("scales",))["scales"]) and torch.equal(scales.cpu(), nb["scales"])
    lo2, gap2 = ops.mx_neighbours(wd_, fmt)
    assert torch.equal(lo2, lo) and torch.equal(gap2, gap)
    # init
    bufs = {}
    alpha = _guarded(bufs, "alpha", shape)
    ops.mx_round_init_alpha(wd_, lo, gap, alpha)
    a0 = RR.init_alpha(w, nb["lo"], nb["gap"])
    torch.testing.assert_close(alpha.cpu(), a0, rtol=2e-6, atol=2e-6)
    live = nb["gap"] > 0
    assert not alpha.cpu()[~live].any()
    tie = live & (((w - nb["lo"]) / torch.where(live, nb["gap"], torch.ones_like(w))) == 0.5)
    assert int(tie[3].sum()) >= inner // 2 and bool((alpha.cpu()[tie] == 0).all())
    # hard forward at alpha0: round to nearest off the ties, ties up; codes decode to it bit for bit; wd is the dgrad layout
    desc = ops.ada_desc(wd_.reshape(rows, 1, 1, inner))
    wq, wdg = _guarded(bufs, "wq", shape), _guarded(bufs, "wd", (inner, rows))
    out, codes = ops.mx_round_fwd(desc, lo, gap, alpha, False, fmt, wq=wq, wd=wdg, codes=True, scales=scales)
    hard = RR.forward(nb["lo"], nb["gap"], alpha.cpu(), False).float()
    assert out is wq and _same_bits(wq.cpu(), hard) and _same_bits(wdg.cpu(), hard.t().contiguous())
    assert _same_bits(ops.mx_dequant(codes, scales, inner, fmt), wq)
    rtn = ops.mx_fakequant(wd_, fmt)["wq"].cpu()
    assert torch.equal(wq.cpu()[~tie], rtn[~tie]) and torch.equal(wq.cpu()[tie], (nb["lo"] + nb["gap"])[tie])
    # every decision flipped: still on the grid, and the codes follow
    flipped = torch.where(alpha >= 0, torch.full_like(alpha, -1.0), torch.ones_like(alpha))
    wq2, codes2 = ops.mx_round_fwd(desc, lo, gap, flipped, False, fmt, codes=True, scales=scales)
    assert _same_bits(wq2.cpu(), RR.forward(nb["lo"], nb["gap"], flipped.cpu(), False).float())
    assert _same_bits(ops.mx_dequant(codes2, scales, inner, fmt), wq2)
    # soft forward, with and without the reparam (h is good to ~1.5e-7 in fp32: 4 ulp of 1 times gap, plus an ulp of the sum)
    g = torch.Generator().manual_seed(7)
    al = (a0 + 1.5 * torch.randn(shape, generator=g)).float()
    for reparam in (None, REPARAM):
        d = ops.ada_desc(wd_, reparam=reparam)          # [rows, inner] -> KH = KW = 1, Cin = inner
        soft = ops.mx_round_fwd(d, lo, gap, al.cuda(), True, fmt, wq=wq, wd=wdg)
        ref = RR.forward(nb["lo"], nb["gap"], al, True, reparam)
        tol = 4 * 2.0 ** -23 * nb["gap"].double() + 2 * _ulp32(nb["lo"]) + 1e-300
        if reparam is not None:
            tol = tol * 2 * (ref + REPARAM[1]).clamp(min=0).sqrt() + 2 * _ulp32(ref.float())
        assert bool(((soft.cpu().double() - ref).abs() <= tol).all())
        assert torch.equal(wdg, wq.t().contiguous())
        if reparam is None:
            assert torch.equal(soft.cpu()[~live], nb["lo"][~live])
    guards_intact({"_bufs": bufs})


def test_codes_with_soft_weights_are_refused():
    from hipops import ops
    w = torch.randn(4, 40).cuda()
    lo, gap, scales = ops.mx_neighbours(w, "mxfp4", want_scales=True)
    d = ops.ada_desc(w, conv_layout=False)
    with pytest.raises(ValueError, match="mx_round_fwd: codes describe the hard weight"):
        ops.mx_round_fwd(d, lo, gap, w, True, "mxfp4", codes=True, scales=scales)


# ----------------------------------------------------------------------------------------------------------------- one step against float64
# name: shape, nsplit, gamma (reparam), seed
STEP_SHAPES = {
    "A40x2x3x36": ((40, 2, 3, 36), 5, False, 1),
    "F12x3x3x7": ((12, 3, 3, 7), 1, False, 17),
    "H5x3x3x3": ((5, 3, 3, 3), 2, False, 9),
    "C32x1x1x96": ((32, 1, 1, 96), 29, False, 4),
    "G36": ((36, 36), 130, True, 5),
    "G64": ((64, 64), 3, True, 6),
}
STEP_CASES = [(n, f) for n in STEP_SHAPES for f in ("mxfp4", "mxfp8_e4m3")] + [("A40x2x3x36", f) for f in ("mxfp6_e2m3", "mxfp6_e3m2", "mxfp8_e5m2")]
COMBOS = [("first", 0, 1.0), ("mid", 2, 0.5), ("mid", 4, 1.0), ("first", 4, 0.5), ("mid", 0, 0.5)]
FIGURES = {}


@functools.lru_cache(maxsize=None)
def step_case(name, fmt):
    shape, nsplit, gamma, seed = STEP_SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    w = (_gamma_like(shape[0], g) if gamma else 0.1 * torch.randn(shape, generator=g)).float()
    n = w.numel()
    low = None
    if gamma:
        # the LowerBound rule's own side of its mask needs a soft weight strictly between 0 and the bound 2^-18; a stored gamma is never
        # below the bound, so eight weights are planted at 0: lo = 0 and h is set below so that q = gap h = min(0.4 gap, 0.75 bound)
        low = torch.tensor([(k * n) // 8 + 5 for k in range(8)])
        w.view(-1)[low] = 0.0
    rows = shape[0]
    # pinned elements in every case: +max X in block 0 of row 0 and, for a conv, a value just below -max X (neither moves the block's scale)
    top = R.FORMATS[fmt][5] * float(torch.ldexp(torch.ones(()), R.quantize(w.reshape(rows, -1), fmt)["scales"][0, 0].int() - 127))
    w.view(-1)[0] = top
    if not gamma:
        w.view(-1)[2] = -top * (1 + 2.0 ** -20)
    nb = RR.neighbours(w.reshape(rows, -1), fmt)
    lo, gap = nb["lo"].reshape(shape), nb["gap"].reshape(shape)
    live = gap > 0
    assert not bool(live.view(-1)[0]) and (gamma or not bool(live.view(-1)[2]))
    spread = 3.0 if fmt == "mxfp4" else 1.5
    alpha = (RR.init_alpha(w, lo, gap) + spread * torch.randn(shape, generator=g)).float()
    free = live.view(-1).clone()
    if low is not None:
        free[low] = False
    planted = []
    for k in range(8):                                                     # the planted alphas go to non-pinned elements
        i = (k * n) // 8 + 1
        while not bool(free[i]):
            i += 1
        free[i] = False
        planted.append(i)
    planted = torch.tensor(planted)
    alpha.view(-1)[planted] = torch.tensor(PLANTS)
    if low is not None:
        assert bool(live.view(-1)[low].all()) and not lo.view(-1)[low].any()
        h = torch.minimum(torch.full((8,), 0.4, dtype=torch.float64), 0.75 * REPARAM[0] / gap.view(-1)[low].double())
        alpha.view(-1)[low] = torch.logit((h + 0.1) / 1.2).float()
    slabs = (1e-2 * torch.randn((nsplit,) + shape, generator=g)).float()
    m = (1e-3 * torch.randn(shape, generator=g)).float()
    v = (1e-3 * torch.randn(shape, generator=g)).float().pow(2)
    return types.SimpleNamespace(name=name, fmt=fmt, shape=shape, nsplit=nsplit, reparam=REPARAM if gamma else None, w=w, lo=lo, gap=gap, live=live,
                                 alpha=alpha, planted=planted, slabs=slabs, m=m, v=v, rows=rows, low=low)


@functools.lru_cache(maxsize=None)
def step_reference(name, fmt, state, counter, grad_scale):
    c = step_case(name, fmt)
    m, v = state_of(c, state)
    return RR.step(c.lo, c.gap, c.alpha, m, v, c.slabs.double().sum(0), sched_table()[counter], grad_scale=grad_scale, round_weight=ROUND_WEIGHT,
                   reparam=c.reparam)


def restate_fp32(c, state, counter, grad_scale):
    """The kernel's chain op by op in torch float32 on the CPU (libm transcendentals): what fp32 alone costs against float64."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    b, on, step, bc2 = (f(float(x)) for x in sched_table()[counter])
    m, v = state_of(c, state)
    G = torch.zeros_like(c.w)
    for s in range(c.nsplit):
        G = G + c.slabs[s]
    k12, k01 = f(1.1) - f(-0.1), f(-0.1)
    sg = 1.0 / (1.0 + torch.exp(-c.alpha))
    hraw = sg * k12 + k01
    h = hraw.clamp(0, 1)
    dh = ((hraw >= 0) & (hraw <= 1)).float() * (k12 * (sg * (1 - sg)))
    g = G
    if c.reparam is not None:
        q = c.lo + c.gap * h
        go = G * (2 * q.clamp(min=REPARAM[0]))
        g = torch.where((q >= REPARAM[0]) | (go < 0), go, torch.zeros_like(go))
    gt = ((g * c.gap) * dh) * f(grad_scale)
    if float(on):
        u = (h - 0.5).abs() * 2
        ub1 = torch.where(u > 0, torch.pow(u.clamp(min=1e-37), b - 1), torch.zeros_like(u))
        gt = gt + (-f(ROUND_WEIGHT) * (b * ub1) * 2 * torch.sign(h - 0.5)) * dh
    fma = lambda x, y, z: (x.double() * y.double() + z.double()).float()
    m1 = fma(gt - m, f(1 - 0.9), m)
    v1 = fma(v, f(0.999), f(1 - 0.999) * gt * gt)
    a1 = c.alpha - step * (m1 / (v1.sqrt() / bc2 + f(1e-8)))
    return dict(m=m1, v=v1, alpha=a1, h=h)


def tolerances(c, ref, state, counter, grad_scale, h_err):
    """per-element bounds for m, v, alpha, wq: test_gpu_adaround_step.py's `tolerances` with delta -> gap per element and pass_q = 1"""
    b, on, step, bc2 = (float(x) for x in sched_table()[counter])
    m_in, v_in = state_of(c, state)
    mk = ref["masks"]
    gap = c.gap.double()
    sg = (mk["hraw"] + 0.1) / 1.2
    dh = ((mk["hraw"] >= 0) & (mk["hraw"] <= 1)).double() * 1.2 * sg * (1 - sg)
    dq = gap * dh
    if c.reparam is not None:
        dq = dq * 2 * mk["q"].clamp(min=REPARAM[0])
    tol_gd = (c.nsplit + 16) * P24 * grad_scale * dq * c.slabs.double().abs().sum(0)
    if c.reparam is not None:
        above = (mk["q"] >= REPARAM[0]).double()
        tol_gd = tol_gd + grad_scale * c.slabs.double().sum(0).abs() * 2 * (gap * 4 * h_err) * gap * dh * above
    u = (mk["h"] - 0.5).abs() * 2
    lg = torch.where(u > 0, torch.log2(u.clamp(min=1e-300)), torch.zeros_like(u))
    tol_gr = P24 * ref["g_round"].abs() * (16 + 2 * ((b - 1) * lg).abs())
    if on:
        ub2 = torch.where(u > 0, u.clamp(min=1e-300) ** (b - 2), torch.zeros_like(u)) if b != 2.0 else torch.ones_like(u)
        tol_gr = tol_gr + ROUND_WEIGHT * b * (b - 1) * ub2 * 2 * 2 * dh * 4 * h_err
    tol_g = tol_gd + tol_gr
    m1, v1 = ref["m"], ref["v"]
    tol_m = 0.1 * tol_g + P24 * torch.maximum(m1.abs(), m_in.double().abs())
    tol_v = 0.001 * 2 * ref["g_total"].abs() * tol_g + 2 * P24 * torch.maximum(v1.abs(), v_in.double().abs())
    D = v1.sqrt() / bc2 + 1e-8
    dv = torch.where(v1 > 0, step * m1.abs() / D ** 2 * tol_v / (2 * v1.sqrt().clamp(min=1e-300) * bc2), torch.zeros_like(v1))
    tol_a = step / D * tol_m + dv + 2 * torch.maximum(_ulp32(c.alpha), _ulp32(ref["alpha"]))
    tol_wq = gap * 1e-4 + 0.3 * gap * tol_a
    if c.reparam is not None:
        tol_wq = tol_wq * 2 * (ref["wq"] + REPARAM[1]).clamp(min=0).sqrt()
    return dict(m=tol_m, v=tol_v, alpha=tol_a, wq=tol_wq)


def _kinks(c, ref):
    mk = ref["masks"]
    hraw, h = mk["hraw"], mk["h"]
    zeros = torch.zeros_like(h, dtype=torch.bool)
    zeros.view(-1)[c.planted[:2]] = True                                      # the planted alpha = 0 (u = 0) must be compared
    k = (hraw.abs() < 1e-5) | ((hraw - 1).abs() < 1e-5) | (((h - 0.5).abs() < 1e-6) & ~zeros)
    if c.reparam is not None:
        # a gamma stores its vanished cross terms as exactly the bound 2^-18, which is on every grid here: with h clamped to 0 or 1 the
        # soft weight is lo or lo + gap in fp32 and in float64 alike (and dh/dalpha = 0): no branch to disagree on, so those are compared
        k |= ((mk["q"] - REPARAM[0]).abs() < 1e-6 * c.gap.double()) & (mk["hraw"] > 0) & (mk["hraw"] < 1)
    return k & c.live


def make_item(c, state):
    from hipops import ops
    bufs = {}
    m, v = state_of(c, state)
    lo = c.lo.cuda()
    d = ops.ada_desc(lo, reparam=c.reparam)
    return dict(d=d, lo=lo, gap=c.gap.cuda(), slabs=c.slabs.cuda(), _bufs=bufs, alpha=_guarded(bufs, "alpha", c.shape, init=c.alpha),
                m=_guarded(bufs, "m", c.shape, init=m), v=_guarded(bufs, "v", c.shape, init=v), wq=_guarded(bufs, "wq", c.shape),
                wd=_guarded(bufs, "wd", c.shape))


def run_step(item, counter, grad_scale):
    from hipops import ops
    log, word = _log(), _counter(counter)
    ops.mx_round_step(item["d"], item["lo"], item["gap"], item["slabs"], grad_scale, ROUND_WEIGHT, _dev_sched(), word, item["alpha"], item["m"],
                      item["v"], item["wq"], item["wd"], log)
    torch.cuda.synchronize()
    assert word.tolist() == [counter]                                         # the step reads the counter and never moves it
    return log


@pytest.mark.parametrize("state,counter,grad_scale", COMBOS)
@pytest.mark.parametrize("name,fmt", STEP_CASES)
def test_step_matches_float64(name, fmt, state, counter, grad_scale):
    c = step_case(name, fmt)
    ref = step_reference(name, fmt, state, counter, grad_scale)
    mk = ref["masks"]
    live, pinned = c.live, ~c.live
    pass_h = (mk["hraw"] >= 0) & (mk["hraw"] <= 1)
    assert float((~pass_h)[live].double().mean()) >= 0.10                     # the reference really exercises the mask of h
    kink = _kinks(c, ref)
    G = c.slabs.double().sum(0)
    if c.reparam is not None:          # the LowerBound rule on both sides of its mask: 0 < q < bound, the gradient blocked and passed
        q, Gl = mk["q"].view(-1)[c.low], G.view(-1)[c.low]
        assert bool(((q > 0) & (q < REPARAM[0])).all()) and not bool(kink.view(-1)[c.low].any()) and bool(pass_h.view(-1)[c.low].all())
        assert int((Gl > 0).sum()) >= 2 and int((Gl < 0).sum()) >= 2
        assert bool((ref["dalpha_data"].view(-1)[c.low][Gl > 0] == 0).all()) and bool((ref["dalpha_data"].view(-1)[c.low][Gl < 0] != 0).all())
    drawn = live.clone()
    drawn.view(-1)[c.planted] = False
    left_out = float((kink & drawn).sum()) / max(1, int(drawn.sum()))
    assert left_out <= 1e-3, f"{left_out:.2e} of the drawn non-pinned elements sit on a kink: change the seed"
    assert bool(kink.view(-1)[c.planted[2:4]].all()) and not bool(kink.view(-1)[c.planted[:2]].any())

    item = make_item(c, state)
    log = run_step(item, counter, grad_scale)
    guards_intact(item)
    fp32 = restate_fp32(c, state, counter, grad_scale)
    h_err = float((fp32.pop("h").double() - mk["h"]).abs()[live].max())
    tol = tolerances(c, ref, state, counter, grad_scale, h_err)
    keep = live & ~kink
    worst = {}
    m_in, v_in = state_of(c, state)
    for k in KEYS:
        got = item[k].cpu().double()
        assert bool(torch.isfinite(got).all()), f"{k}: non-finite output"
        err = (got - ref[k]).abs()
        worst[k] = float((err / tol[k].clamp(min=1e-300))[keep].max())
        if k in fp32:
            e32 = float((fp32[k].double() - ref[k]).abs()[keep].max())
            worst[k + "_vs_fp32"] = float(err[keep].max()) / e32 if e32 > 0 else 0.0
    FIGURES[(name, fmt, state, counter, grad_scale)] = dict(worst, left_out=left_out)
    print(f"\n[mx-step] {name} {fmt} {state} it={counter} gs={grad_scale} pinned={int(pinned.sum())} left_out={left_out:.2e} " +
          " ".join(f"{k}={x:.3g}" for k, x in worst.items()))
    for k in KEYS:
        # a bound that is exceeded is measured against the fp32 restatement's own largest error on the same case: 2 x that is allowed
        # (tests/test_gpu_adaround_step.py has the integer-grid kernel at 1.05-1.32 x the restatement); wq has no restatement
        assert worst[k] <= 1.0 or 0.0 < worst.get(k + "_vs_fp32", 0.0) <= 2.0, \
            f"{k}: error is {worst[k]:.3g} x its bound and {worst.get(k + '_vs_fp32', float('nan')):.3g} x the fp32 restatement's"
    # a pinned element does not exist for the optimiser
    assert int(pinned.sum()) >= 1
    for k, before in (("alpha", c.alpha), ("m", m_in), ("v", v_in)):
        assert _same_bits(item[k].cpu()[pinned], before[pinned]), f"{k} of a pinned element was written"
    want = c.lo if c.reparam is None else (c.lo.clamp(min=REPARAM[0]) ** 2 - REPARAM[1])
    assert torch.equal(item["wq"].cpu()[pinned], want[pinned])
    # the dgrad layout
    co, ci = c.shape[0], c.shape[-1]
    kh, kw = (c.shape[1], c.shape[2]) if len(c.shape) == 4 else (1, 1)
    assert torch.equal(item["wd"].reshape(ci, kh, kw, co), item["wq"].reshape(co, kh, kw, ci).flip(1, 2).permute(3, 1, 2, 0).contiguous())
    on = float(sched_table()[counter, 1])
    log = log.cpu().double()
    if on:
        want = float(ref["round_loss"])
        assert want > 0 and abs(float(log[counter].sum()) - want) <= 1e-5 * want
    assert float(log.abs().sum() - log[counter].abs().sum()) == 0.0 and (on or float(log.abs().sum()) == 0.0)


def test_scalar_form_for_unaligned_streams_equals_the_float4_form():
    """numel % 4 == 0 with streams that are only 4-byte aligned takes the scalar kernel: the same bits"""
    from hipops import ops
    c = step_case("A40x2x3x36", "mxfp4")
    a, b = make_item(c, "mid"), make_item(c, "mid")
    n = c.w.numel()
    shifted = torch.empty(n + 1, device="cuda")[1:].view(c.shape)           # 4 bytes off a 16-byte boundary
    shifted.copy_(b["lo"])
    b["lo"] = shifted
    log_a, log_b = run_step(a, 2, 0.5), run_step(b, 2, 0.5)
    for k in KEYS + ("wd",):
        assert torch.equal(a[k], b[k]), k
    torch.testing.assert_close(log_a.sum(1), log_b.sum(1), rtol=1e-6, atol=0)
    guards_intact(a), guards_intact(b)


# ----------------------------------------------------------------------------------------------------------------- the engine against the oracle
@pytest.fixture(scope="module")
def recon(golden_dir):
    return np.load(os.path.join(golden_dir, "recon_toy.npz"))


def _mx_oracle(op, fmt):
    return RR.MxQOp.of(fmt)(op.kind, op.weight, op.bias, stride=op.stride, padding=op.padding, output_padding=op.output_padding, act=op.act)


def _install(unit, fmt):
    from quantization import QuantModule
    from quantization.mx import MXAdaRoundQuantizer
    for m in unit.modules():
        if isinstance(m, QuantModule) and m.org_weight is not None:
            m.weight_quantizer = MXAdaRoundQuantizer(fmt, tconv=m.if_tconv)


def _engine_vs_oracle(kind, ops_o, unit, mods, fx, tag, B, iters, graph, fwd_ref):
    from quantization.engine import UnitEngine, _MxOp
    idx = fx[f"{tag}/idx"]
    log = O.reconstruct_unit(kind, ops_o, T(fx[f"{tag}/inp_q"]), T(fx[f"{tag}/inp_fp"]), T(fx[f"{tag}/out"]), iters=iters, batch_size=B, idx_stream=idx,
                             mask_fn=lambda i, shape: O.qdrop_keep_mask_nhwc(SEED, i, shape, 0.5), input_prob=0.5, weight=0.01, b_range=(20, 2),
                             warmup=0.2)
    eng = UnitEngine(kind, mods, nhwc(fx[f"{tag}/inp_q"]), nhwc(fx[f"{tag}/inp_fp"]), nhwc(fx[f"{tag}/out"]), batch_size=B, iters=iters, weight=0.01,
                     b_range=(20, 2), warmup=0.2, input_prob=0.5, seed=SEED, idx_table=torch.from_numpy(idx), use_graph=graph)
    assert all(isinstance(op, _MxOp) for op in eng.ops.values()) and not eng._handover and not eng._folded
    eng.run()
    torch.cuda.synchronize()
    total, rt, rd = eng.logs()
    np.testing.assert_allclose(total.numpy(), np.array(log.total), rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(rd.numpy(), np.array(log.round), rtol=2e-4, atol=1e-7)
    assert float(rd[-1]) > 0
    flips = tot = 0
    for n, op in ops_o.items():
        a_gpu, live = eng.alpha_of(n).cpu(), op.gap > 0
        assert a_gpu.shape == op.alpha.shape
        # (the engine's lo / gap in the logical layout are the oracle's: the layout trap of a transposed conv)
        e = eng.ops[n]
        lo_l = e.lo.flip(1, 2).permute(3, 0, 1, 2) if e.tconv is not None else (e.lo.permute(0, 3, 1, 2) if e.lo.dim() == 4 else e.lo)
        assert _same_bits(lo_l.cpu().reshape(op.lo.shape), op.lo)
        np.testing.assert_allclose(a_gpu[live].numpy(), op.alpha[live].numpy(), rtol=0, atol=2e-3)
        assert not a_gpu[~live].any() and bool((op.alpha[~live] == RR.PINNED_ALPHA).all())
        flips += int(((a_gpu >= 0) != (op.alpha >= 0))[live].sum())
        tot += int(live.sum())
    assert flips <= 0.005 * tot, f"{flips}/{tot} rounding decisions differ"
    eng.finish()
    from quantization.mx import MXAdaRoundQuantizer
    for m in unit.modules():
        if hasattr(m, "trained"):
            m.trained = True
        q = getattr(m, "weight_quantizer", None)
        if q is not None and getattr(m, "org_weight", None) is not None:
            assert type(q) is MXAdaRoundQuantizer and q.alpha is not None and q.soft_targets is False
    unit.set_quant_state(True, False)
    with torch.no_grad():
        y = unit(T(fx[f"{tag}/inp_q"][:2]).cuda())
        y_ref = fwd_ref(T(fx[f"{tag}/inp_q"][:2]))
    err = float((y.cpu() - y_ref).abs().max() / (y_ref.abs().max() + 1e-12))
    print(f"\n[mx-engine] {tag} {kind} flips={flips}/{tot} hand-back err={err:.3g} loss {float(total[0]):.5g} -> {float(total[-1]):.5g}")
    assert err < (5e-3 if flips else 2e-5), err


ENGINE_CASES = [(t, k, f, True) for t, k in (("g_a.0", "rbws"), ("g_a.1", "rb"), ("g_a.6", "layer"), ("g_s.1", "rbu")) for f in ("mxfp4", "mxfp8_e4m3")] + \
               [("g_a.1", "rb", "mxfp4", False)]


@pytest.mark.parametrize("tag,kind,fmt,graph", ENGINE_CASES)
def test_engine_matches_the_oracle_loop_on_an_mx_grid(recon, tag, kind, fmt, graph):
    fx = recon
    _, _, B, iters = (int(v) for v in fx["meta"])
    ops_o = {n: _mx_oracle(op, fmt) for n, op in oracle_ops(fx, tag, kind).items()}
    unit, k, mods = product_unit(fx, tag, kind)
    _install(unit, fmt)
    _engine_vs_oracle(kind, ops_o, unit, mods, fx, tag, B, iters, graph, lambda x: O.UNIT_FORWARD[kind](ops_o, x))


def test_engine_transposed_conv_unit_on_an_mx_grid(golden_dir):
    """the flip: a transposed conv's blocks run along the unflipped rows, the engine keeps its tensors with the taps flipped"""
    from helpers import MINNEN_UNITS, minnen_oracle_op, minnen_product_module
    fx = np.load(os.path.join(golden_dir, "recon_minnen.npz"))
    B, iters = int(fx["meta"][3]), int(fx["meta"][4])
    tag = next(t for t in MINNEN_UNITS if str(fx[f"{t}/kind"]) == "tconv")
    op_o = _mx_oracle(minnen_oracle_op(fx, tag), "mxfp4")
    assert op_o.weight.shape[0] % 32 != 0                                 # Cin % 32 != 0: blocks span taps
    qm = minnen_product_module(fx, tag)
    _install(qm, "mxfp4")
    _engine_vs_oracle("layer", {"layer": op_o}, qm, {"layer": qm}, fx, tag, B, iters, True, op_o)


# ----------------------------------------------------------------------------------------------------------------- the public path
def test_learned_rounding_through_the_public_api():
    from hipops import ops
    from quantization import QuantModule, block_reconstruction, layer_reconstruction
    from quantization.mx import MXAdaRoundQuantizer
    from quantization.quantizer import to_rows
    from test_gpu_unit_report import _toy
    qnn, cali, _, kwargs = _toy()
    units = qnn.units()
    qnn.set_quant_state(True, False)
    block, layer, other = "g_a.1", "g_a.6", "g_a.0"
    weighted = lambda u: [m for m in u.modules() if isinstance(m, QuantModule) and m.org_weight is not None]
    x_other = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        y_other = units[other](x_other).clone()
    with pytest.raises(ValueError, match="set_weight_format: rounding must be one of"):
        qnn.set_weight_format({block: "mxfp4"}, rounding="hard")
    qnn.set_weight_format({block: "mxfp4", layer: "mxfp4"}, rounding="learned")
    mods = weighted(units[block]) + weighted(units[layer])
    assert len(mods) >= 3 and all(type(m.weight_quantizer) is MXAdaRoundQuantizer and m.weight_quantizer.alpha is None for m in mods)
    before = []
    for m in mods:                                                            # before calibration: round to nearest, MXQuantizer's bits
        q = m.weight_quantizer
        rows = q._rows(m.weight.detach())
        rtn = ops.mx_fakequant(rows, "mxfp4", want=("wq", "codes", "scales"))
        codes, scales = q.codes_and_scales(m.weight)
        assert torch.equal(codes, rtn["codes"]) and torch.equal(scales, rtn["scales"])
        assert _same_bits(q._rows(q(m.weight).contiguous()), rtn["wq"])
        before.append((rtn["wq"], scales))
    kw = dict(kwargs, iters=12, act_quant=False)
    eng = block_reconstruction(qnn, units[block], block.split(".")[-1], **kw)
    assert eng is not None and float(eng.logs()[0][-1]) > 0
    layer_reconstruction(qnn, units[layer], layer.split(".")[-1], **kw)
    moved = 0
    for m, (rtn, scales0) in zip(mods, before):
        q = m.weight_quantizer
        assert m.trained and type(q) is MXAdaRoundQuantizer and q.alpha is not None and q.soft_targets is False
        assert tuple(q.alpha.shape) == tuple(to_rows(m.weight, m.if_tconv).shape)
        wq = q._rows(q(m.weight).contiguous())
        codes, scales = q.codes_and_scales(m.weight)
        assert _same_bits(ops.mx_dequant(codes, scales, wq.shape[1], "mxfp4"), wq)          # the stored form is what is forwarded
        assert torch.equal(scales, scales0)                                                  # learned rounding never moves a scale
        lo, gap = ops.mx_neighbours(q._rows(m.weight.detach()), "mxfp4")
        assert bool(((wq == lo) | (wq == lo + gap)).all())
        moved += int((wq != rtn).sum())
    print(f"\n[mx-api] {moved} weights left round to nearest in 12 iterations")
    with pytest.raises(ValueError, match=f"set_weight_format: unit '{block}' holds a trained module"):
        qnn.set_weight_format({block: "int"})
    with pytest.raises(ValueError, match=f"set_weight_format: unit '{layer}' holds a trained module"):
        qnn.set_weight_format({layer: "mxfp4"}, rounding="learned")
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        assert _same_bits(units[other](x_other), y_other)                                    # an untouched unit computes what it computed
        out = qnn(cali[:2])
    assert bool(torch.isfinite(out["x_hat"]).all())
