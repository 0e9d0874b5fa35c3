"""One AdaRound step of every kernel form and output layout of csrc/adaround.hip against `O.adaround_step_reference` (float64, closed
form; pinned to autograd by tests/test_adaround_step_reference.py).

The engine tests follow alpha over a dozen Adam steps, and Adam normalises the gradient: a first step moves alpha by lr * sign(g)
whatever the size of g.  adam_m and adam_v are linear and quadratic in g, so one step read against float64 shows a wrong magnitude
(a regulariser slope, an exponent, beta2, grad_scale, the side of a LowerBound mask) at once.

Which form a tensor takes (csrc/adaround.hip):
  * the single-tensor entry `rdo_adaround_step`: the flat form, float4 streams (numel % 4 == 0) or the scalar kernel, then
    wd_transpose_kernel for the dgrad layout;
  * the batch entry `rdo_adaround_step_batch`: the TILE form for every tensor with a conv descriptor, Cin % 4 == 0 and rows % 4 == 0
    (a [C, C] gamma is the one-tap case) -- it takes precedence over the slab count; every other tensor the flat float4 form, or one
    element per thread from `ada_w1_min` slabs on.  A gamma therefore reaches the one-element-per-thread path only with a descriptor
    that has no conv layout (`conv_layout=False`).

Tolerances of `test_step_matches_float64` (per element, from the reference's own magnitudes; P = 2^-24):
  data term       tol_gd = (nsplit + 16) P grad_scale |dq/dalpha| sum_s |slab_s|   (x 2 lb with reparam): one rounding per slab add plus
                  the chain's multiplies
  h's rounding    the list above has no term for the ABSOLUTE rounding of h = clamp(1.2 sigmoid(alpha) - 0.1) (~1e-7, whoever computes it in
                  fp32): it enters u = 2 |h - 1/2| -- near h = 1/2 the relative bound of the rounding term goes to 0 with u -- and, with
                  reparam, lb = q = (h + ...) delta of weights below one step.  No constant is invented for it: the fp32 restatement's own
                  largest |h - h64| of the case is measured (1.2-1.6e-7), allowed 4 x, and carried to first order through |d g_round / d h|
                  and |d g_data / d h|
  rounding term   tol_gr = P |g_round| (16 + 2 |(b - 1) log2 u|): pow_u's documented 4e-8 |p log2 u| plus the chain
  tol_m = 0.1 (tol_gd + tol_gr) + P |m|,   tol_v = 0.001 * 2 |g| (tol_gd + tol_gr) + 2 P |v|
  alpha           tol_m and tol_v through step_size * m / (sqrt(v) / bc2 + 1e-8) to first order, plus 2 ulp32(alpha)
  wq              delta.max() * 1e-4 + 0.3 delta tol_alpha   (x 2 lb with reparam)
  log             rtol 1e-5 (the lp-loss kernel test's figure)
Elements at a kink of the chain (judged on the float64 reference alone, `_kinks`) are left out of the comparison and must be finite; at
most 0.1 % of the DRAWN elements of a case may be left out.  The two planted +-2.3979 = +-ln 11 sit on hraw = 1 / hraw = 0 by
construction (4e-7 away): they are kinks in every case and do not count against that share.

The schedule table is make_sched(5, 0.4, (20, 2)): counter 0 is a warm-up row (round_on = 0), counter 2 has b = 14, counter 4 has b = 2
(exponent b - 1 = 1); one more case takes a row with a fractional b = 19.25 from the anchor's table.

Measured on an MI355X (largest over the cases; `python -m pytest tests/test_gpu_adaround_step.py -s` prints them per case):
  largest share of a bound used       m 0.97   v 0.80   alpha 0.52   wq 0.56      (1.0 = the bound)
  kernel error / fp32-restatement     m 1.32   v 1.20   alpha 1.05               (largest |kernel - f64| over largest |fp32 CPU - f64|)
  largest share of drawn elements left out as kinks: 6.5e-4 (tile-lin-b); 61 cases, under 2 s in total
(first run of the file on the MI355X; the two gamma cases were redrawn afterwards with planted LowerBound elements)
"""
import functools
import math
import types

import numpy as np
import pytest
import torch

from oracle import rdo_oracle as O

pytestmark = pytest.mark.gpu

P24 = 2.0 ** -24
REPARAM = (2.0 ** -18, 2.0 ** -36)
ROUND_WEIGHT = 0.01
GUARD = 64
PLANTS = (0.0, 0.0, 2.3979, -2.3979, 90.0, 90.0, -90.0, -90.0)
KEYS = ("alpha", "m", "v", "wq")


# ----------------------------------------------------------------------------------------------------------------- cases (CPU draws)
def _gamma_like(c, g):
    """A GDN gamma as a trained CompressAI state stores it (tests/helpers.trained_like_): non-diagonal, Laplace tails, sqrt(. + 2^-36)."""
    u = torch.rand((c, c), generator=g) - 0.5
    lap = (-torch.sign(u) * torch.log1p(-2 * u.abs().clamp(max=0.4999999))).abs()
    diag = 0.05 * 8.0 ** torch.rand(c, generator=g)
    off = (0.3 / c) * lap * 10.0 ** ((torch.rand(c, 1, generator=g) - 0.5) * 1.5)
    off = off * (torch.rand((c, c), generator=g) > 0.05)            # one in twenty cross terms vanishes (CompressAI starts gamma at 0.1 I):
    return torch.sqrt((torch.diag(diag) + off).abs() + 2.0 ** -36)  # those entries sit on the LowerBound's bound 2^-18, below one step


# name: shape, n_levels, nsplit, gamma (reparam), seed
SHAPES = {
    "A40x2x3x36": ((40, 2, 3, 36), 256, 5, False, 1),
    "B48x3x3x48": ((48, 3, 3, 48), 1024, 13, False, 2),
    "C64x1x1x32": ((64, 1, 1, 32), 256, 29, False, 3),
    "C32x1x1x96": ((32, 1, 1, 96), 256, 29, False, 4),
    "G36": ((36, 36), 256, 130, True, 5),
    "G64": ((64, 64), 256, 3, True, 6),
    "F12x3x3x7": ((12, 3, 3, 7), 16, 1, False, 17),
    "S8x2": ((8, 2), 256, 2, False, 8),
    "H5x3x3x3": ((5, 3, 3, 3), 256, 2, False, 9),
    "L24x3x3x16": ((24, 3, 3, 16), 256, 4, False, 10),          # layer-wise scales: delta / zp of ONE row
    "T16x1x1x16": ((16, 1, 1, 16), 256, 2, False, 11),          # a one-tile tensor (the ends of the mixed batch)
}


@functools.lru_cache(maxsize=None)
def case(name):
    shape, n_levels, nsplit, gamma, seed = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    bits = int(math.log2(n_levels))
    w = (_gamma_like(shape[0], g) if gamma else 0.1 * torch.randn(shape, generator=g)).float()
    layerwise = name.startswith("L")
    if layerwise:
        delta, zp = O.uaq_init(w, bits, False, "max")
        delta, zp = delta.reshape(1).float(), zp.reshape(1).float()
    else:
        delta, zp = O.uaq_init(w, bits, True, "max")
        delta, zp = delta.reshape(-1).float(), zp.reshape(-1).float()
    bshape = (-1,) + (1,) * (w.dim() - 1)
    spread = 3.0 if bits == 4 else 1.5
    alpha = (O.adaround_init_alpha(w, delta.view(bshape)) + spread * torch.randn(shape, generator=g)).float()
    n = alpha.numel()
    planted = torch.tensor([(k * n) // 8 + 1 for k in range(8)])
    alpha.view(-1)[planted] = torch.tensor(PLANTS)
    slabs = (1e-2 * torch.randn((nsplit,) + shape, generator=g)).float()
    m = (1e-3 * torch.randn(shape, generator=g)).float()
    v = (1e-3 * torch.randn(shape, generator=g)).float().pow(2)
    low = None
    if gamma:
        # the LowerBound rule's own side of its mask: eight more planted elements whose soft q lies strictly between 0 and the bound
        # (floor(w / delta) = 0 and h = 0.75 bound / delta, above the 1e-3 kink zone of xint) -- the drawn alphas put ~1 element there
        dl = delta.view(bshape).expand_as(w).reshape(-1)
        low = ((w.view(-1) < dl) & (dl < REPARAM[0] / 2e-3)).nonzero().view(-1)
        low = low[~torch.isin(low, planted)][:8]
        assert low.numel() == 8
        alpha.view(-1)[low] = torch.logit((0.75 * REPARAM[0] / dl[low] + 0.1) / 1.2).float()
    return types.SimpleNamespace(name=name, shape=shape, n_levels=n_levels, nsplit=nsplit, reparam=REPARAM if gamma else None, w=w,
                                 delta=delta, zp=zp, bshape=bshape, alpha=alpha, planted=planted, slabs=slabs, m=m, v=v,
                                 layerwise=layerwise, rows=shape[0], inner=n // shape[0], low=low)


@functools.lru_cache(maxsize=None)
def sched_table(which="short"):
    from hipops import ops
    return ops.make_sched(5, 0.4, (20, 2), device="cpu") if which == "short" else ops.make_sched(30, 0.2, (20, 2), device="cpu")


def state_of(c, state):
    return (torch.zeros_like(c.m), torch.zeros_like(c.v)) if state == "first" else (c.m, c.v)


@functools.lru_cache(maxsize=None)
def reference(name, state, counter, grad_scale, which="short"):
    c = case(name)
    m, v = state_of(c, state)
    return O.adaround_step_reference(c.w, c.delta.view(c.bshape), c.zp.view(c.bshape), c.alpha, m, v, c.slabs.double().sum(0),
                                     sched_table(which)[counter], n_levels=c.n_levels, grad_scale=grad_scale, round_weight=ROUND_WEIGHT,
                                     reparam=c.reparam)


def restate_fp32(c, state, counter, grad_scale, which="short"):
    """The kernels' chain op by op in torch float32 on the CPU (libm transcendentals): what fp32 alone costs against float64."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    b, on, step, bc2 = (f(float(x)) for x in sched_table(which)[counter])
    m, v = state_of(c, state)
    dl, z = c.delta.view(c.bshape), c.zp.view(c.bshape)
    Lm1 = float(c.n_levels - 1)
    G = torch.zeros_like(c.w)
    for s in range(c.nsplit):
        G = G + c.slabs[s]
    k12, k01 = f(1.1) - f(-0.1), f(-0.1)
    xf = torch.floor(c.w / dl)
    sg = 1.0 / (1.0 + torch.exp(-c.alpha))
    hraw = sg * k12 + k01
    h = hraw.clamp(0, 1)
    xint = xf + h + z
    dh = ((hraw >= 0) & (hraw <= 1)).float() * (k12 * (sg * (1 - sg)))
    g = G
    if c.reparam is not None:
        q = (xint.clamp(0, Lm1) - z) * dl
        go = G * (2 * q.clamp(min=REPARAM[0]))
        g = torch.where((q >= REPARAM[0]) | (go < 0), go, torch.zeros_like(go))
    gt = ((g * dl) * ((xint >= 0) & (xint <= Lm1)).float() * dh) * f(grad_scale)
    if float(on):
        u = (h - 0.5).abs() * 2
        ub1 = torch.where(u > 0, torch.pow(u.clamp(min=1e-37), b - 1), torch.zeros_like(u))
        gt = gt + (-f(ROUND_WEIGHT) * (b * ub1) * 2 * torch.sign(h - 0.5)) * dh
    fma = lambda x, y, z: (x.double() * y.double() + z.double()).float()       # (a float product is exact in double)
    m1 = fma(gt - m, f(1 - 0.9), m)
    v1 = fma(v, f(0.999), f(1 - 0.999) * gt * gt)
    a1 = c.alpha - step * (m1 / (v1.sqrt() / bc2 + f(1e-8)))
    return dict(m=m1, v=v1, alpha=a1, h=h)


def _ulp32(x):
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def tolerances(c, ref, state, counter, grad_scale, which="short", h_err=0.0):
    """-> per-element bounds for m, v, alpha, wq (module docstring); h_err: the fp32 restatement's largest |h - h64| of the case."""
    b, on, step, bc2 = (float(x) for x in sched_table(which)[counter])
    m_in, v_in = state_of(c, state)
    mk = ref["masks"]
    delta = c.delta.view(c.bshape).double()
    sg = (mk["hraw"] + 0.1) / 1.2
    dh = ((mk["hraw"] >= 0) & (mk["hraw"] <= 1)).double() * 1.2 * sg * (1 - sg)
    dq = delta * ((mk["xint"] >= 0) & (mk["xint"] <= c.n_levels - 1)).double() * dh
    if c.reparam is not None:
        dq = dq * 2 * mk["q"].clamp(min=REPARAM[0])
    tol_gd = (c.nsplit + 16) * P24 * grad_scale * dq * c.slabs.double().abs().sum(0)
    if c.reparam is not None:          # d(lb^2)/dlb = 2 q carries h's absolute rounding where q = (xint - zp) delta is the unclamped soft weight
        above = (mk["q"] >= REPARAM[0]).double()
        tol_gd = tol_gd + grad_scale * c.slabs.double().sum(0).abs() * 2 * (delta * 4 * h_err) * delta * dh * above
    u = (mk["h"] - 0.5).abs() * 2
    lg = torch.where(u > 0, torch.log2(u.clamp(min=1e-300)), torch.zeros_like(u))
    tol_gr = P24 * ref["g_round"].abs() * (16 + 2 * ((b - 1) * lg).abs())
    if on:          # |d g_round / d h| * 4 h_err  (u = 2 |h - 1/2|,  g_round = -+ rw b u^(b-1) 2 dh/dalpha)
        ub2 = torch.where(u > 0, u.clamp(min=1e-300) ** (b - 2), torch.zeros_like(u)) if b != 2.0 else torch.ones_like(u)
        tol_gr = tol_gr + ROUND_WEIGHT * b * (b - 1) * ub2 * 2 * 2 * dh * 4 * h_err
    tol_g = tol_gd + tol_gr
    m1, v1 = ref["m"], ref["v"]
    # |m|, |v|: the larger of the state that goes in and the state that comes out -- the roundings these terms stand for are those of
    # the products with the state that goes in and of the sum that comes out
    tol_m = 0.1 * tol_g + P24 * torch.maximum(m1.abs(), m_in.double().abs())
    tol_v = 0.001 * 2 * ref["g_total"].abs() * tol_g + 2 * P24 * torch.maximum(v1.abs(), v_in.double().abs())
    D = v1.sqrt() / bc2 + 1e-8
    dv = torch.where(v1 > 0, step * m1.abs() / D ** 2 * tol_v / (2 * v1.sqrt().clamp(min=1e-300) * bc2), torch.zeros_like(v1))
    tol_a = step / D * tol_m + dv + 2 * torch.maximum(_ulp32(c.alpha), _ulp32(ref["alpha"]))
    tol_wq = float(c.delta.max()) * 1e-4 + 0.3 * delta * tol_a
    if c.reparam is not None:
        tol_wq = tol_wq * 2 * (ref["wq"] + REPARAM[1]).clamp(min=0).sqrt()
    return dict(m=tol_m, v=tol_v, alpha=tol_a, wq=tol_wq)


def _kinks(c, ref):
    """Elements where the float64 reference sits on a kink of the chain: an fp32 evaluation may rightly take the other branch there."""
    mk = ref["masks"]
    hraw, h, xint = mk["hraw"], mk["h"], mk["xint"]
    zeros = torch.zeros_like(h, dtype=torch.bool)
    zeros.view(-1)[c.planted[:2]] = True                                      # the planted alpha = 0 (u = 0) must be compared
    k = (hraw.abs() < 1e-5) | ((hraw - 1).abs() < 1e-5) | (((h - 0.5).abs() < 1e-6) & ~zeros)
    k |= (hraw > 0) & (hraw < 1) & ((xint.abs() < 1e-3) | ((xint - (c.n_levels - 1)).abs() < 1e-3))
    if c.reparam is not None:
        k |= (mk["q"] - REPARAM[0]).abs() < 1e-6 * c.delta.view(c.bshape).double()
    return k


# ----------------------------------------------------------------------------------------------------------------- GPU side
def _sentinel(dtype):
    return -777.0 if dtype == torch.float32 else 0x5A5A


def _guarded(bufs, name, shape, dtype=torch.float32, init=None):
    """A tensor inside a larger buffer with GUARD sentinel elements on each side (ragged tiles store 16 bytes at a time)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), _sentinel(dtype), dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(shape)
    if init is not None:
        view.copy_(init)
    bufs[name] = buf
    return view


def guards_intact(item):
    for name, buf in item["_bufs"].items():
        s = _sentinel(buf.dtype)
        assert bool((buf[:GUARD] == s).all()) and bool((buf[-GUARD:] == s).all()), f"guard of {name} overwritten"


def make_item(c, state, *, conv_layout=True, planes=None, lin=False, dalpha=False):
    """Device tensors of one case as an item of ops.adaround_step_batch (also the arguments of the single-tensor entry).
    planes: None | 'bf16' (scale 0: three-way bf16 planes) | 'h2' (fp16 two-way planes at scale 4.0); lin: rdo_linear_h2 planes at 8.0."""
    from hipops import ops
    bufs = {}
    m, v = state_of(c, state)
    w = c.w.cuda()
    if c.layerwise:
        d = ops.ada_desc(w.view(1, -1), c.n_levels, conv_layout=False)
    else:
        d = ops.ada_desc(w, c.n_levels, reparam=c.reparam, conv_layout=conv_layout)
    has_wd = d.Cin > 0
    it = dict(d=d, w=w, delta=c.delta.cuda(), zp=c.zp.cuda(), slabs=c.slabs.cuda(), _bufs=bufs, _case=c,
              alpha=_guarded(bufs, "alpha", c.shape, init=c.alpha), m=_guarded(bufs, "m", c.shape, init=m),
              v=_guarded(bufs, "v", c.shape, init=v), wq=_guarded(bufs, "wq", c.shape),
              wd=_guarded(bufs, "wd", c.shape) if has_wd else None)
    n = c.w.numel()
    if planes == "bf16":
        it["wq_planes"] = _guarded(bufs, "wq_planes", (3, n), torch.int16)
        it["wd_planes"] = _guarded(bufs, "wd_planes", (3, n), torch.int16) if has_wd else None
    elif planes == "h2":
        it["wq_planes"] = ops.H2(_guarded(bufs, "wq_planes", (2, n), torch.int16), 4.0)
        it["wd_planes"] = ops.H2(_guarded(bufs, "wd_planes", (2, n), torch.int16), 4.0) if has_wd else None
    if lin:
        it["lin_fwd"] = ops.H2(_guarded(bufs, "lin_fwd", (2, n), torch.int16), 8.0)
        it["lin_bwd"] = ops.H2(_guarded(bufs, "lin_bwd", (2, n), torch.int16), 8.0)
    if dalpha:
        it["dalpha"] = _guarded(bufs, "dalpha", c.shape)
    return it


def _dev_sched(which="short"):
    return sched_table(which).cuda()


def _counter(k):
    return torch.full((1,), k, dtype=torch.int32, device="cuda")


def _log(which="short"):
    from hipops import _lib as L
    return torch.zeros(sched_table(which).shape[0], L.LOG_SLOTS, device="cuda")


def step_single(item, counter, grad_scale, which="short"):
    from hipops import ops
    log = _log(which)
    ops.adaround_step(item["d"], item["w"], item["delta"], item["zp"], item["slabs"], grad_scale, ROUND_WEIGHT, _dev_sched(which),
                      _counter(counter), item["alpha"], item["m"], item["v"], item["wq"], item["wd"], log, item.get("wq_planes"),
                      item.get("wd_planes"))
    torch.cuda.synchronize()
    return log


def step_batch(items, counter, grad_scale, which="short", **kw):
    from hipops import ops
    log = _log(which)
    ops.adaround_step_batch(items, grad_scale, ROUND_WEIGHT, _dev_sched(which), _counter(counter), log, **kw)
    torch.cuda.synchronize()
    return log


class w1_min:
    """`ada_w1_min` is process-wide: set for the block, restored whatever happens."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from hipops import ops
        self.prev = None if self.value is None else ops.set_tuning("ada_w1_min", self.value)

    def __exit__(self, *exc):
        from hipops import ops
        if self.prev is not None:
            ops.set_tuning("ada_w1_min", self.prev)
        return False


# name -> (case, entry, conv_layout, ada_w1_min or None): the entry and descriptor that reach the path named
PATHS = {
    "tile-ragged": ("A40x2x3x36", "batch", True, None),            # tile form, 2 x 2 ragged tiles, KH != KW, plain plane order
    "tile-frag": ("B48x3x3x48", "batch", True, None),              # tile form, ragged 32-tiles, 8 + 4 + 1 slab tree
    "tile-lin-a": ("C64x1x1x32", "batch", True, None),             # tile form with lin planes, 16 + 8 + 4 + 1 tree
    "tile-lin-b": ("C32x1x1x96", "batch", True, None),
    "w1-gamma": ("G36", "batch", False, None),                     # batch entry, one element per thread (nsplit 130 >= 128), reparam
    "tile-gamma-130": ("G36", "batch", True, 1 << 30),             # the same gamma on the tile form (8 x 16 + 2 slabs)
    "flat4-gamma-130": ("G36", "batch", False, 1 << 30),           # ... and on the batch entry's flat float4 form
    "tile-gamma-lin": ("G64", "batch", True, None),                # tile form + reparam + lin planes
    "flat4-straddle": ("F12x3x3x7", "single", True, None),         # single entry, float4 form, inner = 63: float4s straddle rows
    "flat4-inner2": ("S8x2", "single", False, None),               # single entry, inner < 4: fallback row division
    "scalar": ("H5x3x3x3", "single", True, None),                  # single entry, numel % 4 != 0: the scalar kernel
    "layerwise": ("L24x3x3x16", "single", False, None),            # single entry, one row of scales
}
COMBOS = [("first", 0, 1.0), ("mid", 2, 0.25), ("mid", 4, 1.0), ("first", 4, 0.25), ("mid", 0, 0.25)]
LIN_OK = ("C64x1x1x32", "C32x1x1x96", "G64")
FIGURES = {}


def run_path(path, state, counter, grad_scale, which="short", planes=None):
    name, entry, conv_layout, w1 = PATHS[path]
    c = case(name)
    item = make_item(c, state, conv_layout=conv_layout, planes=planes, lin=(entry == "batch" and conv_layout and name in LIN_OK))
    with w1_min(w1):
        log = step_single(item, counter, grad_scale, which) if entry == "single" else step_batch([item], counter, grad_scale, which)
    guards_intact(item)
    return item, log


@pytest.mark.parametrize("state,counter,grad_scale", COMBOS)
@pytest.mark.parametrize("path", list(PATHS))
def test_step_matches_float64(path, state, counter, grad_scale, which="short"):
    """adam_m, adam_v, alpha, wq and the log row of one step against float64, per-element bounds of the module docstring."""
    c = case(PATHS[path][0])
    ref = reference(c.name, state, counter, grad_scale, which)
    mk = ref["masks"]
    # the reference really exercises the masks
    pass_h = (mk["hraw"] >= 0) & (mk["hraw"] <= 1)
    pass_q = (mk["xint"] >= 0) & (mk["xint"] <= c.n_levels - 1)
    assert float((~pass_h).double().mean()) >= 0.10
    assert int((~pass_q).sum()) >= 1
    kink = _kinks(c, ref)
    if c.reparam is not None:          # ... and the LowerBound rule on both sides of ITS mask: 0 < q < bound, the gradient blocked and passed
        q, G = mk["q"].view(-1)[c.low], c.slabs.double().sum(0).view(-1)[c.low]
        assert bool(((q > 0) & (q < REPARAM[0])).all()) and not bool(kink.view(-1)[c.low].any()) and bool(pass_h.view(-1)[c.low].all())
        assert int((G > 0).sum()) >= 2 and int((G < 0).sum()) >= 2
        assert bool((ref["dalpha_data"].view(-1)[c.low][G > 0] == 0).all()) and bool((ref["dalpha_data"].view(-1)[c.low][G < 0] != 0).all())
    drawn = torch.ones_like(kink)
    drawn.view(-1)[c.planted] = False
    left_out = float((kink & drawn).sum()) / kink.numel()
    assert left_out <= 1e-3, f"{left_out:.2e} of the drawn elements sit on a kink: change the seed"
    assert bool(kink.view(-1)[c.planted[2:4]].all()) and not bool(kink.view(-1)[c.planted[:2]].any())

    item, log = run_path(path, state, counter, grad_scale, which)
    fp32 = restate_fp32(c, state, counter, grad_scale, which)
    h_err = float((fp32.pop("h").double() - mk["h"]).abs().max())
    tol = tolerances(c, ref, state, counter, grad_scale, which, h_err=h_err)
    keep = ~kink
    worst = {}
    for k in KEYS:
        got = item[k].cpu().double()
        assert bool(torch.isfinite(got).all()), f"{k}: non-finite output"
        err = (got - ref[k]).abs()
        worst[k] = float((err / tol[k].clamp(min=1e-300))[keep].max())
        if k in fp32:
            e32 = float((fp32[k].double() - ref[k]).abs()[keep].max())
            worst[k + "_vs_fp32"] = float(err[keep].max()) / e32 if e32 > 0 else 0.0
    FIGURES[(path, state, counter, grad_scale, which)] = dict(worst, left_out=left_out)
    print(f"\n[ada-step] {path} {state} it={counter} gs={grad_scale} left_out={left_out:.2e} " +
          " ".join(f"{k}={x:.3g}" for k, x in worst.items()))
    for k in KEYS:
        assert worst[k] <= 1.0, f"{k}: error is {worst[k]:.3g} x its bound"
    on = float(sched_table(which)[counter, 1])
    log = log.cpu().double()
    if on:
        want = float(ref["round_loss"])
        assert want > 0 and abs(float(log[counter].sum()) - want) <= 1e-5 * want
    assert float(log.abs().sum() - log[counter].abs().sum()) == 0.0 and (on or float(log.abs().sum()) == 0.0)      # every other row stays exactly 0


def test_step_matches_float64_fractional_b():
    """Row 6 of make_sched(30, 0.2, (20, 2)) has b = 19.25: a fractional exponent through pow_u on the tile form."""
    assert float(sched_table("long")[6, 0]) == 19.25
    test_step_matches_float64("tile-ragged", "mid", 6, 1.0, which="long")


def _outputs(item, keys=KEYS):
    return {k: item[k].clone() for k in keys if item.get(k) is not None}


@pytest.mark.parametrize("name", ["A40x2x3x36", "G36"])
def test_forms_agree_bit_for_bit(name):
    """The forms promise 'the same per-element summation order': the same inputs through the single-tensor entry (flat float4), the batch
    entry's tile form, its one-element-per-thread form (`ada_w1_min` = 1, a descriptor without conv layout -- so no wd) and, for the gamma,
    its flat float4 form (`ada_w1_min` = 1 << 30) leave identical alpha, m, v, wq and wd; the log rows agree in total."""
    c = case(name)
    counter, gs = 2, 0.25
    runs = {}
    it = make_item(c, "mid")
    runs["single"] = (it, step_single(it, counter, gs))
    it = make_item(c, "mid")
    runs["tile"] = (it, step_batch([it], counter, gs))
    it = make_item(c, "mid", conv_layout=False)
    with w1_min(1):
        runs["w1"] = (it, step_batch([it], counter, gs))
    if c.reparam is not None:
        it = make_item(c, "mid", conv_layout=False)
        with w1_min(1 << 30):
            runs["flat4-batch"] = (it, step_batch([it], counter, gs))
        it = make_item(c, "mid")
        with w1_min(1 << 30):
            runs["tile-w1-off"] = (it, step_batch([it], counter, gs))
    base, base_log = runs["single"]
    assert float(base_log[counter].sum()) > 0
    for form, (it, log) in runs.items():
        guards_intact(it)
        for k in KEYS + ("wd",):
            if it.get(k) is not None:
                assert torch.equal(it[k], base[k]), f"{form}: {k} differs from the single-tensor entry"
        torch.testing.assert_close(log.sum(1), base_log.sum(1), rtol=1e-6, atol=0)
    assert runs["tile"][0]["wd"] is not None and runs["w1"][0]["wd"] is None


def test_grad_then_apply_equals_fused():
    """Mode 1 into dalpha, dalpha doubled (exact), mode 2 with grad_scale 0.5 == mode 0 with grad_scale 1: a tile-form and a flat-form tensor
    in the same batch (the data-parallel path all-reduces dalpha between the two)."""
    names = ["A40x2x3x36", "F12x3x3x7"]
    counter = 2
    fused = [make_item(case(n), "mid") for n in names]
    log_f = step_batch(fused, counter, 1.0)
    split = [make_item(case(n), "mid", dalpha=True) for n in names]
    before = [_outputs(it, ("alpha", "m", "v")) for it in split]
    log_g = step_batch(split, counter, 1.0, mode=1)
    assert float(log_g.abs().sum()) == 0.0
    for it, b4 in zip(split, before):                        # the gradient pass writes dalpha and nothing else
        assert all(torch.equal(it[k], b4[k]) for k in b4) and bool((it["wq"] == _sentinel(torch.float32)).all())
        it["dalpha"].mul_(2.0)
    log_a = step_batch(split, counter, 0.5, mode=2)
    for a, b in zip(split, fused):
        guards_intact(a), guards_intact(b)
        for k in KEYS + ("wd",):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(log_a, log_f) and float(log_f[counter].sum()) > 0


@pytest.mark.parametrize("planes", ["bf16", "h2"])
@pytest.mark.parametrize("name", ["A40x2x3x36", "B48x3x3x48", "C64x1x1x32", "C32x1x1x96", "G36", "G64"])
def test_tile_form_layouts_equal_the_standalone_splits(name, planes):
    """Everything the tile form writes next to wq: the dgrad layout wd = wq.flip(1, 2).permute(3, 1, 2, 0) (a gamma's transpose), the planes
    of both in either format against the stand-alone split kernels, the rdo_linear_h2 planes of wq and of its transpose; no overflow word
    raised, no store outside a tensor (64 guard elements on each side of every output)."""
    from hipops import ops
    c = case(name)
    lin = name in LIN_OK
    ops.h2_overflow(reset=True)
    item = make_item(c, "mid", planes=planes, lin=lin)
    step_batch([item], 2, 0.25)
    guards_intact(item)
    assert not ops.h2_overflow(reset=True)
    co, ci = c.rows, c.shape[-1]
    kh, kw = (c.shape[1], c.shape[2]) if len(c.shape) == 4 else (1, 1)
    wq4 = item["wq"].reshape(co, kh, kw, ci)
    wd4 = item["wd"].reshape(ci, kh, kw, co)
    assert torch.equal(wd4, wq4.flip(1, 2).permute(3, 1, 2, 0).contiguous())
    if planes == "bf16":
        assert torch.equal(item["wq_planes"].reshape(3, -1), ops.split_bf16x3(wq4.contiguous()).reshape(3, -1))
        assert torch.equal(item["wd_planes"].reshape(3, -1), ops.split_bf16x3(wd4.contiguous()).reshape(3, -1))
    else:
        assert torch.equal(item["wq_planes"].t.reshape(2, -1), ops.split_h2_conv(wq4.contiguous(), scale=4.0).t.reshape(2, -1))
        assert torch.equal(item["wd_planes"].t.reshape(2, -1), ops.split_h2_conv(wd4.contiguous(), scale=4.0).t.reshape(2, -1))
    if lin:
        w2 = item["wq"].reshape(co, -1)
        assert torch.equal(item["lin_fwd"].t.reshape(2, -1), ops.split_h2_linear(w2.contiguous(), scale=8.0).t.reshape(2, -1))
        assert torch.equal(item["lin_bwd"].t.reshape(2, -1), ops.split_h2_linear(w2.t().contiguous(), scale=8.0).t.reshape(2, -1))
    assert not ops.h2_overflow(reset=True)


# one launch of eight items: tile, flat, one element per thread, tile with reparam, ..., a one-tile tensor first and last
MIXED = [("T16x1x1x16", True, False), ("F12x3x3x7", True, False), ("G36", False, False), ("G64", True, True), ("A40x2x3x36", True, False),
         ("S8x2", False, False), ("C64x1x1x32", True, True), ("T16x1x1x16", True, False)]


def _mixed_items():
    return [make_item(case(n), "mid", conv_layout=cl, lin=lin, planes="bf16" if k % 2 else "h2") for k, (n, cl, lin) in enumerate(MIXED)]


def test_batch_of_mixed_forms_equals_single_launches():
    """Eight tensors of every form in one launch leave what eight launches of one item each leave; `advance_iter` moves the counter by
    exactly 1, `iter_shadow` receives it + 1 and leaves the published word alone."""
    from hipops import ops
    counter, gs = 2, 0.25
    sched = _dev_sched()
    singles = _mixed_items()
    log_s = _log()
    for it in singles:
        ops.adaround_step_batch([it], gs, ROUND_WEIGHT, sched, _counter(counter), log_s)
    torch.cuda.synchronize()
    assert float(log_s[counter].sum()) > 0

    def same(items, log):
        for k, (a, b) in enumerate(zip(items, singles)):
            guards_intact(a)
            for key in KEYS + ("wd", "wq_planes", "wd_planes", "lin_fwd", "lin_bwd"):
                if b.get(key) is not None:
                    x, y = (a[key].t, b[key].t) if isinstance(b[key], ops.H2) else (a[key], b[key])
                    assert torch.equal(x, y), f"item {k} ({MIXED[k][0]}): {key}"
        torch.testing.assert_close(log.sum(1), log_s.sum(1), rtol=1e-6, atol=0)
        assert float(log.abs().sum() - log[counter].abs().sum()) == 0.0
    items, log, word = _mixed_items(), _log(), _counter(counter)
    ops.adaround_step_batch(items, gs, ROUND_WEIGHT, sched, word, log, advance_iter=word)
    torch.cuda.synchronize()
    assert word.tolist() == [counter + 1]
    same(items, log)
    items, log = _mixed_items(), _log()
    word = torch.tensor([-5, counter], dtype=torch.int32, device="cuda")             # [real counter, published copy]
    ops.adaround_step_batch(items, gs, ROUND_WEIGHT, sched, word[1:2], log, iter_shadow=word[0:1])
    torch.cuda.synchronize()
    assert word.tolist() == [counter + 1, counter]
    same(items, log)
