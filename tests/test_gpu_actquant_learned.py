"""Learned static activation ranges on the GPU: the backward kernel of the static quantiser against float64 (regions bit for bit, range
sums within the fp32 chain bound), `ActQuantStaticFn` in every layout, the projected Adam range step against float64, the range
gradients of a toy Cheng2020 unit against a float64 restatement, the learning loop (lower reconstruction error than its 'l2' start,
inside the max range, reproducible, exported, pickled), loss_mode='rd' through frozen quantisers, and two data-parallel ranks."""
import functools
import io
import os
import socket
import sys
import types

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(16384, 192), (35, 1280), (561, 3), (1, 6), (300000, 1)]


def _unaligned(x):
    """the same values behind a data pointer that is 4 bytes past a 16-byte boundary"""
    buf = torch.empty(x.numel() + 1, device=x.device, dtype=x.dtype)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _search_input(npix, C):
    """heavy-tailed, as `_search_input` of test_gpu_actquant_static.py (the constant channel only where there is a channel 1)"""
    g = torch.Generator().manual_seed(npix + C)
    z = torch.randn(npix, C, generator=g)
    x = z ** 3 * (0.25 + torch.arange(C) % 7) * 0.3
    x = torch.where(x < 0, x * 0.01, x)
    if C > 2:
        x[:, 1] = 0.75
    return x.float().contiguous()


@functools.lru_cache(maxsize=None)
def _case(npix, C):
    """(x, g, range) on the CPU, made once per shape: ranges at the 5 % / 95 % quantiles per channel; channel 1 constant (inside its
    range [0.5, 1]); channel 2 narrower than 1e-6.  A single pixel has no quantiles: its ranges are set by hand so that the six channels
    fall below, above and inside."""
    x = _search_input(npix, C)
    g = torch.randn(npix, C, generator=torch.Generator().manual_seed(7 * npix + C))
    if npix == 1:
        off = torch.tensor([1.0, -2.0, 0.5, -1.0, 3.0, -0.25])[:C]
        lo = x[0] + torch.where(off > 0, off, off * 2)                   # below: channels 0, 2, 4 (lo = x + 1 | 0.5 | 3)
        hi = lo + torch.tensor([1.0, 1.0, 5e-7, 4.0, 2.0, 0.375])[:C]    # above: channels 1, 5 (hi = x - 3 | - 0.125); inside: channel 3
    else:
        q = torch.quantile(x.double(), torch.tensor([0.05, 0.95], dtype=torch.float64), dim=0).float()
        lo, hi = q[0].clone(), q[1].clone()
        if C > 2:
            lo[1], hi[1] = 0.5, 1.0
            lo[2] = x[:, 2].median()
            hi[2] = lo[2] + 5e-7
            assert float(hi[2] - lo[2]) < 1e-6
    return x, g, torch.cat([lo, hi]).contiguous()


def _bwd_ref64(x, g, rng, y):
    """float64 restatement: the region from the same fp32 comparisons, y from the product's forward, terms and sums in float64.
    -> (dx, drange, sum |g term| per entry)"""
    C = x.shape[-1]
    lo, hi = rng[:C], rng[C:]
    below, above = x < lo, x > hi
    r = torch.clamp(hi - lo, min=1e-6).double()
    xd, yd, gd = x.double(), y.double(), g.double()
    one, zero = torch.ones_like(xd), torch.zeros_like(xd)
    tl = torch.where(below, one, torch.where(above, zero, (xd - yd) / r))
    th = torch.where(above, one, torch.where(below, zero, (yd - xd) / r))
    wide = (~((hi - lo) < 1e-6)).double()
    flat = lambda t: t.reshape(-1, C)
    dr = torch.cat([flat(gd * tl).sum(0) * wide, flat(gd * th).sum(0) * wide])
    mass = torch.cat([flat(gd * tl).abs().sum(0) * wide, flat(gd * th).abs().sum(0) * wide])
    return torch.where(below | above, torch.zeros_like(g), g), dr, mass, (below, above)


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("n_bits", [4, 8, 16])
@pytest.mark.parametrize("npix,C", SHAPES)
def test_backward_kernel_against_float64(npix, C, n_bits):
    """dx: bit for bit (no division in the region decision).  drange: |got - ref| <= 1e-4 sum |g term| per entry -- an fp32 sum whose serial
    chains hold at most 1024 terms, plus the tree, is within about (1024 + 20) 2^-24 = 6.2e-5 of the exact sum relative to the sum of the
    absolute terms (the terms are signed), the bound of test_search_sums_match_float64; the two roundings of a term itself add 1.2e-7.
    (With 256 workgroups of 256 lanes, 300000 pixels of one channel are 5 per thread: the chains of this thread map close at 1024 terms
    only beyond 67 M pixels per channel group, which no test here allocates.)  A single pixel cannot hold ten elements per region."""
    from hipops import ops
    x, g, rng = _case(npix, C)
    xc, gc, rc = x.cuda(), g.cuda(), rng.cuda()
    y = ops.actquant_static(xc, rc, n_bits=n_bits).cpu()
    dx_ref, dr_ref, mass, (below, above) = _bwd_ref64(x, g, rng, y)
    need = 10 if npix > 1 else 1
    assert int(below.sum()) >= need and int(above.sum()) >= need and int((~(below | above)).sum()) >= need
    bound = 1e-4 * mass

    def run(xs, gs, dx=None):
        dr = torch.zeros(2 * C, device="cuda")
        out = ops.actquant_static_bwd(xs, gs, rc, dr, dx=dx, n_bits=n_bits)
        return out, dr
    dx, dr = run(xc, gc)
    assert torch.equal(dx.cpu(), dx_ref)
    err = (dr.cpu().double() - dr_ref).abs()
    print(f"bwd npix={npix} C={C} n_bits={n_bits}: worst |err| / sum|g term| = {float((err / mass.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= bound).all())
    if C > 2 and npix > 1:
        assert float(dr[2]) == 0.0 and float(dr[C + 2]) == 0.0          # the degenerate channel: exactly nothing
        assert float(mass[0]) > 0
    dx2, dr2 = run(xc, gc)
    assert torch.equal(dx2, dx) and torch.equal(dr2, dr)                 # fixed reduction order
    dxu, dru = run(_unaligned(xc), _unaligned(gc), dx=_unaligned(torch.empty_like(xc)))      # 4 bytes past a 16-byte boundary
    assert torch.equal(dxu.cpu(), dx_ref) and bool(((dru.cpu().double() - dr_ref).abs() <= bound).all())
    gi = gc.clone()
    dxi, dri = run(xc, gi, dx=gi)                                        # in place
    assert dxi is gi and torch.equal(gi, dx) and torch.equal(dri, dr)
    if npix > 1:                                                         # two calls on an uneven split accumulate
        cut = (npix * 3) // 8 + 1
        two = torch.zeros(2 * C, device="cuda")
        a = ops.actquant_static_bwd(xc[:cut].contiguous(), gc[:cut].contiguous(), rc, two, n_bits=n_bits)
        b = ops.actquant_static_bwd(xc[cut:].contiguous(), gc[cut:].contiguous(), rc, two, n_bits=n_bits)
        assert torch.equal(torch.cat([a, b]), dx)
        assert bool(((two.cpu().double() - dr_ref).abs() <= bound).all())
    with pytest.raises(ValueError):
        ops.actquant_static_bwd(xc, gc, torch.zeros(2 * (C + 1), device="cuda"), torch.zeros(2 * C, device="cuda"), n_bits=n_bits)


def test_backward_closes_long_chains():
    """More than 1024 pixels per thread (one channel: all 256 lanes of all 256 workgroups walk the pixels), as test_search_closes_long_chains:
    the running sums are closed every 1024 terms.  The float64 reference is evaluated by torch on the device (67.5 M values and their
    float64 temporaries, a few GB of device memory for the duration of the test)."""
    from hipops import ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    npix = 256 * 256 * 1030
    x = (torch.rand(npix, 1, generator=gen, device="cuda") ** 2).contiguous()
    g = torch.randn(npix, 1, generator=gen, device="cuda")
    rng = torch.tensor([0.04, 0.7], device="cuda")
    y = ops.actquant_static(x, rng, n_bits=8)
    dx_ref, dr_ref, mass, (below, above) = _bwd_ref64(x, g, rng, y)
    del y
    dr = torch.zeros(2, device="cuda")
    dx = ops.actquant_static_bwd(x, g, rng, dr, n_bits=8)
    assert torch.equal(dx, dx_ref) and int(below.sum()) > 10 and int(above.sum()) > 10
    err = (dr.double() - dr_ref).abs()
    print(f"bwd {npix} x 1: worst |err| / sum|g term| = {float((err / mass).max()):.3e}")
    assert bool((err <= 1e-4 * mass).all())


# ----------------------------------------------------------------------------- the Function's layouts
class _SteRows(torch.autograd.Function):
    """torch-CPU restatement in float64 on channels-last rows; y is handed in (the product's own forward, tested on its own)."""

    @staticmethod
    def forward(ctx, x, rng, y):
        ctx.save_for_backward(x, rng, y)
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        x, rng, y = ctx.saved_tensors
        C = x.shape[-1]
        lo, hi = rng[:C], rng[C:]
        below, above = x < lo, x > hi
        r = torch.clamp(hi - lo, min=1e-6)
        tl = torch.where(below, torch.ones_like(x), torch.where(above, torch.zeros_like(x), (x - y) / r))
        th = torch.where(above, torch.ones_like(x), torch.where(below, torch.zeros_like(x), (y - x) / r))
        _SteRows.mass = torch.cat([(g * tl).reshape(-1, C).abs().sum(0), (g * th).reshape(-1, C).abs().sum(0)])
        return torch.where(below | above, torch.zeros_like(g), g), torch.cat([(g * tl).reshape(-1, C).sum(0), (g * th).reshape(-1, C).sum(0)]), None


@pytest.mark.parametrize("view,channels_last", [((2, 12, 6, 7), False), ((2, 72, 7), False), ((84, 12), False), ((2, 12, 6, 7), True)])
def test_function_layouts(view, channels_last):
    from hipops.autograd import ActQuantStaticFn
    gen = torch.Generator().manual_seed(31)
    base = torch.randn(2, 12, 6, 7, generator=gen) * 2
    up = torch.randn(2, 12, 6, 7, generator=gen)
    x = base.reshape(view).clone()
    to_rows = (lambda t: t.permute(0, 2, 3, 1)) if (x.dim() == 4 and not channels_last) else (lambda t: t)
    C = to_rows(x).shape[-1]
    rows = to_rows(x).reshape(-1, C)
    rng = torch.cat([rows.quantile(0.1, dim=0), rows.quantile(0.9, dim=0)]).contiguous()
    xg, rg = x.cuda().requires_grad_(True), rng.cuda().requires_grad_(True)
    out = ActQuantStaticFn.apply(xg, rg, 8, channels_last)
    assert out.shape == x.shape
    w = up.reshape(view)
    gx, gr = torch.autograd.grad((out * w.cuda()).sum(), [xg, rg])
    x64 = x.double().requires_grad_(True)
    r64 = rng.double().requires_grad_(True)
    ref = _SteRows.apply(to_rows(x64), r64, to_rows(out.detach().cpu().double()))
    rx, rr = torch.autograd.grad((ref * to_rows(w.double())).sum(), [x64, r64])
    assert gx.shape == x.shape and torch.equal(gx.cpu().double(), rx)
    assert int((rx == 0).sum()) >= 10 and int((rx != 0).sum()) >= 10
    assert bool(((gr.cpu().double() - rr).abs() <= 1e-4 * _SteRows.mass).all())


# ----------------------------------------------------------------------------- the range step
def _step_ref64(rng, grad, obs, m, v, step, lr):
    C = rng.numel() // 2
    w = (obs[C:] - obs[:C]).repeat(2)
    m = 0.9 * m + 0.1 * grad
    v = 0.999 * v + 0.001 * grad * grad
    new = rng - lr * w * (m / (1 - 0.9 ** step)) / ((v / (1 - 0.999 ** step)).sqrt() + 1e-8)
    lo0, hi0, gap = obs[:C], obs[C:], 1e-3 * (obs[C:] - obs[:C])
    hit = dict(lo=(new[:C] < lo0) | (new[:C] > hi0), hi=(new[C:] < lo0) | (new[C:] > hi0))
    lo, hi = torch.minimum(torch.maximum(new[:C], lo0), hi0), torch.minimum(torch.maximum(new[C:], lo0), hi0)
    hit["width"] = hi < lo + gap
    hi = torch.minimum(torch.maximum(hi, lo + gap), hi0)
    lo = torch.maximum(torch.minimum(lo, hi - gap), lo0)
    return torch.cat([lo, hi]), m, v, hit


def test_range_step_against_float64_and_its_projections():
    from hipops import ops
    C, lr = 7, 1e-3
    lo0 = torch.tensor([-1.0, -2.0, 0.0, 0.5, -3.0, -0.25, 1.0])
    hi0 = torch.tensor([1.0, 3.0, 4.0, 2.5, -1.0, 0.75, 9.0])
    w = hi0 - lo0
    mid = (lo0 + hi0) / 2
    lo, hi = lo0 + 0.2 * w, hi0 - 0.2 * w
    lo[0] = lo0[0]                                   # channel 0: lo sits on the observed minimum and is pushed down
    hi[1] = hi0[1]                                   # channel 1: hi sits on the observed maximum and is pushed up
    lo[2], hi[2] = mid[2] - 0.6e-3 * w[2], mid[2] + 0.6e-3 * w[2]        # channel 2: the ends are pushed through each other
    lo[3], hi[3] = hi0[3] - 1.1e-3 * w[3], hi0[3]    # channel 3: lo is pushed up against a hi that cannot give way
    obs = torch.cat([lo0, hi0])
    rng = torch.cat([lo, hi])
    gen = torch.Generator().manual_seed(3)
    grads = [torch.randn(2 * C, generator=gen) for _ in range(5)]
    for g in grads:
        g[0], g[C + 1] = abs(g[0]) + 0.1, -abs(g[C + 1]) - 0.1
        g[2], g[C + 2] = -abs(g[2]) - 0.1, abs(g[C + 2]) + 0.1
        g[3] = -abs(g[3]) - 0.1
    dev = [t.clone().cuda() for t in (rng, obs, torch.zeros(2 * C), torch.zeros(2 * C))]
    r64, m64, v64 = rng.double(), torch.zeros(2 * C, dtype=torch.float64), torch.zeros(2 * C, dtype=torch.float64)
    hits = dict(lo=torch.zeros(C, dtype=torch.bool), hi=torch.zeros(C, dtype=torch.bool), width=torch.zeros(C, dtype=torch.bool))
    for step, g in enumerate(grads, 1):
        ops.act_range_step(dev[0], g.cuda(), dev[1], dev[2], dev[3], step, lr)
        r64, m64, v64, hit = _step_ref64(r64, g.double(), obs.double(), m64, v64, step, lr)
        for k in hits:
            hits[k] |= hit[k]
        got = dev[0].cpu()
        torch.testing.assert_close(got.double(), r64, rtol=1e-6, atol=1e-9)
        # (m is a signed sum: its rounding error scales with its terms 0.1 g, not with what is left after they cancel)
        torch.testing.assert_close(dev[2].cpu().double(), m64, rtol=1e-6, atol=1e-7 * float(torch.stack(grads).abs().max()))
        torch.testing.assert_close(dev[3].cpu().double(), v64, rtol=1e-6, atol=1e-12)
        assert bool((got[:C] >= lo0).all()) and bool((got[C:] <= hi0).all()) and bool((got[C:] > got[:C]).all())
        assert float(got[0]) == float(lo0[0]) and float(got[C + 1]) == float(hi0[1]) and float(got[C + 3]) == float(hi0[3])
    assert bool(hits["lo"][0]) and bool(hits["hi"][1]) and bool(hits["width"][2]) and bool(hits["width"][3])
    with pytest.raises(ValueError):
        ops.act_range_step(dev[0], grads[0][:-2].cuda(), dev[1], dev[2], dev[3], 1, lr)
    with pytest.raises(RuntimeError):
        ops.act_range_step(dev[0], grads[0].cuda(), dev[1], dev[2], dev[3], 0, lr)


# ----------------------------------------------------------------------------- a toy Cheng2020 unit
BITS, N, B, LEARN_ITERS = 4, 16, 4, 200


def _toy_model(n_ch, bits, n_img, **extra):
    import lic
    from quantization import QuantModel
    torch.manual_seed(1005)
    model = lic.Cheng2020Anchor(N=n_ch).cuda().eval()
    g = torch.Generator().manual_seed(13)
    cali = torch.rand(n_img, 3, 64, 64, generator=g).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    if bits != 8:
        aq["dynamic_bits"] = bits
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq, is_cheng=True).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:2])
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Cheng2020", **extra)
    kwargs = dict(cali_data=cali, batch_size=B, iters=6, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2),
                  warmup=0.2, act_quant=True, opt_mode="mse", config=None, args=args)
    qnn.set_quant_state(True, True)
    qnn.model.g_s[-1][0].set_quant_state(True, False)
    return qnn, cali, kwargs


def _quant_mods(unit):
    from quantization import BaseQuantBlock, QuantModule
    return [m for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]


def _flags(unit):
    return [(m.use_weight_quant, m.use_act_quant, m.trained, getattr(m.act_quantizer, "act_ste", False), m.act_quantizer.act_phase,
             sorted(getattr(m.act_quantizer, "act_obs", {}))) for m in _quant_mods(unit)]


def _ranges(unit):
    return {(i, k): r.detach().clone() for i, m in enumerate(_quant_mods(unit)) for k, r in sorted(m.act_quantizer.act_range.items())}


def _set_ranges(unit, ranges):
    for i, m in enumerate(_quant_mods(unit)):
        m.act_quantizer.act_range = {k: r.clone() for (j, k), r in ranges.items() if j == i}


def _w8a8_error(unit, inp_q, out_fp):
    """lp_loss(unit(inp_q), out_fp, p=2) of the unit in the W8A8 state over the whole cache, summed in float64"""
    mods = _quant_mods(unit)
    keep = [(m.use_weight_quant, m.use_act_quant) for m in mods]
    try:
        for m in mods:
            m.use_weight_quant = m.use_act_quant = True
        with torch.no_grad():
            out = unit(inp_q)
    finally:
        for m, (w_, a_) in zip(mods, keep):
            m.use_weight_quant, m.use_act_quant = w_, a_
    return float(((out.double() - out_fp.double()) ** 2).sum(1).mean())


@pytest.fixture(scope="module")
def learned():
    """g_a[3] of a toy Cheng2020 (N = 16; a ResidualBlock on 16^2 inputs of 8 images of 64^2), activation grid of 4 bits, calibrated through
    block_reconstruction with act_range='learned' (200 range steps); then the same two steps by hand on the trained unit: the 'l2'
    starting ranges, and a second learning run."""
    from quantization import block_reconstruction
    from quantization.recon import calibrate_act_ranges, learn_act_ranges, unit_seed
    from quantization.utils import save_inp_oup_data
    qnn, cali, kwargs = _toy_model(N, BITS, 8, act_mode="static", act_range="learned", act_iters=LEARN_ITERS)
    unit = qnn.model.g_a[3]
    assert unit.unit_kind == "rb"
    (inp_q, _), out_fp = save_inp_oup_data(qnn, unit, cali, asym=True, act_quant=True, batch_size=8, input_prob=True)
    assert tuple(inp_q.shape) == (8, N, 16, 16)
    inp_q, out_fp = inp_q.clone(), out_fp.clone()
    block_reconstruction(qnn, unit, "3", **kwargs)
    first = _ranges(unit)
    calibrate_act_ranges(unit, inp_q, "max", batch=8)
    mx = _ranges(unit)
    calibrate_act_ranges(unit, inp_q, "l2", batch=8, keep_obs=True)
    l2 = _ranges(unit)
    flags = _flags(unit)
    learn_act_ranges(unit, inp_q, out_fp, LEARN_ITERS, 1e-3, B, seed=unit_seed("3"))
    flags_after = _flags(unit)
    return dict(qnn=qnn, unit=unit, inp_q=inp_q, out_fp=out_fp, first=first, second=_ranges(unit), l2=l2, mx=mx, flags=flags,
                flags_after=flags_after)


def test_learning_loop_lowers_the_reconstruction_error(learned):
    from quantization.export import activation_state
    t = learned
    unit, first, l2, mx = t["unit"], t["first"], t["l2"], t["mx"]
    assert sorted(first) == sorted(l2) == sorted(mx) and len(first) == 3            # the block's three quantisation points
    _set_ranges(unit, l2)
    e_l2 = _w8a8_error(unit, t["inp_q"], t["out_fp"])
    _set_ranges(unit, first)
    e_learned = _w8a8_error(unit, t["inp_q"], t["out_fp"])
    moved = max(float((first[k] - l2[k]).abs().max()) for k in first)
    print(f"W{8}A{BITS} reconstruction error of the unit: l2 ranges {e_l2:.6e}, learned ranges {e_learned:.6e}; largest move of an end {moved:.4f}")
    assert e_learned < e_l2
    for k, r in first.items():
        c = r.numel() // 2
        assert bool((r[:c] >= mx[k][:c]).all()) and bool((r[c:] <= mx[k][c:]).all()) and bool((r[c:] > r[:c]).all())
    # a second run (the same two steps on the trained unit) gives the same bits
    assert all(torch.equal(first[k], t["second"][k]) for k in first)
    # the state flags are as they were found; nothing of the learning phase is left on the quantisers
    before = [f[:5] for f in t["flags"]]
    assert [f[:5] for f in t["flags_after"]] == before and all(f[3] is False and f[5] == [] for f in t["flags_after"])
    q = unit.act_quantizer
    assert q.act_frozen() and not any(r.requires_grad for r in q.act_range.values())
    # a learned range is a frozen range: exported, pickled and moved like one
    qnn = t["qnn"]
    name = next(n for n, qq in qnn.act_quantizers() if qq is q)
    st = activation_state(qnn)
    for s, key in ((0, name), (1, name + "#1"), (2, name + "#2")):
        r = first[(0, s)].cpu()
        assert st[key]["n_bits"] == BITS and torch.equal(st[key]["lo"], r[:N]) and torch.equal(st[key]["hi"], r[N:])
    buf = io.BytesIO()
    torch.save(qnn, buf)
    buf.seek(0)
    qnn2 = torch.load(buf, weights_only=False)
    q2 = qnn2.model.g_a[3].act_quantizer
    assert q2.act_frozen() and all(torch.equal(q2.act_range[s], first[(0, s)]) for s in (0, 1, 2)) and q2.act_ste is False
    qnn2.cpu()
    assert all(not q2.act_range[s].is_cuda and torch.equal(q2.act_range[s], first[(0, s)].cpu()) for s in (0, 1, 2))


class _Ste(torch.autograd.Function):
    """the static quantiser with the straight-through backward on an NCHW tensor, in the dtype it is given (CPU)"""

    @staticmethod
    def forward(ctx, x, rng, n_bits, sink, tag):
        C = x.shape[1]
        lo, hi = rng[:C].view(1, C, 1, 1), rng[C:].view(1, C, 1, 1)
        r = torch.clamp(hi - lo, min=1e-6)
        R = float(2 ** n_bits - 1)
        y = torch.round(torch.clamp((x - lo) / r, 0, 1) * R) / R * r + lo
        ctx.save_for_backward(x, y, lo, hi, r)
        ctx.sink, ctx.tag = sink, tag
        return y

    @staticmethod
    def backward(ctx, g):
        x, y, lo, hi, r = ctx.saved_tensors
        below, above = x < lo, x > hi
        one, zero = torch.ones_like(x), torch.zeros_like(x)
        tl = torch.where(below, one, torch.where(above, zero, (x - y) / r))
        th = torch.where(above, one, torch.where(below, zero, (y - x) / r))
        wide = (~((hi - lo) < 1e-6)).to(x.dtype).view(-1)
        ctx.sink[ctx.tag] = torch.cat([(g * tl).abs().sum((0, 2, 3)) * wide, (g * th).abs().sum((0, 2, 3)) * wide])
        return (torch.where(below | above, zero, g), torch.cat([(g * tl).sum((0, 2, 3)) * wide, (g * th).sum((0, 2, 3)) * wide]),
                None, None, None)


def _restated_range_grads(unit, x, tgt, ranges, dtype):
    """QuantRB.forward in the W8A8 state from the oracle's modules (QOp on the unit's effective, hard-rounded weights) with `_Ste` at the
    block's three quantisation points, lp_loss(out, tgt, p=2), gradients to the three ranges -- on the CPU in `dtype`."""
    from oracle import rdo_oracle as O
    ops = {}
    for n in ("conv1", "conv2"):
        m = getattr(unit, n)
        w_, b_ = m._weights()
        ops[n] = O.QOp("conv", w_.detach().cpu().to(dtype), b_.detach().cpu().to(dtype), stride=1, padding=1)
    assert unit.skip is None
    rs = [ranges[k].cpu().to(dtype).requires_grad_(True) for k in sorted(ranges)]
    sink = {}
    x = x.cpu().to(dtype)
    out = _Ste.apply(F.leaky_relu(ops["conv1"](x), 0.01), rs[0], BITS, sink, 0)
    out = _Ste.apply(F.leaky_relu(ops["conv2"](out), 0.01), rs[1], BITS, sink, 1)
    out = _Ste.apply(out + x, rs[2], BITS, sink, 2)
    loss = O.lp_loss(out, tgt.cpu().to(dtype), p=2)
    return [g_.double() for g_ in torch.autograd.grad(loss, rs)], [sink[i].double() for i in range(3)]


def test_first_iteration_range_gradients_of_a_unit(learned):
    """The product's tape (split-precision convolutions, HIP backward) against the float64 restatement, per quantisation point in the
    largest-entry norm: at most 5 x the distance of the SAME restatement run in fp32, plus 1e-6 of the largest sum |g term| of the point
    -- the margin test_gpu_nic_fullsize.py gives split-fp16 arithmetic against fp32.  Per point and not per entry: on a 4-bit grid a last-bit
    difference upstream moves single elements to the neighbouring level, which lands on whichever channels those elements are in."""
    from hipops.autograd import SqDiffSumFn
    t = learned
    unit, l2 = t["unit"], t["l2"]
    x, tgt = t["inp_q"][:B].contiguous(), t["out_fp"][:B].contiguous()
    _set_ranges(unit, l2)
    mods = _quant_mods(unit)
    keep = [(m.use_weight_quant, m.use_act_quant) for m in mods]
    q = unit.act_quantizer
    try:
        for m in mods:
            m.use_weight_quant = m.use_act_quant = True
        q.act_learn()
        xs = x.detach().requires_grad_(True)
        out = unit(xs)
        loss = SqDiffSumFn.apply(out, tgt, float(out.shape[1]) / out.numel())
        got = torch.autograd.grad(loss, [q.act_range[s] for s in (0, 1, 2)])
        got = [g_.cpu().double() for g_ in got]
    finally:
        q.act_freeze()
        for m, (w_, a_) in zip(mods, keep):
            m.use_weight_quant, m.use_act_quant = w_, a_
    ranges = {s: l2[(0, s)] for s in (0, 1, 2)}
    ref64, mass = _restated_range_grads(unit, x, tgt, ranges, torch.float64)
    ref32, _ = _restated_range_grads(unit, x, tgt, ranges, torch.float32)
    ok = True
    for s in (0, 1, 2):
        d32 = float((ref32[s] - ref64[s]).abs().max())
        dp_ = float((got[s] - ref64[s]).abs().max())
        allowed = 5 * d32 + 1e-6 * float(mass[s].max())
        print(f"site {s}: |fp32 restatement - fp64| = {d32:.3e}, |product - fp64| = {dp_:.3e}, allowed {allowed:.3e}, "
              f"largest |gradient| {float(ref64[s].abs().max()):.3e}")
        ok = ok and dp_ <= allowed
        assert float(ref64[s].abs().max()) > 0
    assert ok


# ----------------------------------------------------------------------------- loss_mode='rd' behind frozen quantisers
def test_rd_task_loss_through_frozen_activation_quantisers():
    """The toy flow of test_main2_flow_with_static_activation_ranges (first pass: every unit, W8A8, static), then a second pass over one
    unit with loss_mode='rd': the task gradient now comes back through the frozen quantisers of the trained modules behind it."""
    import torch.nn as nn
    from quantization import BaseQuantBlock, QuantModule, block_reconstruction, layer_reconstruction
    from quantization.recon import reconstruct
    qnn, cali, kwargs = _toy_model(8, 8, 4, act_mode="static")
    kwargs["batch_size"] = 2

    def walk(m: nn.Module):
        for name, module in m.named_children():
            if isinstance(module, QuantModule):
                layer_reconstruction(qnn, module, name, **kwargs)
            elif isinstance(module, BaseQuantBlock):
                block_reconstruction(qnn, module, name, **kwargs)
            else:
                walk(module)
    walk(qnn)
    quants = [m.act_quantizer for m in qnn.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    assert sum(q.act_frozen() for q in quants) >= 20
    qnn.set_quant_state(True, True)
    qnn.model.g_s[-1][0].set_quant_state(True, False)
    unit = qnn.model.g_a[1]
    rd = dict(kwargs, iters=3, args=types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Cheng2020", act_mode="static", loss_mode="rd"))
    eng = reconstruct(qnn, unit, "1", is_block=True, **rd)
    torch.cuda.synchronize()
    assert eng.rd is not None
    g_task = eng.g_task.cpu()
    print(f"rd behind frozen quantisers: |g_task| max {float(g_task.abs().max()):.3e}, task loss {eng.logs_terms()[1].tolist()}")
    assert bool(torch.isfinite(g_task).all()) and float(g_task.abs().max()) > 0
    assert not any(getattr(q, "act_ste", False) for q in quants) and unit.act_quantizer.act_frozen()
    rd["args"].act_mode = "dynamic"
    with pytest.raises(RuntimeError, match="no gradient reached"):
        reconstruct(qnn, unit, "1", is_block=True, **rd)
    assert not any(getattr(q, "act_ste", False) for q in quants)


# ----------------------------------------------------------------------------- two ranks on one GPU
DP_ITERS = 8


def _dp_unit():
    """a trained ResidualBlock unit (N = 16, nearest-rounded 8-bit weights, 4-bit static activation grid), 8 inputs of 16^2 and its
    full-precision outputs: the same on every rank"""
    import lic
    from helpers import WQ
    from quantization.quant_block import QuantRB
    torch.manual_seed(77)
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False, "dynamic_bits": BITS, "act_mode": "static"}
    unit = QuantRB(lic.ResidualBlock(N, N), WQ, aq).cuda().eval()
    x = torch.randn(8, N, 16, 16, generator=torch.Generator().manual_seed(78)).cuda()
    unit.set_quant_state(False, False)
    with torch.no_grad():
        out_fp = unit(x).clone()
    for m in _quant_mods(unit):
        m.trained = True
    return unit, x, out_fp


def _dp_idx():
    return torch.tensor([[i % 4, 4 + (3 * i) % 4] for i in range(DP_ITERS)])       # one image from each rank's shard


def _dp_learn(unit, x, out_fp, idx, batch):
    from quantization.recon import calibrate_act_ranges, learn_act_ranges
    calibrate_act_ranges(unit, x, "l2", batch=4, keep_obs=True)
    obs = {k: r.clone() for k, r in unit.act_quantizer.act_obs.items()}
    learn_act_ranges(unit, x, out_fp, DP_ITERS, 1e-3, batch, idx_table=idx)
    return {k: r.cpu() for k, r in unit.act_quantizer.act_range.items()}, {k: r.cpu() for k, r in obs.items()}


def _dp_rank(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "rdo-ptq_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from quantization import dp
        unit, x, out_fp = _dp_unit()
        lo, hi = dp.shard_range(x.shape[0], rank, world)
        got, _ = _dp_learn(unit, x[lo:hi].contiguous(), out_fp[lo:hi].contiguous(), _dp_idx()[:, rank:rank + 1] - lo, 1)
        out_q.put((rank, got))
        dist.barrier()
    except BaseException as e:          # the parent must not wait out its queue timeout for a rank that failed
        out_q.put(("error", f"rank {rank}: {e!r}"))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_learn_the_same_ranges_as_one():
    """Two processes on cuda:0 over gloo (as test_gpu_dp_engine.py): each learns on its half of the cache with its row of the global
    mini-batch; the mean of the ranks' range gradients is the gradient of the global mini-batch."""
    unit, x, out_fp = _dp_unit()
    ref, obs = _dp_learn(unit, x, out_fp, _dp_idx(), 2)
    assert sorted(ref) == [0, 1, 2]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(2):
            rk, val = q.get(timeout=180)
            assert rk != "error", val
            got[rk] = val
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    for k in ref:
        assert torch.equal(got[0][k], got[1][k])                          # every rank holds the same grid, bit for bit
        w = (obs[k][N:] - obs[k][:N]).repeat(2)
        worst = float(((got[0][k] - ref[k]).abs() / w).max())
        print(f"site {k}: two ranks against one, largest difference {worst:.3e} of the observed width")
        assert bool(((got[0][k] - ref[k]).abs() <= 1e-5 * w).all())
        assert float((ref[k] - unit.act_quantizer.act_range[k].cpu()).abs().max()) == 0
