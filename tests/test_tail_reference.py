"""tests/tail_reference.py against float64 autograd of the oracle (oracle/rdo_oracle.py: lp_loss, f_gdn), so that the reference the GPU
parity tests compare with is itself pinned from outside.  Also the admission check of the GDN bounds: for the inputs the GPU test uses,
the fp32 chain run on the CPU stays within 0.75 of `gdn_bounds` (so a GPU result outside them is a finding, not noise)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_reference as R
from oracle import rdo_oracle as O

U = R.U
nchw = lambda t: t.permute(0, 3, 1, 2)


def _within(got, ref, bound):
    err = (got.double() - ref.double()).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


def _case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    pre = torch.randn(*shape, generator=g)
    res = torch.randn(*shape, generator=g)
    tgt = torch.randn(R.N_TARGETS, *shape[1:], generator=g)
    return pre, res, tgt, R.idx_table(B)


@pytest.mark.parametrize("it", [0, 2])
def test_lp2_emulation_matches_autograd(it):
    shape, coef = (3, 5, 7, 12), 0.75
    pred, _, tgt, idx = _case(shape, 1)
    y = R.rows(tgt, idx, it, 3)
    pred.view(-1)[[0, 17, 1259]] = y.reshape(-1)[[0, 17, 1259]]
    pr = pred.double().requires_grad_(True)
    loss = coef * O.lp_loss(nchw(pr), nchw(y.double()), p=2.0)
    loss.backward()
    grad, d = R.lp2(pred, tgt, idx, it, coef)
    # d = fl(pred - y) carries u relative to the exact difference, gs two products and the rounded 1 / npix: 5u of the gradient
    _within(grad, pr.grad, 6 * U * pr.grad.abs())
    assert bool((grad.view(-1)[[0, 17, 1259]] == 0).all())
    assert abs(R.loss64(d, coef, 3, 35) - float(loss.detach())) <= 4 * U * float(loss.detach())


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_res", [False, True])
def test_loss_act_emulation_matches_autograd(act, with_res):
    shape, coef, it = (3, 5, 7, 16), 2.0, 2
    pre, res, tgt, idx = _case(shape, 2 + act)
    pre.view(-1)[[3, 40]] = torch.tensor([0.0, -0.0])
    res = res if with_res else None
    y = R.rows(tgt, idx, it, 3).double()
    p64 = pre.double().requires_grad_(True)
    a = p64 if act == 0 else (F.leaky_relu(p64, 0.01) if act == 1 else F.relu(p64))
    o64 = (a + res.double()) if with_res else a + 0.0
    o64.retain_grad()
    loss = coef * O.lp_loss(nchw(o64), nchw(y), p=2.0)
    loss.backward()
    r = R.loss_act(pre, res, tgt, idx, it, coef, act)
    gs = float(R.grad_scale(coef, 3, 35))
    e_o = U * a.detach().abs() + U * o64.detach().abs()                        # slope product (0.01f is 0.01 to 4e-8: 1u more below), add
    _within(r["out"], o64.detach(), 2 * (e_o + U * a.detach().abs()))
    e_g = gs * (e_o + U * a.detach().abs() + U * (o64.detach() - y).abs()) + 4 * U * o64.grad.abs()
    _within(r["grad_out"], o64.grad, 2 * e_g)
    _within(r["dpre"], p64.grad, 2 * (e_g + 2 * U * p64.grad.abs()))            # the slope once more (autograd's slope is the double 0.01)
    # at the kink both sides take the negative branch: slope * g, and 0 for ReLU
    kink = r["dpre"].view(-1)[[3, 40]]
    want = {0: 1.0, 1: float(np.float32(0.01)), 2: 0.0}[act]
    assert torch.equal(kink, (torch.tensor(want, dtype=torch.float32) * r["grad_out"].view(-1)[[3, 40]]))
    assert abs(R.loss64(r["d"], coef, 3, 35) - float(loss.detach())) <= 1e-6 * float(loss.detach())


@pytest.mark.parametrize("ks", [2, 3, 5])
def test_splitk_pre_is_the_ordered_sum(ks):
    g = torch.Generator().manual_seed(ks)
    part = torch.randn(ks, 2, 3, 5, 12, generator=g)
    bias = torch.randn(12, generator=g)
    for b in (None, bias):
        got = R.splitk_pre(part, b)
        ref = part.double().sum(0) + (0 if b is None else b.double())
        mag = part.double().abs().sum(0) + (0 if b is None else b.double().abs())
        _within(got, ref, (ks + 1) * U * mag)
    # the order is slab 0 first: a case where another order rounds differently
    p = torch.tensor([1.0, 2.0 ** -24, 2.0 ** -24]).reshape(3, 1, 1, 1, 1).repeat(1, 1, 1, 1, 4)
    assert float(R.splitk_pre(p)[0, 0, 0, 0]) == 1.0


@pytest.mark.parametrize("p", [1.0, 1.5, 3.0])
@pytest.mark.parametrize("it", [0, 2])
def test_lp64_matches_autograd(p, it):
    shape, c2, cp = (3, 5, 7, 12), 0.75, 1.25
    pred, _, tgt, idx = _case(shape, 7)
    y = R.rows(tgt, idx, it, 3)
    pred.view(-1)[[1, 500]] = y.reshape(-1)[[1, 500]]
    pr = pred.double().requires_grad_(True)
    l2 = c2 * O.lp_loss(nchw(pr), nchw(y.double()), p=2.0)
    lp = cp * O.lp_loss(nchw(pr), nchw(y.double()), p=p)
    (l2 + lp).backward()
    grad, s2, sp = R.lp64(pred, tgt, idx, it, c2, cp, p)
    torch.testing.assert_close(grad, pr.grad, rtol=2 * U, atol=0)              # (the fp32 1 / npix against the exact one)
    assert bool((grad.view(-1)[[1, 500]] == 0).all()) and bool(torch.isfinite(grad).all())
    l2, lp = float(l2.detach()), float(lp.detach())
    assert abs(s2 - l2) <= 4 * U * l2 and abs(sp - lp) <= (p + 2) * U * lp


@pytest.mark.parametrize("shape,mag", R.GDN_CASES)
@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_formulas_match_f_gdn_autograd(shape, mag, inverse):
    """out, dL/dout, t and dx against autograd through the oracle's f_gdn.  f_gdn computes norm = gamma' . x^2 + beta itself, so the
    check runs with a real (non-diagonal) gamma: the reference is fed the norm f_gdn's expression gives, and dL/dx of the whole block
    must equal gdn_dx64 with acc = gamma'^T . t -- which holds only if t = dL/dnorm and the dx formula are both right."""
    B, H, W, C = shape
    coef, it = 2.0, 2
    c = R.gdn_inputs(shape, mag)
    idx = R.idx_table(B)
    g = torch.Generator().manual_seed(C)
    gamma = (0.1 * torch.eye(C) + 0.02 * torch.rand(C, C, generator=g)).double().sqrt()
    beta = (0.5 + torch.rand(C, generator=g)).double().sqrt()
    x = nchw(c["x"]).double().contiguous().requires_grad_(True)
    y = O.f_gdn(x, gamma, beta, inverse)
    o = y + nchw(c["res"]).double()
    o.retain_grad()
    loss = coef * O.lp_loss(o, nchw(R.rows(c["tgt"], idx, it, B)).double(), p=2.0)
    loss.backward()
    gp = O._GAMMA_REPARAM(gamma)
    n = F.conv2d(x.detach() ** 2, gp.reshape(C, C, 1, 1), O._BETA_REPARAM(beta)).permute(0, 2, 3, 1).contiguous()
    r = R.loss_gdn64(c["x"].double(), n, c["res"], c["tgt"], idx, it, coef, inverse)
    tol = dict(rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(r["out"], o.detach().permute(0, 2, 3, 1), **tol)
    # the reference's gs is the kernel's fp32 value: 3u from the exact 2 coef / npix
    torch.testing.assert_close(r["grad_out"], o.grad.permute(0, 2, 3, 1), rtol=4 * U, atol=1e-13)
    acc = torch.einsum("bhwo,oi->bhwi", r["t"], gp)                             # gamma'^T . t
    dx, _ = R.gdn_dx64(r["grad_out"], c["x"], n, acc, inverse)
    torch.testing.assert_close(dx, x.grad.permute(0, 2, 3, 1), rtol=1e-6, atol=1e-6 * float(x.grad.abs().max()))
    assert abs(R.loss64((r["out"] - R.rows(c["tgt"], idx, it, B).double()), coef, B, H * W) - float(loss.detach())) <= 1e-12 * float(loss.detach())


@pytest.mark.parametrize("shape,mag", R.GDN_CASES)
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_gdn_bounds_admit_the_fp32_cpu_chain(shape, mag, inverse, with_res):
    """Condition on the inputs of the GPU test: the fp32 chain of the reference itself reaches at most 0.75 of every bound."""
    B = shape[0]
    c = R.gdn_inputs(shape, mag)
    idx = R.idx_table(B)
    res = c["res"] if with_res else None
    for it in (0, 2):
        r64 = R.loss_gdn64(c["x"], c["n"], res, c["tgt"], idx, it, 2.0, inverse)
        r32 = R.loss_gdn32(c["x"], c["n"], res, c["tgt"], idx, it, 2.0, inverse)
        bnd = R.gdn_bounds(r64)
        for k in ("out", "grad_out", "t"):
            _within(r32[k], r64[k], 0.75 * bnd[k])
    dx64, b = R.gdn_dx64(c["g"], c["x"], c["n"], c["acc"], inverse)
    _within(R.gdn_dx32(c["g"], c["x"], c["n"], c["acc"], inverse), dx64, 0.75 * b)


def test_gather_mask_runs_over_the_global_batch():
    g = torch.Generator().manual_seed(5)
    cq, cf = torch.randn(5, 3, 4, 8, generator=g), torch.randn(5, 3, 4, 8, generator=g)
    idx = torch.tensor([[4, 0, 2, 1, 3], [0, 0, 1, 4, 2]], dtype=torch.int32)
    whole = R.gather(cq, cf, idx, 1, 5, 0.5, 0xDEADBEEF)
    part = R.gather(cq, cf, idx[:, 2:].contiguous(), 1, 3, 0.5, 0xDEADBEEF, batch_offset=2)
    assert torch.equal(part, whole[2:])
    assert not torch.equal(part, R.gather(cq, cf, idx[:, 2:].contiguous(), 1, 3, 0.5, 0xDEADBEEF))
    assert torch.equal(R.gather(cq, cf, idx, 0, 5, 1.0, 77), cq[idx[0].long()])      # prob = 1: threshold 2^32, every element kept
    assert torch.equal(R.gather(cq, cf, idx, 0, 5, 0.0, 77), cf[idx[0].long()])
    keep = (whole == cq[idx[1].long()]).float().mean()
    assert 0.4 < float(keep) < 0.6


def test_h2_planes_layout_and_exactness():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 5, 48, generator=g) * torch.logspace(-4, 1, 48)
    s = 8.0
    pl = R.h2_planes(x, s)
    assert pl.shape == (2, 3, 30, 16) and pl.dtype == torch.int16
    back = (pl[0].view(torch.float16).double() + pl[1].view(torch.float16).double()).permute(1, 0, 2).reshape(x.shape) / s
    # |x s - h1 - h2| <= 2^-24 |x s|, with an absolute floor where h2 is an fp16 denormal (spacing 2^-24)
    assert bool(((back - x.double()).abs() <= 2.0 ** -22 * x.double().abs() + 2.0 ** -25 / s).all())
    assert pl[0, 2, 7, 5].view(torch.float16) == (x.reshape(-1, 48)[7, 37] * s).half()
    assert R.overflow_word(torch.tensor([1.0, -3.0, 2.0]), 4.0) == 0x41400000   # 12.0f


def test_pixel_shuffles_are_the_nhwc_permutation():
    x = torch.arange(2 * 3 * 5 * 16, dtype=torch.float32).reshape(2, 3, 5, 16)
    big = R.pixel_shuffle2(x)
    assert big.shape == (2, 6, 10, 4)
    # channel c of large pixel (2h + dy, 2w + dx) is channel 4c + 2dy + dx of small pixel (h, w)
    assert big[1, 2 * 2 + 1, 2 * 3 + 0, 3] == x[1, 2, 3, 4 * 3 + 2 * 1 + 0]
    assert torch.equal(R.pixel_unshuffle2(big), x)
