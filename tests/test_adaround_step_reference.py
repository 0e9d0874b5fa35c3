"""CPU anchor of `oracle.rdo_oracle.adaround_step_reference`, the float64 closed form that tests/test_gpu_adaround_step.py holds the
AdaRound step kernels against: thirty consecutive steps of torch.autograd through `O.adaround_forward(soft=True)` and
`O.round_loss_term` -- the two functions the reference goldens pin -- driven by torch.optim.Adam(lr=1e-3), every step restated by the
closed form from the optimiser's state before it."""
import pytest
import torch

from oracle import lic_oracle
from oracle import rdo_oracle as O

ITERS = 30
REPARAM = (2.0 ** -18, 2.0 ** -36)          # CompressAI's NonNegativeParametrizer of a GDN gamma: bound, pedestal


def _sched():
    from hipops import ops
    return ops.make_sched(ITERS, 0.2, (20, 2), device="cpu")


def _inputs(reparam, seed):
    g = torch.Generator().manual_seed(seed)
    if reparam:
        w = torch.sqrt((0.05 * torch.rand(24, 24, generator=g).pow(4)).pow(2) + 2.0 ** -36).float()      # a quarter of it below one step
    else:
        w = (0.1 * torch.randn(12, 2, 3, 8, generator=g)).float()
    delta, zp = O.uaq_init(w, 8, True, "max")
    alpha = O.adaround_init_alpha(w, delta) + 1.5 * torch.randn(w.shape, generator=g)
    flat = alpha.view(-1)
    n = flat.numel()
    for k, val in enumerate((0.0, 0.0, 90.0, 90.0, -90.0, -90.0)):           # u = 0 (h = 1/2) and saturated sigmoids
        flat[(k * n) // 6 + 5] = val
    # w, delta and zp stay float32: floor(w / delta) is then the reference's own fp32 floor on both sides, everything behind it float64
    return w, delta, zp, alpha.double(), g


@pytest.mark.parametrize("reparam", [False, True])
def test_closed_form_reproduces_autograd_and_adam(reparam):
    w, delta, zp, alpha0, g = _inputs(reparam, 3 + int(reparam))
    sched = _sched()
    assert float(sched[0, 1]) == 0.0 and float(sched[4, 1]) == 0.0 and float(sched[5, 1]) == 1.0      # warm-up rows and rows behind it
    alpha = alpha0.clone().requires_grad_(True)
    opt = torch.optim.Adam([alpha], lr=1e-3)
    lower = lic_oracle.LowerBound(REPARAM[0]).double()
    grad_scale, round_weight = 0.25, 0.01
    n_round = 0
    for it in range(ITERS):
        b, round_on = float(sched[it, 0]), float(sched[it, 1])
        G = 1e-2 * torch.randn(w.shape, generator=g, dtype=torch.float64)
        st = opt.state.get(alpha, {})
        m0 = st["exp_avg"].clone() if st else torch.zeros_like(alpha0)
        v0 = st["exp_avg_sq"].clone() if st else torch.zeros_like(alpha0)
        a0 = alpha.detach().clone()
        ref = O.adaround_step_reference(w, delta, zp, a0, m0, v0, G, sched[it], n_levels=256, grad_scale=grad_scale,
                                        round_weight=round_weight, reparam=REPARAM if reparam else None)
        if reparam and it == 0:          # the LowerBound rule is exercised on both of its sides: clipped elements that pass and that do not
            low = ref["masks"]["q"] < REPARAM[0]
            assert int((low & (G < 0)).sum()) >= 3 and int((low & (G > 0)).sum()) >= 3
        opt.zero_grad()
        wq = O.adaround_forward(w, alpha, delta, zp, 256, soft=True)
        if reparam:
            wq = lower(wq) ** 2 - REPARAM[1]
        loss = (wq * G).sum() * grad_scale
        if round_on:
            rl = O.round_loss_term(alpha, b, round_weight)
            torch.testing.assert_close(ref["round_loss"], rl.detach(), rtol=1e-12, atol=0)
            loss = loss + rl
            n_round += 1
        else:
            assert float(ref["round_loss"]) == 0.0
        loss.backward()
        torch.testing.assert_close(ref["g_total"], alpha.grad, rtol=1e-12, atol=1e-300)
        opt.step()
        st = opt.state[alpha]
        # exp_avg / exp_avg_sq do not see the schedule row: the arithmetic alone, rtol 1e-9 (they agree to ~1e-15)
        torch.testing.assert_close(ref["m"], st["exp_avg"], rtol=1e-9, atol=1e-300)
        torch.testing.assert_close(ref["v"], st["exp_avg_sq"], rtol=1e-9, atol=1e-300)
        # alpha: the row stores step_size and bc2_sqrt as float32 -- one rounding of 2^-24 (relative) each, where torch.optim.Adam holds
        # doubles -- so this step's MOVE may differ by 2 * 2^-24 of itself; everything else to rtol 1e-9
        move = (alpha.detach() - a0).abs()
        err = (ref["alpha"] - alpha.detach()).abs()
        assert bool((err <= 1e-9 * alpha.detach().abs() + 2 * 2.0 ** -24 * move).all()), (it, float(err.max()))
        torch.testing.assert_close(ref["wq"], (lower(O.adaround_forward(w, ref["alpha"], delta, zp, 256, True)) ** 2 - REPARAM[1]) if reparam
                                   else O.adaround_forward(w, ref["alpha"], delta, zp, 256, True), rtol=1e-12, atol=0)
    assert n_round == ITERS - 5
    flat = alpha.detach().view(-1)
    assert bool(torch.isfinite(flat).all())
    moved = (alpha.detach() - alpha0).abs()
    assert float(moved.max()) > 5e-3                 # the run went somewhere: thirty steps of ~1e-3


def test_planted_elements_take_the_documented_branches():
    """alpha = 0 is u = 0 (no rounding gradient, the regulariser's full value), alpha = +-90 a saturated sigmoid (no gradient at all)."""
    w, delta, zp, alpha, g = _inputs(False, 3)
    G = 1e-2 * torch.randn(w.shape, generator=g, dtype=torch.float64)
    z = torch.zeros_like(alpha)
    ref = O.adaround_step_reference(w, delta, zp, alpha, z, z, G, (7.5, 1.0, 1e-3, 1.0), n_levels=256, grad_scale=1.0, round_weight=0.01)
    a = alpha.view(-1)
    zero, sat = a == 0, a.abs() == 90
    assert int(zero.sum()) == 2 and int(sat.sum()) == 4
    # (float64 leaves h = 1/2 + 1e-16 where the kernels' fp32 chain gives 1/2 exactly: u^(b-1) is 1e-100 against 0)
    assert bool((ref["g_round"].view(-1)[zero].abs() < 1e-90).all()) and bool(((ref["masks"]["h"].view(-1)[zero] - 0.5).abs() < 1e-15).all())
    assert bool((ref["g_total"].view(-1)[sat] == 0).all()) and bool((ref["alpha"].view(-1)[sat] == a[sat]).all())
    for k in ("m", "v", "alpha", "wq", "g_total"):
        assert bool(torch.isfinite(ref[k]).all()), k
