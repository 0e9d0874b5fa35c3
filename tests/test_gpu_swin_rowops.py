"""Row operations of the transformer path against the float64 references of oracle/rowops_oracle.py, per element: the four LayerNorm
kernels (`layer_norm` of csrc/elementwise.hip; `layer_norm_bwd`, `add_layer_norm`, `layer_norm_bwd_add` of csrc/swin.hip), GELU and its
derivative, round.  Outputs are NaN-filled before every launch and must come back finite.  Bound per element: 4 x the worst err / unit of
the float32 restatement on the same inputs (units: the oracle's docstring; they carry the cancellation in x - mean and are absolute in
u |v| for GELU); dgamma: the derived bound of the same docstring with the factor 1.  Inputs: tests/attention_cases.py -- rows with mean 100
and spread 0.1, a constant row, a row whose variance is below eps, gains in [0.3, 3].  Each figure is printed before it is asserted."""
import pytest
import torch

import attention_cases as AC
from oracle import attention_oracle as A
from oracle import rowops_oracle as R

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def _hold(what, got, ref, unit, r32):
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not finite (never written?)"
    ratio = A.worst_ratio(got, ref, unit)
    print(f"  {what}: err / unit  restatement {r32:.3f}  kernel {ratio:.3f}  allowed {4 * r32:.3f}")
    assert ratio <= 4 * r32, (what, ratio, 4 * r32)


# C: 4, 16 (one partial lane group), 192 | 208 and 320 | 336 (the VPL boundaries C / 4 = 48 | 52 and 80 | 84), 512 (the most), and 7, 65 for
# the scalar kernels.  rows: 1, 15 | 16 | 17 (one block of the vector kernels holds 16), 1 030, and 65 552 = one lap of 4 096 blocks x 16
# rows + 16 -- at the narrow widths, where the float64 reference stays small; the row loop is the same code at every width.
SHAPES = [(rows, C) for C in (4, 16, 192, 208, 320, 336, 512, 7, 65) for rows in (1, 15, 16, 17, 1030)] + [(65552, 4), (65552, 16), (65552, 192)]


@pytest.mark.parametrize("rows,C", SHAPES)
def test_layer_norm_kernels_match_float64_per_element(rows, C):
    from hipops import ops
    print(f"\nrows {rows} C {C}")
    x, w, b, dy = AC.ln_inputs(rows, C, rows + C)
    nslabs = 8 if rows < 4096 else 64
    f = R.layer_norm64(x, w, b)
    bw = R.layer_norm_bwd64(x, w, dy, nslabs=nslabs)
    # the restatement adds a row in the order of the kernel it stands for: 64 lanes (scalar kernels), 16 lanes of float4 (vector kernels)
    r_y = A.worst_ratio(R.layer_norm32(x, w, b)[0], f["y"], f["unit_y"])
    r_dx = A.worst_ratio(R.layer_norm_bwd32(x, w, dy), bw["dx"], bw["unit_dx"])
    assert r_y < float("inf") and r_dx < float("inf")
    if C % 4 == 0:
        r_yv = A.worst_ratio(R.layer_norm32(x, w, b, order="group16")[0], f["y"], f["unit_y"])
        r_dxv = A.worst_ratio(R.layer_norm_bwd32(x, w, dy, order="group16"), bw["dx"], bw["unit_dx"])
    xc, wc, bc, dyc = x.cuda(), w.cuda(), b.cuda(), dy.cuda()

    def dgamma(what, slabs):
        assert bool(torch.isfinite(slabs).all()), f"{what}: a slab element was not written"
        err = (slabs.double().sum(0).cpu() - bw["dgamma"]).abs()
        worst = float((err / bw["bound_dgamma"]).max())
        print(f"  {what}: err / bound {worst:.3f}")
        assert bool((err <= bw["bound_dgamma"]).all()), (what, worst)

    y = _nan(rows, C)
    ops.layer_norm(xc, wc, bc, out=y)
    _hold("layer_norm y", y, f["y"], f["unit_y"], r_y)
    dx, slabs = _nan(rows, C), _nan(nslabs, C)
    ops.layer_norm_bwd(xc, wc, dyc, dx=dx, dgamma_slabs=slabs)
    _hold("layer_norm_bwd dx", dx, bw["dx"], bw["unit_dx"], r_dx)
    dgamma("layer_norm_bwd dgamma", slabs)
    dx_only = _nan(rows, C)
    ops.layer_norm_bwd(xc, wc, dyc, dx=dx_only)                                    # another grid (no slabs): capped at 2 048 blocks
    _hold("layer_norm_bwd dx (no slabs)", dx_only, bw["dx"], bw["unit_dx"], r_dx)
    if C % 4:
        return
    half = (x * 0.5)
    rest = x - half                                                               # exact (Sterbenz): half + rest == x bit for bit
    assert torch.equal(half + rest, x)
    y1, y2, s = _nan(rows, C), _nan(rows, C), _nan(rows, C)
    ops.add_layer_norm(xc, None, wc, bc, out=y1)
    _hold("add_layer_norm y", y1, f["y"], f["unit_y"], r_yv)
    ops.add_layer_norm(half.cuda(), rest.cuda(), wc, bc, sum_out=s, out=y2)
    assert torch.equal(s, xc) and torch.equal(y2, y1)
    dxv, slabv = _nan(rows, C), _nan(nslabs, C)
    ops.layer_norm_bwd_add(xc, wc, dyc, dx=dxv, dgamma_slabs=slabv)
    _hold("layer_norm_bwd_add dx", dxv, bw["dx"], bw["unit_dx"], r_dxv)
    dgamma("layer_norm_bwd_add dgamma", slabv)
    dxv2 = _nan(rows, C)
    ops.layer_norm_bwd_add(xc, wc, dyc, dx=dxv2)                                   # no slabs: the grid capped at 4 096 blocks, rows in laps
    assert torch.equal(dxv2, dxv)
    e1, e2, dxa = dyc * 0.75, xc * 0.125, _nan(rows, C)
    ops.layer_norm_bwd_add(xc, wc, dyc, e1, e2, dx=dxa)
    assert torch.equal(dxa, e2 + (e1 + dxv))                                       # the addends enter in this order


def test_layer_norm_without_gain_and_bias():
    """weight / bias None (the kernels then use 1 and 0) on the scalar and the vector kernels"""
    from hipops import ops
    rows, C = 33, 192
    x, _, _, dy = AC.ln_inputs(rows, C, 5)
    f = R.layer_norm64(x)
    bw = R.layer_norm_bwd64(x, None, dy)
    xc, dyc = x.cuda(), dy.cuda()
    for name, fn, bwd, order in (("layer_norm", lambda out: ops.layer_norm(xc, None, None, out=out), ops.layer_norm_bwd, "wave64"),
                                 ("add_layer_norm", lambda out: ops.add_layer_norm(xc, None, None, None, out=out), ops.layer_norm_bwd_add, "group16")):
        r_y = A.worst_ratio(R.layer_norm32(x, order=order)[0], f["y"], f["unit_y"])
        r_dx = A.worst_ratio(R.layer_norm_bwd32(x, None, dy, order=order), bw["dx"], bw["unit_dx"])
        _hold(name, fn(_nan(rows, C)), f["y"], f["unit_y"], r_y)
        _hold(name + " backward", bwd(xc, None, dyc, dx=_nan(rows, C)), bw["dx"], bw["unit_dx"], r_dx)


def test_gelu_and_its_derivative_over_the_tails():
    """x on a grid over [-12, 12] with +-0, +-1e-30, +-5, +-8.5 planted, long enough for a second grid-stride lap (4 096 blocks x 256)"""
    from hipops import ops
    n = 4096 * 256 + 77
    v = AC.gelu_inputs(n)
    dy = torch.randn(n, generator=torch.Generator().manual_seed(11)) * 3
    y_ref, uy = R.gelu64(v)
    g_ref, ug = R.gelu_bwd64(dy, v)
    gp_ref, ugp = R.gelu_grad64(v)
    r_y = A.worst_ratio(R.gelu32(v), y_ref, uy)
    r_g = A.worst_ratio(dy * R.gelu_grad32(v), g_ref, ug)
    r_gp = A.worst_ratio(R.gelu_grad32(v), gp_ref, ugp)
    vc = v.cuda()
    print()
    _hold("gelu", ops.gelu(vc, out=_nan(n)), y_ref, uy, r_y)
    _hold("gelu_bwd", ops.gelu_bwd(dy.cuda(), vc, dx=_nan(n)), g_ref, ug, r_g)
    _hold("gelu'", ops.gelu_bwd(torch.ones(n, device="cuda"), vc, dx=_nan(n)), gp_ref, ugp, r_gp)


def test_round_is_exact_ties_to_even():
    from hipops import ops
    gen = torch.Generator().manual_seed(2)
    k = torch.cat([torch.arange(-2050, 2051), torch.randint(-2 ** 22, 2 ** 22 + 1, (4096 * 256,), generator=gen),
                   torch.tensor([2 ** 22, -2 ** 22, 2 ** 22 - 1, -2 ** 22 + 1])]).double()
    ties = (k + 0.5).float()
    assert torch.equal(ties.double(), k + 0.5)                                      # representable
    want_ties = torch.copysign((k + (k.abs() % 2 == 1).double()).float(), ties)     # even k stays, odd k goes to k + 1; -0.5 -> -0
    other = torch.tensor([0.0, -0.0, 2.0 ** 23 + 1, -(2.0 ** 23 + 1), 0.49999997, -0.49999997, 1e-30, -1e-30, 2.0 ** 31, 3.4e38])
    want_other = torch.tensor([0.0, -0.0, 2.0 ** 23 + 1, -(2.0 ** 23 + 1), 0.0, -0.0, 0.0, -0.0, 2.0 ** 31, 3.4e38])
    v, want = torch.cat([other, ties]), torch.cat([want_other, want_ties])
    got = ops.round_(v.cuda(), out=_nan(v.numel())).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))               # bits: the sign of zero included
    assert torch.equal(want.view(torch.int32), torch.round(v).view(torch.int32))    # (the expectation itself, against torch on the CPU)
