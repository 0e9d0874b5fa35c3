"""Pins tests/tape_reference.py (CPU, no GPU, no library): S dominates the reference, the float32 chain of an exactly representable case
is the float64 value, the input gradient of every conv geometry has the input's shape -- with PER-AXIS output padding, which the
mixed-remainder cases need --, the unfolded zero-insertion form the chain is built from is the autograd gradient, and the kink mask of
every listed case stays under the cap the GPU test enforces."""
import pytest
import torch
import torch.nn.functional as F

import tape_reference as T

SMALL_CONV = [n for n, c in T.CONV_CASES.items() if c[9] != "x6"]
SMALL_TCONV = [n for n, c in T.TCONV_CASES.items() if c[11] != "x6"]


def _refs(c):
    r = c["ref"]
    return r, r.backward(c["go"])


@pytest.mark.parametrize("name", SMALL_CONV)
def test_conv_reference_dominated_by_s_and_dgrad_has_the_input_shape(name):
    B, H, W, Cin, Cout, K, s, p, act = T.CONV_CASES[name][:9]
    c = T.conv_case(name)
    r, bw = _refs(c)
    assert not c["go"].is_contiguous()
    assert bool((r.S_pre >= r.pre.abs()).all()) and bool((r.S >= r.y.abs()).all()) and bool((bw["S"] >= bw["dx"].abs()).all())
    assert tuple(bw["dx"].shape) == tuple(bw["S"].shape) == (B, Cin, H, W)
    # the geometry the library's dgrad must use: conv_transpose2d with the remainders of BOTH axes as output padding
    op = T.conv_out_pad(H, W, K, s, p)
    s64, _ = T._slopes(r.pos, act)
    g = c["go"].double() if s64 is None else c["go"].double() * s64
    dx_t = F.conv_transpose2d(g, c["w"].double(), None, s, p, output_padding=op)
    assert tuple(dx_t.shape) == (B, Cin, H, W)
    assert float((dx_t - bw["dx"]).abs().max()) <= 1e-12 * float(bw["S"].max())
    if name in T.MIXED_CASES:
        assert op[0] != op[1]
        wrong = F.conv_transpose2d(g, c["w"].double(), None, s, p, output_padding=op[0])
        assert tuple(wrong.shape) != (B, Cin, H, W)                  # one scalar for both axes gives another size
    # ... and the stride-1 conv over the zero-inserted gradient with flipped taps (what the chain unfolds) is the same tensor
    zi = F.conv2d(T.zero_insert(g, s, K - 1 - p, *op), T.tconv_weight_as_conv(c["w"].double()))
    assert float((zi - bw["dx"]).abs().max()) <= 1e-12 * float(bw["S"].max())
    assert 0.0 < r.q < 16.0 and 0.0 < bw["q"] < 16.0                 # a sequential chain of <= 1 728 terms on random data: a few u S


@pytest.mark.parametrize("name", SMALL_TCONV)
def test_tconv_reference_dominated_by_s(name):
    B, H, W, Cin, Cout, K, s, p, op, act = T.TCONV_CASES[name][:10]
    c = T.tconv_case(name)
    r, bw = _refs(c)
    assert tuple(r.y.shape) == (B, Cout, (H - 1) * s - 2 * p + K + op, (W - 1) * s - 2 * p + K + op)
    assert bool((r.S >= r.y.abs()).all()) and bool((bw["S"] >= bw["dx"].abs()).all())
    assert tuple(bw["dx"].shape) == (B, Cin, H, W)
    zi = F.conv2d(T.zero_insert(c["x"].double(), s, K - 1 - p, op, op), T.tconv_weight_as_conv(c["w"].double()), c["b"].double())
    assert float((zi - r.pre).abs().max()) <= 1e-12 * float(r.S_pre.max())
    assert 0.0 < r.q < 16.0 and 0.0 < bw["q"] < 16.0


@pytest.mark.parametrize("kind", ["conv", "tconv"])
def test_chain32_of_an_exactly_representable_case_is_the_float64_value(kind):
    """small integers: every product and partial sum is exact in float32, so the chain equals float64 bit for bit (q = 0), with the
    taps flipped and the output padding placed as conv_transpose2d does"""
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 5, (2, 5, 7, 6), generator=gen).float()
    b = torch.randint(-3, 4, (4,), generator=gen).float()
    if kind == "conv":
        w = torch.randint(-4, 5, (4, 5, 3, 3), generator=gen).float()
        r = T.TapeRef("conv", x, w, b, 2, 1, act="lrelu")
        go = torch.randint(-4, 5, tuple(r.pre.shape), generator=gen).float()
        idx, c = T.chain32(x, w, b, 2, 1)
    else:
        w = torch.randint(-4, 5, (5, 4, 3, 3), generator=gen).float()
        r = T.TapeRef("tconv", x, w, b, 2, 1, (1, 0))
        go = torch.randint(-4, 5, tuple(r.pre.shape), generator=gen).float()
        idx, c = T.tconv_chain32(x, w, b, 2, 1, (1, 0))
    assert r.q_pre == 0.0
    assert torch.equal(c.double(), T.rows_of(r.pre)[idx])
    if kind == "tconv":
        assert r.backward(go)["q"] == 0.0
    else:
        r0 = T.TapeRef("conv", x, w, b, 2, 1)                        # (without the LeakyReLU: 0.01f times an integer is not exact)
        assert r0.backward(go)["q"] == 0.0


def test_chain32_subsamples_large_cases_with_both_ends():
    gen = torch.Generator().manual_seed(4)
    x, w = torch.randn(1, 8, 9, 9, generator=gen), torch.randn(8, 8, 3, 3, generator=gen)
    full, part = T.chain32(x, w, None, 1, 1), T.chain32(x, w, None, 1, 1, max_products=8 * 72 * 10)
    assert len(full[0]) == 81 and len(part[0]) == 10 and int(part[0][0]) == 0 and int(part[0][-1]) == 80
    assert torch.equal(full[1][part[0]], part[1])


@pytest.mark.parametrize("name", [n for n, c in T.CONV_CASES.items() if c[8] != "none"] +
                         [n for n, c in T.TCONV_CASES.items() if c[9] != "none"])
def test_kink_mask_stays_under_the_cap(name):
    """with the widest d (2): the cap of the GPU test is met by the reference's inputs alone"""
    r = (T.conv_case if name in T.CONV_CASES else T.tconv_case)(name)["ref"]
    m = r.mask(2)
    assert int(m.sum()) <= T.MASK_CAP * m.numel(), (name, int(m.sum()), m.numel())
    assert bool((r.bound_y(2) >= 0).all())


@pytest.mark.parametrize("name", ["gdn_c8_7x9", "igdn_c36_7x9", "gdn_c36_span", "igdn_c36_span"])
def test_gdn_reference_and_its_first_order_bounds(name):
    """the float32 restatement of the same formulas stays inside the derived bounds (value and input gradient)"""
    c = T.gdn_case(name)
    r = c["ref"]
    bw = r.backward(c["go"])
    assert bool((r.S_n >= r.n.abs()).all()) and float(r.n.min()) >= 1.0
    x, go = c["x"], c["go"].contiguous()
    n32 = F.conv2d(x * x, r.w, c["beta"])
    f32 = n32.sqrt() if r.inverse else n32.rsqrt()
    assert bool(((x * f32).double() - r.y).abs().le(r.bound_y(0)).all())
    t32 = go * x * (0.5 * n32.rsqrt() if r.inverse else -0.5 * n32.rsqrt() ** 3)
    dx32 = go * f32 + 2.0 * x * F.conv2d(t32, bw["wt"])
    assert bool((dx32.double() - bw["dx"]).abs().le(r.bound_dx(bw, 0)).all())
    if "span" in name:
        tok = x.abs().amax(1)
        assert float(tok.max() / tok.min()) > 50.0


@pytest.mark.parametrize("name", ["3d_conv_path", "4d_conv_path"])
def test_linear_reference_is_f_linear(name):
    c = T.linear_case(name)
    r = c["ref"]
    assert not c["x"].is_contiguous() and not c["go"].is_contiguous()
    x64 = c["x"].double().requires_grad_(True)
    y = F.linear(x64, c["w"].double(), c["b"].double())
    (dx,) = torch.autograd.grad(y, x64, c["go"].double())
    assert torch.allclose(y.detach().reshape(-1, y.shape[-1]), r.y.flatten(1), rtol=0, atol=1e-13)
    bw = r.backward(c["go"].reshape(-1, c["go"].shape[-1], 1, 1))
    assert torch.allclose(dx.reshape(-1, dx.shape[-1]), bw["dx"].flatten(1), rtol=0, atol=1e-13)
    assert bool((r.S >= r.y.abs()).all()) and bool((bw["S"] >= bw["dx"].abs()).all())


@pytest.mark.parametrize("name", ["flip_3x3_lrelu", "flip_5x5", "zi_3x3_s2_odd", "mixed_9x10", "mixed_10x9", "phase_4x4_s2", "no_bias"])
def test_bound_admits_float32_torch_and_refuses_a_wrong_tape(name):
    """the bound is neither vacuous nor out of reach: torch's own float32 conv / dgrad (another summation order) stays inside it with
    d = 0; taps that are not flipped, the branch slopes left out, or the output padding on the wrong axis do not"""
    B, H, W, Cin, Cout, K, s, p, act = T.CONV_CASES[name][:9]
    c = T.conv_case(name)
    r, bw = _refs(c)
    x, w, b = c["x"].contiguous(), c["w"], c["b"]
    _, s32 = T._slopes(r.pos, act)
    pre32 = F.conv2d(x, w, b, s, p)
    y32 = pre32 if s32 is None else pre32 * s32
    assert bool(((y32.double() - r.y).abs() <= r.bound_y(0)).all())
    g32 = c["go"].contiguous() if s32 is None else c["go"].contiguous() * s32
    op = T.conv_out_pad(H, W, K, s, p)
    inside = lambda dx: bool(((dx.double() - bw["dx"]).abs() <= T.bound_dx(bw, 0)).all())
    assert inside(F.conv_transpose2d(g32, w, None, s, p, output_padding=op))
    if K > 1:
        assert not inside(F.conv_transpose2d(g32, w.flip(2, 3), None, s, p, output_padding=op))
    if s32 is not None:
        assert not inside(F.conv_transpose2d(c["go"].contiguous(), w, None, s, p, output_padding=op))
    if op[0] != op[1]:
        # the padding row / column on the other axis: not the input's size
        swapped = F.conv_transpose2d(g32, w, None, s, p, output_padding=(op[1], op[0]))
        assert tuple(swapped.shape) != (B, Cin, H, W)
