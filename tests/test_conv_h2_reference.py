"""Pins tests/conv_h2_reference.py (the CPU reference of rdo_conv2d_fwd_h2) without a GPU:
  * the restated split against hand-written values, its two layouts against the index formulas of the headers;
  * `ref` against a tap-by-tap float64 sum and F.conv2d on a tiny case, every epilogue form against its definition;
  * 'exact' family: integer `ref`, max S < 2^24, q = 0 and an all-zero plane 1 on every geometry;
  * 'randn' family: the masked share of every geometry and epilogue is <= MASK_CAP (pytest -s prints q and the share), the scaled channels
    defeat the max-norm, and a float32 convolution in another summation order stays within 0.75 of the bound;
  * `expected_launch`: every case reaches the launch its row names, every row of the table is reached, every tag is one of the four."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_h2_reference as R

U = R.U
GEOMS = list(R.GEOMS)


def _bits(t):
    return [int(v) & 0xFFFF for v in t.view(torch.int16).reshape(-1)]


def test_split_hand_values():
    s = 4.0
    v = torch.tensor([0.0, -0.0, 0.25, (1.0 + 2.0 ** -11 + 2.0 ** -21) / 4.0, 2.0 ** -2 * (2.0 ** -12 + 2.0 ** -24), 65504.0 / 4.0, 65536.0 / 4.0, -7.5])
    p0, p1, rep = R.split(v, s)
    #        0       -0      1.0     1 + 2^-11 + 2^-21: ties-to-even would keep 1, the extra 2^-21 rounds up to 1 + 2^-10; the remainder
    #                                -2^-11 + 2^-21 = -(1 - 2^-10) 2^-11 is an fp16 number
    assert _bits(p0)[:3] == [0x0000, 0x8000, 0x3C00] and _bits(p1)[:3] == [0x0000, 0x0000, 0x0000]
    assert _bits(p0)[3] == 0x3C01 and float(p1[3]) == -(2.0 ** -11) + 2.0 ** -21
    # 2^-12 + 2^-24: a quarter of an ulp stays behind, plane 1 is the smallest fp16 DENORMAL (0x0001)
    assert _bits(p0)[4] == 0x0C00 and _bits(p1)[4] == 0x0001
    # 65504 fits; 65536 rounds to +inf and the remainder to -inf: the represented value is no number
    assert _bits(p0)[5] == 0x7BFF and _bits(p1)[5] == 0x0000
    assert _bits(p0)[6] == 0x7C00 and _bits(p1)[6] == 0xFC00 and bool(torch.isnan(rep[6]))
    assert float(rep[7]) == -7.5 and float(rep[3]) == float(v[3]) and float(rep[4]) == float(v[4])
    assert torch.equal(rep[:6].float().double(), rep[:6])                              # a float32 number
    assert R.pow2_scale(3.0) == 32.0 and R.pow2_scale(128.0) == 1.0 and R.pow2_scale(129.0) == 0.5 and R.pow2_scale(0.0) == 1.0
    assert R.pow2_scale(64.0) == 2.0 and R.pow2_scale(64.5) == 1.0


def test_plane_layouts_are_the_index_formulas():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 5, 32, generator=gen)
    p0, p1, _ = R.split(x, 8.0)
    pl = R.act_planes(p0, p1)
    assert pl.shape == (2, 2, 30, 16) and pl.dtype == torch.int16
    f0, f1 = p0.view(torch.int16).reshape(30, 32), p1.view(torch.int16).reshape(30, 32)
    for m in (0, 7, 29):
        for c in (0, 15, 16, 31):
            assert pl[0, c // 16, m, c % 16] == f0[m, c] and pl[1, c // 16, m, c % 16] == f1[m, c]
    assert torch.equal(R.planes_to_float64(pl, x.shape, 8.0), (p0.double() + p1.double()) / 8.0)
    Cout, KH, KW, Cin = 5, 3, 2, 48
    w = torch.randn(Cout, KH, KW, Cin, generator=gen)
    w0, w1, _ = R.split(w, 16.0)
    wp = R.weight_planes(w0, w1).reshape(2, -1)
    flat = w0.view(torch.int16).reshape(-1)
    for e in range(flat.numel()):                                                      # rdo::frag_index, csrc/rdo_common.h
        t, ci = divmod(e, Cin)
        t, kw = divmod(t, KW)
        co, kh = divmod(t, KH)
        assert wp[0, (((((ci >> 4) * KH + kh) * KW + kw) * Cout + co) << 4) + (ci & 15)] == flat[e]


def _tiny(family="randn"):
    gen = torch.Generator().manual_seed(11)
    B, H, W, Cin, Cout, K, s, p = 2, 6, 5, 16, 16, 3, 2, 1
    Ho, Wo = R.out_hw(H, W, K, s, p)
    d = lambda shape, sc: R._draw(shape, gen, family, sc)
    x, w, b, res, aux = d((B, H, W, Cin), 3.0), d((Cout, K, K, Cin), 0.1), d((Cout,), 0.1), d((B, Ho, Wo, Cout), 1.0), d((B, Ho, Wo, Cout), 1.0)
    aux = torch.where(aux >= 0, aux.clamp_min(R.AUX_MIN), aux.clamp_max(-R.AUX_MIN))
    return x, w, b, res, aux, s, p


def test_ref_is_the_convolution_of_the_represented_operands():
    x, w, b, res, aux, s, p = _tiny()
    r = R.ConvH2Ref(x, w, b, res, aux, s, p)
    B, H, W, Cin = x.shape
    Cout, K = w.shape[0], w.shape[1]
    Ho, Wo = R.out_hw(H, W, K, s, p)
    xr, wr = R.split(x, r.sx)[2], R.split(w, r.sw)[2]
    assert 64.0 < float(x.abs().max()) * r.sx <= 128.0 and 64.0 < float(w.abs().max()) * r.sw <= 128.0
    assert float((xr - x.double()).abs().max()) <= 2.0 ** -22 * float(x.abs().max())   # the split loses about 2^-24 of a value
    want = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64)
    wantS = torch.zeros_like(want)
    xp = F.pad(xr, (0, 0, p, p, p, p))
    for kh in range(K):
        for kw in range(K):
            patch = xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s, :]
            want += patch @ wr[:, kh, kw, :].t()
            wantS += patch.abs() @ wr[:, kh, kw, :].abs().t()
    want, wantS = want + b.double(), wantS + b.double().abs()
    assert float((r.pre - want).abs().max()) <= 1e-13 * float(wantS.max())
    assert float((r.S_pre - wantS).abs().max()) <= 1e-13 * float(wantS.max())
    direct = F.conv2d(xr.permute(0, 3, 1, 2), wr.permute(0, 3, 1, 2), b.double(), s, p).permute(0, 2, 3, 1)
    assert float((r.pre - direct).abs().max()) <= 1e-13 * float(wantS.max())
    assert r.q_pre > 0 and bool((r.S_pre >= r.pre.abs() * (1 - 1e-12)).all())
    # every epilogue form against its definition
    lo = float(np.float32(0.01))
    assert lo != 0.01
    rd, pre = res.double(), r.pre
    defs = {"none": pre, "none_res": pre + rd, "lrelu_res_pre": torch.where(pre > 0, pre, lo * pre) + rd, "relu": pre.clamp_min(0.0),
            "lrelu_bwd": torch.where(aux > 0, pre, lo * pre), "relu_bwd_res": torch.where(aux > 0, pre, torch.zeros_like(pre)) + rd}
    assert set(defs) == set(R.EPILOGUES)
    for key, want in defs.items():
        o = r.out(key)
        assert torch.equal(o.ref, want), key
        assert o.q >= r.q_pre and bool((o.bnd >= 0).all()) and bool((o.bnd[o.ref != 0] > 0).all())    # (ReLU's dead side: exactly 0)
        assert (o.mask is not None) == (key in ("lrelu_res_pre", "relu"))
    o = r.out("lrelu_res_pre")
    assert torch.equal(o.alt, torch.where(pre > 0, lo * pre, pre) + rd) and torch.equal(o.mask, pre.abs() <= r.bound_pre)
    assert torch.equal(o.S, r.S_pre * torch.where(pre > 0, 1.0, lo) + rd.abs())
    # finish32: the same definitions in float32, one rounding per step
    v = pre.float().numpy()
    got = R.finish32(v, R.EPI_LRELU, None, res.numpy())
    assert got.dtype == np.float32 and np.array_equal(got, np.where(v > 0, v, np.float32(0.01) * v).astype(np.float32) + res.numpy())


@pytest.mark.parametrize("name", GEOMS)
def test_exact_family_is_exact_in_float32(name):
    c = R.case(name, "exact")
    r = c["ref"]
    assert float(r.S_pre.max()) + 3.0 < 2.0 ** 24, (name, float(r.S_pre.max()))
    assert r.plane1_zero and r.q_pre == 0.0
    assert torch.equal(r.x64, c["x"].double()) and torch.equal(r.w64, c["w"].double())
    assert torch.equal(r.pre, r.pre.round()) and torch.equal(r.pre.float().double(), r.pre)
    frac0 = float((c["x"] == 0).float().mean())
    assert 0.15 < frac0 < 0.35, (name, frac0)
    assert bool((c["aux"] != 0).all())
    for key in R.epilogues_of(name):
        o = r.out(key)
        out32, pre32 = r.expected32(key)
        assert torch.equal(pre32.double(), r.pre)
        # one rounding per step: within an ulp of the float64 value, and equal to it wherever no slope was applied
        assert float((out32.double() - o.ref).abs().max()) <= 2.0 * U * float(o.ref.abs().max()), (name, key)
        if R.EPILOGUES[key][0] in (R.EPI_NONE, R.EPI_RELU, R.EPI_RELU_BWD):
            assert torch.equal(out32.double(), o.ref), (name, key)
        if o.mask is not None:                                                         # the bound of an exact 0 is 0: both branches give 0 there
            assert torch.equal(o.mask, r.pre == 0) and torch.equal(o.alt[o.mask], o.ref[o.mask])


@pytest.mark.parametrize("name", GEOMS)
def test_randn_family_masked_share_and_q(name):
    c = R.case(name, "randn")
    r = c["ref"]
    assert not r.plane1_zero and r.q_pre > 0
    assert 64.0 < float(c["x"].abs().max()) * r.sx <= 128.0 and 64.0 < float(c["w"].abs().max()) * r.sw <= 128.0
    assert bool(torch.isfinite(r.pre).all()) and bool((c["aux"].abs() >= R.AUX_MIN).all())
    # plane 0 of the aux tensor keeps the sign (the activation-backward forms read only that plane)
    a0, _, _ = R.split(c["aux"], R.pow2_scale(c["aux"].abs().max()))
    assert torch.equal(a0.float() > 0, c["aux"] > 0) and bool((a0.float() != 0).all())
    for key in R.epilogues_of(name):
        o = r.out(key)
        share = 0.0 if o.mask is None else float(o.mask.double().mean())
        print(f"  [{name} {key}] q {o.q:.2f}  masked share {share:.2e}")
        assert share <= R.MASK_CAP, (name, key, share)
    # for the forms every case runs even when it is not an "epi" case
    for key in R.BASIC:
        o = r.out(key)
        assert o.mask is None or float(o.mask.double().mean()) <= R.MASK_CAP


def test_scaled_channels_defeat_the_max_norm():
    """an error of the max-norm allowance test_gpu_h2.py holds (2e-6 of max |ref|) in an element of the smallest output channel... is
    many of its bounds: the per-element bound sees what the max-norm cannot"""
    r = R.case("1x1_cout208", "randn")["ref"]
    o = r.out("none")
    spread = float(o.bnd.amax(dim=(0, 1, 2)).max() / o.bnd.amax(dim=(0, 1, 2)).min())
    assert 2e-6 * float(o.ref.abs().max()) > 30.0 * float(o.bnd.median())
    assert spread > 3.0


def test_another_summation_order_stays_within_the_bound():
    """admission of the bound: torch's own float32 convolution of the represented operands (blocked GEMM order) and a 12-way K split of
    the float32 chain, added split after split"""
    for name in ("5x5_m4095", "halo_cin16"):
        c = R.case(name, "randn")
        r = c["ref"]
        g = R.GEOMS[name]
        o = r.out("none")
        x32, w32 = r.x64.float().permute(0, 3, 1, 2), r.w64.float().permute(0, 3, 1, 2)
        got = F.conv2d(x32, w32, c["bias"], g[6], g[7]).permute(0, 2, 3, 1).double()
        worst = float(((got - o.ref).abs() / o.bnd).max())
        cin = g[3]
        parts = torch.zeros_like(got, dtype=torch.float32)
        for lo in range(0, cin, 16):
            parts = parts + F.conv2d(x32[:, lo:lo + 16], w32[:, lo:lo + 16], None, g[6], g[7]).permute(0, 2, 3, 1)
        worst2 = float((((parts + c["bias"]).double() - o.ref).abs() / o.bnd).max())
        print(f"  [{name}] q {o.q:.2f}  other orders / bound {worst:.3f} {worst2:.3f}")
        assert worst <= 0.75 and worst2 <= 0.75, (name, worst, worst2)


def test_expected_launch_reaches_every_row():
    reached = {}
    for name, c in R.CASES.items():
        e = R.expected_launch(name)
        assert set(e) == {"tag", "kernel", "tile", "ksplit"} and e["tag"] in R.TAGS, (name, e)
        assert R.launch_name(e) == c[8], (name, e, c[8])
        assert R.supported(c[:8]) and set(c[9]) <= set(R.TUNING_DEFAULTS)
        reached.setdefault(c[8], []).append(name)
        t = dict(R.TUNING_DEFAULTS, **c[9])
        B, H, W, Cin, Cout, K, s, p = c[:8]
        Ho, Wo = R.out_hw(H, W, K, s, p)
        if e["ksplit"] > 1:
            assert R.workspace_floats(c[:8], t) >= e["ksplit"] * B * Ho * Wo * Cout
        gmac = B * Ho * Wo * Cout * K * K * Cin / 1e9
        assert gmac <= 2.0 or name.startswith("k32_192"), (name, gmac)                   # (the unsplit 256 x 192 K32 grid needs 256 tiles: 3.6)
    for launch, names in R.TABLE.items():
        for n in names:
            assert R.CASES[n][8] == launch and n in reached[launch], (launch, n)
    assert set(reached) == set(R.TABLE)
    assert {R.expected_launch(n)["tag"] for n in R.CASES} == set(R.TAGS)
    # what the rows are there for
    assert R.expected_launch("5x5_m4095")["ksplit"] == 12 and 125 % 12 != 0            # uneven stage ranges
    assert R.expected_launch("k32_split64") == {"tag": "conv_fwd_h2_halo64k", "kernel": "h2k", "tile": (256, 64), "ksplit": 3}
    assert R.expected_launch("k32_split48") == {"tag": "conv_fwd_h2_halo64k", "kernel": "h2k", "tile": (256, 48), "ksplit": 3}
    assert R.expected_launch("k32_n48")["tile"] == (256, 48) and R.expected_launch("k32_n48@n64")["tile"] == (256, 64)
    assert R.expected_launch("k32_halo3")["tile"] == (256, 48) and R.GEOMS["k32_halo3"][4] % 64 != 0
    assert R.GEOMS["1x1_m49062"][1] * R.GEOMS["1x1_m49062"][2] % 256 == 166
    for name, flag in (("5x5_m4095", "pertap_split"), ("halo_cin16", "k16_192"), ("k32_64", "k32_64"), ("k32_split48", "k32_48_split")):
        assert "epi" in R.CASES[name][10] and R.CASES[name][8] == flag                 # one per-tap split, one k16 halo, one K32, one K32 K split


def test_overflow_setup_raises_one_element():
    name = next(n for n, c in R.CASES.items() if "ovf" in c[10])
    res, scale, want = R.overflow_setup(name)
    over = (want.double().abs() * scale) > R.F16_MAX
    assert int(over.sum()) == 1 and float((want.double().abs() * scale).max()) == 65536.0
    assert int((res != R.case(name, "exact")["res"]).sum()) == 1
