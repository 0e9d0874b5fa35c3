"""GPU checks of the MX transposed convolution (include/rdo_ptq_mxtconv.h) against tests/mx_tconv_reference.py: exact products for all
25 format pairs and over geometries (phases of 4, 2, 2 and 1 taps, K steps that straddle taps, an N tail, stride 1, k = s, stride 3
with bias-only rows, 4x4 stride 2, k < s with tapless phases; batch > 1 with non-zero data everywhere, which is what catches a tap that
reads the neighbouring image or row), bit-equality with `mx_gemm` on every phase's gathered operands -- the K order is a contract --,
random products within the header's bound, `mx.native_tconv` on a module (round to nearest and learned rounding) and
`QuantModel.mx_native_report(tconvs=True)`.

The allowed difference of a random product is the header's, derived in tests/test_gpu_mx_gemm.py and taken over with K the elements of
the output pixel's gathered row: |y - ref| <= K 2^-23 (sum |a b| + |bias|), elementwise.  Measured on the MI355X, max |y - ref| /
(sum |a b| + |bias|) at (2, 4, 5, 64, 37, 5, 2, 2, 1) and (1, 3, 3, 32, 16, 3, 2, 1, 1), activations x weights:
  mxfp8_e4m3 x mxfp8_e4m3   3.71e-08, 3.65e-08      mxfp4 x mxfp8_e4m3   4.22e-08, 3.99e-08
  mxfp8_e5m2 x mxfp6_e2m3   2.97e-08, 3.57e-08      mxfp4 x mxfp4        2.99e-08, 3.99e-08
against bounds K 2^-23 of 3.1e-5 to 6.9e-5 and 3.8e-6 to 1.5e-5; the report's 5x5 stride-2 row has rel_l2 0 against the emulation
(cap 1.6e-4)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mx_gemm_reference as G
import mx_reference as R
import mx_tconv_reference as TR
from test_mx_tconv_args import AQ, WQ, forward_model

pytestmark = pytest.mark.gpu

BIT_PAIRS = (("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp6_e2m3"), ("mxfp4", "mxfp4"))     # (x, w)
BIT_GEOMETRIES = (TR.GEOMETRIES[0], TR.PAIRS_GEOMETRY)                                  # the 5x5 and the 3x3 at stride 2
MODULE_GEOMETRY = (2, 3, 4, 32, 16, 5, 2, 2, 1)


def _operand(codes, scales, fmt):
    from hipops import ops
    return ops.mx_pack_codes(G.to_torch(codes).cuda(), G.to_torch(scales).cuda(), fmt)


# ----------------------------------------------------------------------------- exact products
def _exact(fx, fw, geometry, seed):
    from hipops import ops
    B, H, W, C, N, k, s, pad, op = geometry
    c = TR.exact_tconv_case(fx, fw, geometry, seed)
    x, w = _operand(c["x_codes"], c["x_scales"], fx), _operand(c["w_codes"], c["w_scales"], fw)
    y = ops.mx_conv_transpose2d(x, w, (B, H, W), k, s, pad, op, G.to_torch(c["bias"]).cuda())
    Ho, Wo = TR.out_size(H, k, s, pad, op), TR.out_size(W, k, s, pad, op)
    assert tuple(y.shape) == (B, Ho, Wo, N) and y.dtype == torch.float32 and y.is_contiguous()
    got = y.reshape(-1, N).cpu().numpy().astype(np.float64)
    wrong = np.argwhere(got != c["ref"])
    assert wrong.size == 0, (fx, fw, geometry, len(wrong), wrong[:8].tolist())
    y0 = ops.mx_conv_transpose2d(x, w, (B, H, W), k, s, pad, op).reshape(-1, N)
    assert (y0.cpu().numpy().astype(np.float64) == c["ref"] - c["bias"].astype(np.float64)[None, :]).all()


@pytest.mark.parametrize("fw", R.NAMES)
@pytest.mark.parametrize("fx", R.NAMES)
def test_exact_product_for_every_format_pair(fx, fw):
    _exact(fx, fw, TR.PAIRS_GEOMETRY, seed=300 + R.NAMES.index(fx) * 5 + R.NAMES.index(fw))


@pytest.mark.parametrize("geometry", TR.GEOMETRIES)
@pytest.mark.parametrize("pair", TR.EXACT_PAIRS)
def test_exact_product_over_geometries(pair, geometry):
    _exact(*pair, geometry, seed=400 + TR.EXACT_PAIRS.index(pair) * 8 + TR.GEOMETRIES.index(geometry))


# ----------------------------------------------------------------------------- random data: the GEMM's bits, the derived bound
_RANDOM = {}


def _random_case(fx, fw, geometry):
    """Student-t activations through `mx_quant_pack`, Student-t weights through `mx_fakequant` + `mx_pack_codes`, a bias; made once per
    (pair, geometry) and shared, unchanged, by the two tests below"""
    from hipops import ops
    key = (fx, fw, geometry)
    if key not in _RANDOM:
        B, H, W, C, N, k, s, pad, op = geometry
        torch.manual_seed(11 + sum(geometry))
        t = torch.distributions.StudentT(3.0)
        x = (t.sample((B * H * W, C)) * 0.01).float().contiguous()
        w = (t.sample((N, k * k * C)) * 0.03).float().contiguous()
        bias = (torch.randn(N) * 0.01).float()
        a, xq = ops.mx_quant_pack(x.cuda(), fx, want_xq=True)
        q = ops.mx_fakequant(w.cuda(), fw, want=("codes", "scales", "wq"))
        b = ops.mx_pack_codes(q["codes"], q["scales"], fw)
        y = ops.mx_conv_transpose2d(a, b, (B, H, W), k, s, pad, op, bias.cuda())
        _RANDOM[key] = dict(a=a, b=b, bias=bias, y=y, xq=xq, x_codes=ops.mx_unpack_codes(a).cpu().numpy(), x_scales=a.scales.cpu().numpy(),
                            w_codes=ops.mx_unpack_codes(b).cpu().numpy(), w_scales=q["scales"].cpu().numpy(), wq=q["wq"])
    return _RANDOM[key]


@pytest.mark.parametrize("geometry", BIT_GEOMETRIES)
@pytest.mark.parametrize("fx,fw", BIT_PAIRS)
def test_bit_equal_to_the_gemm_on_the_gathered_operands_of_every_phase(fx, fw, geometry):
    """gathered operands through mx_unpack_codes -> index -> mx_pack_codes"""
    from hipops import ops
    B, H, W, C, N, k, s, pad, op = geometry
    c = _random_case(fx, fw, geometry)
    y = c["y"].reshape(-1, N)
    y0 = ops.mx_conv_transpose2d(c["a"], c["b"], (B, H, W), k, s, pad, op).reshape(-1, N)
    bias = c["bias"].cuda()
    phases = TR.phases(B, H, W, k, s, pad, op)
    assert len(phases) == s * s and sum(len(p["pixels"]) for p in phases) == y.shape[0]
    padded = False
    for ph in phases:
        assert ph["taps"], "every phase of these geometries has taps"
        ac, asc = TR.gathered_activation(c["x_codes"], c["x_scales"], ph)
        wc, ws = TR.gathered_weight(c["w_codes"], ph, k, C), TR.gathered_weight(c["w_scales"], ph, k, C // 32)
        padded = padded or bool((asc == 127).any())
        ga, gb = _operand(ac, asc, fx), _operand(wc, ws, fw)
        at = torch.from_numpy(ph["pixels"]).cuda()
        assert torch.equal(y[at].view(torch.int32), ops.mx_gemm(ga, gb, bias).view(torch.int32)), (ph["ry"], ph["rx"])
        assert torch.equal(y0[at].view(torch.int32), ops.mx_gemm(ga, gb).view(torch.int32)), (ph["ry"], ph["rx"])
    assert padded


@pytest.mark.parametrize("geometry", BIT_GEOMETRIES)
@pytest.mark.parametrize("fx,fw", BIT_PAIRS)
def test_random_product_stays_within_the_derived_bound(fx, fw, geometry):
    B, H, W, C, N, k, s, pad, op = geometry
    c = _random_case(fx, fw, geometry)
    x64, w64 = G.decode(c["x_codes"], c["x_scales"], fx), G.decode(c["w_codes"], c["w_scales"], fw)
    assert (x64 == c["xq"].cpu().double().numpy()).all() and (w64 == c["wq"].cpu().double().numpy()).all()
    bias = c["bias"].numpy()
    ref = TR.tconv64(c["x_codes"], c["x_scales"], fx, c["w_codes"], c["w_scales"], fw, geometry, bias)
    assert (ref == TR.values64(x64, w64, geometry, bias)).all()
    sab, K = TR.abs_tconv64(x64, w64, geometry, bias)
    assert K.max() == (-(-k // s)) ** 2 * C
    tol = K[:, None] * 2.0 ** -23 * sab
    y = c["y"].reshape(-1, N).cpu().numpy().astype(np.float64)
    print(f"mx_conv_transpose2d {fx} x {fw} {geometry}: max |y - ref| / (sum|ab| + |bias|) = {np.max(np.abs(y - ref) / sab):.3e}, "
          f"bound K 2^-23 from {K.min() * 2.0 ** -23:.3e} to {K.max() * 2.0 ** -23:.3e}")
    assert np.isfinite(y).all() and (np.abs(y - ref) <= tol).all(), float(np.max(np.abs(y - ref) / np.maximum(tol, 1e-300)))


# ----------------------------------------------------------------------------- module level
def _module(org, fmt, learned):
    from quantization import QuantModule
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer
    m = QuantModule(org, WQ, AQ).cuda()
    m.weight_quantizer = (MXAdaRoundQuantizer if learned else MXQuantizer)(fmt, tconv=True).cuda()
    m.set_quant_state(True, False)
    return m


@pytest.mark.parametrize("learned", [False, True])
def test_native_tconv_on_a_module(learned):
    from hipops import ops
    from quantization.mx import native_tconv, native_tconv_operand
    from quantization.quantizer import to_rows
    torch.manual_seed(23)
    fmt = "mxfp4"
    geometry = MODULE_GEOMETRY
    B, H, W, C, N, k, s, pad, op = geometry
    m = _module(nn.ConvTranspose2d(C, N, k, stride=s, padding=pad, output_padding=op), fmt, learned)
    x = torch.randn(B, C, H, W).cuda()
    K = k * k * C
    if learned:
        g = torch.Generator().manual_seed(5)
        m.weight_quantizer.alpha = (torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1).cuda()     # a hand-set sign pattern: up or down
    y = native_tconv(m, x, fmt)
    Ho, Wo = TR.out_size(H, k, s, pad, op), TR.out_size(W, k, s, pad, op)
    assert tuple(y.shape) == (B, N, Ho, Wo) and y.permute(0, 2, 3, 1).is_contiguous()
    y2 = y.permute(0, 2, 3, 1).reshape(-1, N).cpu().numpy().astype(np.float64)
    # the forwarded weight along to_rows(., tconv=True): what the module's own quantised forward multiplies with
    wq = m.weight_quantizer(m.weight).detach()
    wf = to_rows(wq, True).reshape(N, K).cpu().double().numpy()
    if learned:
        rtn = ops.mx_fakequant(to_rows(m.weight.detach(), True).reshape(N, K).contiguous(), fmt)["wq"].cpu().double().numpy()
        assert 0.2 < float((wf != rtn).mean()) < 0.8                                  # the learned rounding moved about half of them
    opnd = native_tconv_operand(m)
    assert (opnd.rows, opnd.K, opnd.fmt) == (N, K, fmt)
    assert (G.decode(ops.mx_unpack_codes(opnd).cpu().numpy(), opnd.scales.cpu().numpy(), fmt) == wf).all()
    assert native_tconv_operand(m) is opnd and list(m._pack_memo) == ["mx_native_tconv"]   # memoised under its own key, reused by the call ...
    assert torch.equal(native_tconv(m, x, fmt), y) and native_tconv_operand(m) is opnd
    m.drop_weight_pack()
    assert m._pack_memo == {} and native_tconv_operand(m) is not opnd                  # ... and dropped with the weight pack
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    _, xq = ops.mx_quant_pack(rows, fmt, want_xq=True)
    x64 = xq.cpu().double().numpy()
    bias = m.bias.detach().cpu().numpy()
    ref = TR.values64(x64, wf, geometry, bias)
    sab, Kp = TR.abs_tconv64(x64, wf, geometry, bias)
    assert (np.abs(y2 - ref) <= Kp[:, None] * 2.0 ** -23 * sab).all()
    # ... which is torch's float64 transposed convolution of xq with the forwarded weight
    want = torch.nn.functional.conv_transpose2d(xq.cpu().double().reshape(B, H, W, C).permute(0, 3, 1, 2), wq.cpu().double(),
                                                m.bias.detach().cpu().double(), stride=s, padding=pad, output_padding=op)
    want = want.permute(0, 2, 3, 1).reshape(-1, N).numpy()
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# ----------------------------------------------------------------------------- the report
def _state(mods):
    return [(id(m.weight_quantizer), id(m.act_quantizer), m.use_weight_quant, m.use_act_quant, m.trained, len(m._forward_pre_hooks),
             len(m._forward_hooks)) for m in mods]


def test_report_with_tconvs():
    from hipops import ops
    from quantization import QuantModule
    from quantization import mx
    fmt = "mxfp6_e2m3"
    qnn = forward_model().cuda()
    qnn.set_weight_format(fmt)
    qnn.set_quant_state(True, False)
    mods = [m for m in qnn.modules() if isinstance(m, QuantModule)]
    before = _state(mods)
    torch.manual_seed(29)
    images = torch.rand(2, 3, 8, 8)
    seen = []
    up = qnn.model.up
    h = up.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    try:
        rep = qnn.mx_native_report(images, act_fmt=fmt, batch=2, convs=True, tconvs=True)
    finally:
        h.remove()
    assert list(rep["modules"]) == ["conv", "up", "head", "fc"] and list(rep["skipped"]) == ["stem"]
    row = rep["modules"]["up"]
    assert (row["unit"], row["rows"], row["K"], row["N"], row["w_fmt"], row["act_fmt"]) == ("up", 2 * 16 * 16, 25 * 32, 32, fmt, fmt)
    assert (row["k"], row["stride"], row["pad"], row["output_padding"]) == (5, 2, 2, 1)
    assert set(row) == {"unit", "rows", "K", "N", "w_fmt", "act_fmt", "max_abs_diff", "rel_l2", "act_sqnr_db", "k", "stride", "pad", "output_padding"}
    assert "output_padding" not in rep["modules"]["conv"] and rep["modules"]["conv"]["k"] == 3
    assert np.isfinite(row["rel_l2"]) and np.isfinite(row["max_abs_diff"]) and 10.0 < row["act_sqnr_db"] < 60.0
    # what the bound allows, from the same tensors: |K_p 2^-23 (sum |a b| + |bias|)| / |emulated|
    assert len(seen) == 1 and tuple(seen[0].shape) == (2, 32, 8, 8)
    geometry = (2, 8, 8, 32, 32, 5, 2, 2, 1)
    rows = seen[0].permute(0, 2, 3, 1).reshape(-1, 32).contiguous()
    _, xq = ops.mx_quant_pack(rows, fmt, want_xq=True)
    b = mx.native_tconv_operand(up)
    x64 = xq.cpu().double().numpy()
    w64 = G.decode(ops.mx_unpack_codes(b).cpu().numpy(), b.scales.cpu().numpy(), fmt)
    bias = up.bias.detach().cpu().numpy()
    exact = TR.values64(x64, w64, geometry, bias)
    sab, Kp = TR.abs_tconv64(x64, w64, geometry, bias)
    native = mx.native_tconv(up, seen[0], fmt).permute(0, 2, 3, 1).reshape(-1, 32).cpu().double().numpy()
    assert (np.abs(native - exact) <= Kp[:, None] * 2.0 ** -23 * sab).all()
    emulated = ops.conv_transpose2d(xq.reshape(2, 8, 8, 32), None, None, 2, 2, 1, pack=ops.WeightPack(
        ops.mx_dequant(ops.mx_unpack_codes(b), b.scales, b.K, b.fmt).reshape(32, 5, 5, 32), up.bias.detach().contiguous()))
    emulated = emulated.reshape(-1, 32).cpu().double().numpy()
    assert row["rel_l2"] == pytest.approx(np.linalg.norm(native - emulated) / np.linalg.norm(emulated), rel=1e-9, abs=1e-300)
    assert row["max_abs_diff"] == float(np.abs(native - emulated).max())
    cap = np.linalg.norm(Kp[:, None] * 2.0 ** -23 * sab) / np.linalg.norm(emulated)
    print(f"mx_native_report(tconvs=True): 5x5 stride-2 rel_l2 {row['rel_l2']:.3e}, cap {cap:.3e}, native vs exact "
          f"{np.linalg.norm(native - exact) / np.linalg.norm(exact):.3e}")
    assert row["rel_l2"] <= cap
    assert _state(mods) == before
    # tconvs=False: key for key the report as it was
    old = qnn.mx_native_report(images, act_fmt=fmt, batch=2, convs=True)
    same = qnn.mx_native_report(images, act_fmt=fmt, batch=2, convs=True, tconvs=False)
    assert list(same) == list(old) == ["modules", "skipped", "act_fmt", "n", "batch"] and same["skipped"] == old["skipped"]
    assert list(old["modules"]) == ["conv", "head", "fc"] and list(old["skipped"]) == ["stem", "up"]
    assert old["skipped"]["up"] == mx.native_refusal(up) and "a tconv module is not GEMM-shaped" in old["skipped"]["up"]
    for name in old["modules"]:
        assert set(same["modules"][name]) == set(old["modules"][name]) == set(rep["modules"][name])
        for key in ("unit", "rows", "K", "N", "w_fmt", "act_fmt", "act_sqnr_db", "rel_l2", "max_abs_diff"):
            assert same["modules"][name][key] == old["modules"][name][key] == rep["modules"][name][key], (name, key)
    plain = qnn.mx_native_report(images, act_fmt=fmt, batch=2)
    assert list(plain["modules"]) == ["head", "fc"] and list(plain["skipped"]) == ["stem", "conv", "up"]
    assert set(plain["modules"]["head"]) == {"unit", "rows", "K", "N", "w_fmt", "act_fmt", "max_abs_diff", "rel_l2", "act_sqnr_db"}
    assert _state(mods) == before
