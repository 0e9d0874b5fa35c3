"""GPU checks of the MX convolution (include/rdo_ptq_mxconv.h) against tests/mx_conv_reference.py: exact products for all 25 format
pairs and over geometries (taps that straddle K steps, M / N tails, strides, no padding, batch > 1 with non-zero data everywhere, which
is what catches a tap that reads the neighbouring image or row), bit-equality with `mx_gemm` on the im2col operand -- the K order is a
contract --, 1x1 as the GEMM itself, random products within the header's bound, `mx.native_conv` on modules (round to nearest and learned
rounding) and `QuantModel.mx_native_report(convs=True)`.

The allowed difference of a random product is the header's, derived in tests/test_gpu_mx_gemm.py and taken over with K = k k C:
|y - ref| <= K 2^-23 (sum |a b| + |bias|), elementwise.  Measured on the MI355X, max |y - ref| / sum |a b| of the random products next
to the reference's k-ordered fp32 chain, at (2, 5, 7, 96, 37, 3, 1, 1) and (2, 8, 6, 64, 16, 5, 2, 2), activations x weights:
  mxfp8_e4m3 x mxfp8_e4m3   3.60e-08 (chain 3.60e-08), 2.37e-08 (2.03e-08)      mxfp4 x mxfp8_e4m3   1.76e-08 (1.76e-08), 1.23e-08 (1.23e-08)
  mxfp8_e5m2 x mxfp6_e2m3   2.35e-08 (2.35e-08), 1.16e-08 (1.16e-08)            mxfp4 x mxfp4        1.83e-08 (1.83e-08), 7.83e-09 (7.83e-09)
against bounds K 2^-23 of 1.03e-4 and 1.91e-4; the report's 3x3 row has rel_l2 0 against the emulation (cap 2.6e-4)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mx_conv_reference as CR
import mx_gemm_reference as G
import mx_reference as R
from test_mx_conv_args import AQ, WQ, three_layer_model

pytestmark = pytest.mark.gpu

BIT_PAIRS = (("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp4", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp6_e2m3"), ("mxfp4", "mxfp4"))     # (x, w)
BIT_GEOMETRIES = (CR.GEOMETRIES[1], CR.GEOMETRIES[2])


def _operand(codes, scales, fmt):
    from hipops import ops
    return ops.mx_pack_codes(G.to_torch(codes).cuda(), G.to_torch(scales).cuda(), fmt)


def _bound(a64, b64, bias, K):
    tol = G.abs_product64(a64, b64)
    if bias is not None:
        tol = tol + np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return K * 2.0 ** -23 * tol


# ----------------------------------------------------------------------------- 1., 2. exact product
def _exact(fx, fw, geometry, seed):
    from hipops import ops
    B, H, W, C, N, k, stride, pad = geometry
    c = CR.exact_conv_case(fx, fw, geometry, seed)
    x, w = _operand(c["x_codes"], c["x_scales"], fx), _operand(c["w_codes"], c["w_scales"], fw)
    y = ops.mx_conv2d(x, w, (B, H, W), k, stride, pad, G.to_torch(c["bias"]).cuda())
    Ho, Wo = CR.out_size(H, k, stride, pad), CR.out_size(W, k, stride, pad)
    assert tuple(y.shape) == (B, Ho, Wo, N) and y.dtype == torch.float32 and y.is_contiguous()
    got = y.reshape(-1, N).cpu().numpy().astype(np.float64)
    wrong = np.argwhere(got != c["ref"])
    assert wrong.size == 0, (fx, fw, geometry, len(wrong), wrong[:8].tolist())
    y0 = ops.mx_conv2d(x, w, (B, H, W), k, stride, pad).reshape(-1, N)
    assert (y0.cpu().numpy().astype(np.float64) == c["ref"] - c["bias"].astype(np.float64)[None, :]).all()


@pytest.mark.parametrize("fw", R.NAMES)
@pytest.mark.parametrize("fx", R.NAMES)
def test_exact_product_for_every_format_pair(fx, fw):
    _exact(fx, fw, CR.PAIRS_GEOMETRY, seed=100 + R.NAMES.index(fx) * 5 + R.NAMES.index(fw))


@pytest.mark.parametrize("geometry", CR.GEOMETRIES)
@pytest.mark.parametrize("pair", G.EXACT_PAIRS)
def test_exact_product_over_geometries(pair, geometry):
    _exact(*pair, geometry, seed=200 + G.EXACT_PAIRS.index(pair) * 8 + CR.GEOMETRIES.index(geometry))


# ----------------------------------------------------------------------------- 3., 5. random data: the GEMM's bits, the derived bound
_RANDOM = {}


def _random_case(fx, fw, geometry):
    """Student-t activations through `mx_quant_pack`, Student-t weights through `mx_fakequant` + `mx_pack_codes`, a bias; made once per
    (pair, geometry) and shared, unchanged, by the two tests below"""
    from hipops import ops
    key = (fx, fw, geometry)
    if key not in _RANDOM:
        B, H, W, C, N, k, stride, pad = geometry
        torch.manual_seed(7 + sum(geometry))
        t = torch.distributions.StudentT(3.0)
        x = (t.sample((B * H * W, C)) * 0.01).float().contiguous()
        w = (t.sample((N, k * k * C)) * 0.03).float().contiguous()
        bias = (torch.randn(N) * 0.01).float()
        a, xq = ops.mx_quant_pack(x.cuda(), fx, want_xq=True)
        q = ops.mx_fakequant(w.cuda(), fw, want=("codes", "scales", "wq"))
        b = ops.mx_pack_codes(q["codes"], q["scales"], fw)
        y = ops.mx_conv2d(a, b, (B, H, W), k, stride, pad, bias.cuda())
        _RANDOM[key] = dict(a=a, b=b, bias=bias, y=y, xq=xq, x_codes=ops.mx_unpack_codes(a).cpu().numpy(), x_scales=a.scales.cpu().numpy(),
                            w_codes=q["codes"].cpu().numpy(), w_scales=q["scales"].cpu().numpy(), wq=q["wq"])
    return _RANDOM[key]


@pytest.mark.parametrize("geometry", BIT_GEOMETRIES)
@pytest.mark.parametrize("fx,fw", BIT_PAIRS)
def test_bit_equal_to_the_gemm_on_the_im2col_operand(fx, fw, geometry):
    from hipops import ops
    B, H, W, C, N, k, stride, pad = geometry
    c = _random_case(fx, fw, geometry)
    ic, isc = CR.im2col_operand(c["x_codes"], c["x_scales"], CR.im2col_index(B, H, W, k, stride, pad))
    M = ic.shape[0]
    assert (isc == 127).any() == (pad > 0) and ic.shape == (M, k * k * C)
    want = ops.mx_gemm(_operand(ic, isc, fx), c["b"], c["bias"].cuda())
    assert torch.equal(c["y"].reshape(M, N).view(torch.int32), want.view(torch.int32))
    y0 = ops.mx_conv2d(c["a"], c["b"], (B, H, W), k, stride, pad)
    assert torch.equal(y0.reshape(M, N).view(torch.int32), ops.mx_gemm(_operand(ic, isc, fx), c["b"]).view(torch.int32))


@pytest.mark.parametrize("fx,fw", BIT_PAIRS)
def test_one_by_one_is_the_gemm(fx, fw):
    from hipops import ops
    B, H, W, C, N = 3, 5, 5, 64, 33
    c = _random_case(fx, fw, (B, H, W, C, N, 1, 1, 0))
    want = ops.mx_gemm(c["a"], c["b"], c["bias"].cuda())
    assert torch.equal(c["y"].reshape(-1, N).view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("geometry", BIT_GEOMETRIES)
@pytest.mark.parametrize("fx,fw", BIT_PAIRS)
def test_random_product_stays_within_the_derived_bound(fx, fw, geometry):
    B, H, W, C, N, k, stride, pad = geometry
    K = k * k * C
    c = _random_case(fx, fw, geometry)
    idx = CR.im2col_index(B, H, W, k, stride, pad)
    ic, isc = CR.im2col_operand(c["x_codes"], c["x_scales"], idx)
    a64, b64 = G.decode(ic, isc, fx), G.decode(c["w_codes"], c["w_scales"], fw)
    assert (a64 == CR.im2col(c["xq"].cpu().double().numpy(), idx)).all() and (b64 == c["wq"].cpu().double().numpy()).all()
    bias = c["bias"].numpy()
    ref = CR.conv64(c["x_codes"], c["x_scales"], fx, c["w_codes"], c["w_scales"], fw, geometry, bias)
    assert (ref == G.product64(a64, b64, bias)).all()
    y = c["y"].reshape(-1, N).cpu().numpy().astype(np.float64)
    tol = _bound(a64, b64, bias, K)
    s = G.abs_product64(a64, b64)
    chain = G.chain32(a64, b64, bias).astype(np.float64)
    print(f"mx_conv2d {fx} x {fw} {geometry}: max |y - ref| / sum|ab| = {np.max(np.abs(y - ref) / s):.3e}, "
          f"k-ordered fp32 chain {np.max(np.abs(chain - ref) / s):.3e}")
    assert np.isfinite(y).all() and (np.abs(y - ref) <= tol).all(), float(np.max(np.abs(y - ref) / tol))


# ----------------------------------------------------------------------------- 6. module level
def _module(org, fmt, learned):
    from quantization import QuantModule
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer
    m = QuantModule(org, WQ, AQ).cuda()
    m.weight_quantizer = (MXAdaRoundQuantizer if learned else MXQuantizer)(fmt).cuda()
    m.set_quant_state(True, False)
    return m


@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("which", [0, 1])
def test_native_conv_on_a_module(which, learned):
    from hipops import ops
    from quantization.mx import native_conv, native_conv_operand
    from quantization.quantizer import to_rows
    torch.manual_seed(19 + which)
    w_fmt, a_fmt = "mxfp6_e2m3", "mxfp6_e2m3"
    geometry = CR.MODULE_GEOMETRIES[which]
    B, H, W, C, N, k, stride, pad = geometry
    m = _module(nn.Conv2d(C, N, k, stride=stride, padding=pad), w_fmt, learned)
    x = torch.randn(B, C, H, W).cuda()
    K = k * k * C
    if learned:
        g = torch.Generator().manual_seed(5)
        m.weight_quantizer.alpha = (torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1).cuda()     # a random sign pattern: up or down
    y = native_conv(m, x, a_fmt)
    Ho, Wo = CR.out_size(H, k, stride, pad), CR.out_size(W, k, stride, pad)
    assert tuple(y.shape) == (B, N, Ho, Wo) and y.permute(0, 2, 3, 1).is_contiguous()
    y2 = y.permute(0, 2, 3, 1).reshape(-1, N).cpu().numpy().astype(np.float64)
    # the forwarded weight in to_rows order: what the module's own quantised forward multiplies with
    wf = to_rows(m.weight_quantizer(m.weight).detach()).reshape(N, K).cpu().double().numpy()
    if learned:
        rtn = ops.mx_fakequant(to_rows(m.weight.detach()).reshape(N, K).contiguous(), w_fmt)["wq"].cpu().double().numpy()
        assert 0.2 < float((wf != rtn).mean()) < 0.8                                  # the learned rounding moved about half of them
    op = native_conv_operand(m)
    assert (op.rows, op.K, op.fmt) == (N, K, w_fmt)
    assert (G.decode(ops.mx_unpack_codes(op).cpu().numpy(), op.scales.cpu().numpy(), w_fmt) == wf).all()
    assert native_conv_operand(m) is op and "mx_native_conv" in m._pack_memo            # memoised under its own key ...
    m.drop_weight_pack()
    assert m._pack_memo == {} and native_conv_operand(m) is not op                      # ... and dropped with the weight pack
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    _, xq = ops.mx_quant_pack(rows, a_fmt, want_xq=True)
    a64 = CR.im2col(xq.cpu().double().numpy(), CR.im2col_index(B, H, W, k, stride, pad))
    bias = m.bias.detach().cpu().numpy()
    ref = G.product64(a64, wf, bias)
    assert (np.abs(y2 - ref) <= _bound(a64, wf, bias, K)).all()
    # ... which is torch's float64 convolution of xq with the forwarded weight
    want = torch.nn.functional.conv2d(xq.cpu().double().reshape(B, H, W, C).permute(0, 3, 1, 2), m.weight_quantizer(m.weight).detach().cpu().double(),
                                      m.bias.detach().cpu().double(), stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1, N).numpy()
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_a_one_by_one_module_shares_the_operand_of_native_operand():
    from quantization.mx import native_conv, native_conv_operand, native_linear, native_operand
    m = _module(nn.Conv2d(64, 24, 1), "mxfp4", False)
    op = native_conv_operand(m)
    assert op is native_operand(m) and native_conv_operand(m) is op and list(m._pack_memo) == ["mx_native"]
    torch.manual_seed(3)
    x = torch.randn(2, 64, 5, 7).cuda()
    assert torch.equal(native_conv(m, x, "mxfp8_e4m3"), native_linear(m, x, "mxfp8_e4m3"))


# ----------------------------------------------------------------------------- 7. the report
def _state(mods):
    return [(id(m.weight_quantizer), id(m.act_quantizer), m.use_weight_quant, m.use_act_quant, m.trained, len(m._forward_pre_hooks),
             len(m._forward_hooks)) for m in mods]


def test_report_with_convs():
    from hipops import _lib as L
    from hipops import ops
    from quantization import QuantModule
    from quantization import mx
    fmt = "mxfp6_e2m3"
    qnn = three_layer_model().cuda()
    qnn.set_weight_format(fmt)
    qnn.set_quant_state(True, False)
    mods = [m for m in qnn.modules() if isinstance(m, QuantModule)]
    before = _state(mods)
    torch.manual_seed(29)
    images = torch.rand(2, 3, 16, 16)
    seen = []
    mid = mods[1]
    h = mid.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    try:
        rep = qnn.mx_native_report(images, act_fmt=fmt, batch=2, convs=True)
    finally:
        h.remove()
    assert list(rep["modules"]) == ["2", "4"] and list(rep["skipped"]) == ["0"]
    assert "its 3 input channels are no multiple of the MX block size 32" in rep["skipped"]["0"]
    assert (rep["act_fmt"], rep["n"], rep["batch"]) == (fmt, 2, 2)
    row = rep["modules"]["2"]
    assert (row["unit"], row["rows"], row["K"], row["N"], row["w_fmt"], row["act_fmt"]) == ("2", 2 * 16 * 16, 288, 32, fmt, fmt)
    assert (row["k"], row["stride"], row["pad"]) == (3, 1, 1)
    one = rep["modules"]["4"]
    assert (one["rows"], one["K"], one["N"], one["k"], one["stride"], one["pad"]) == (2 * 16 * 16, 32, 16, 1, 1, 0)
    for r in (row, one):
        assert np.isfinite(r["rel_l2"]) and np.isfinite(r["max_abs_diff"]) and 10.0 < r["act_sqnr_db"] < 60.0
    # the bound's ratio from the same tensors: K 2^-23 |sum |a b|| / |emulated|
    assert len(seen) == 1 and tuple(seen[0].shape) == (2, 32, 16, 16)
    rows = seen[0].permute(0, 2, 3, 1).reshape(-1, 32).contiguous()
    a, xq = ops.mx_quant_pack(rows, fmt, want_xq=True)
    b = mx.native_conv_operand(mid)
    idx = CR.im2col_index(2, 16, 16, 3, 1, 1)
    a64 = CR.im2col(xq.cpu().double().numpy(), idx)
    b64 = G.decode(ops.mx_unpack_codes(b).cpu().numpy(), b.scales.cpu().numpy(), fmt)
    bias = mid.bias.detach().contiguous()
    wdec = ops.mx_dequant(ops.mx_unpack_codes(b), b.scales, b.K, b.fmt)
    emulated = ops.conv2d_fwd_pack(xq.reshape(2, 16, 16, 32), ops.WeightPack(wdec.reshape(32, 3, 3, 32), bias), 1, 1,
                                   epilogue=L.EPI_NONE).reshape(-1, 32).cpu().double().numpy()
    native = ops.mx_conv2d(a, b, (2, 16, 16), 3, 1, 1, bias).reshape(-1, 32).cpu().double().numpy()
    assert row["rel_l2"] == pytest.approx(np.linalg.norm(native - emulated) / np.linalg.norm(emulated), rel=1e-9, abs=1e-300)
    assert row["max_abs_diff"] == float(np.abs(native - emulated).max())
    exact = G.product64(a64, b64, bias.cpu().numpy())
    cap = 288 * 2.0 ** -23 * np.linalg.norm(G.abs_product64(a64, b64)) / np.linalg.norm(emulated)
    print(f"mx_native_report(convs=True): 3x3 rel_l2 {row['rel_l2']:.3e}, cap {cap:.3e}, emulated vs exact "
          f"{np.linalg.norm(emulated - exact) / np.linalg.norm(emulated):.3e}, native vs exact {np.linalg.norm(native - exact) / np.linalg.norm(emulated):.3e}")
    assert row["rel_l2"] <= cap
    x64 = rows.cpu().double().numpy()
    assert row["act_sqnr_db"] == pytest.approx(10 * np.log10((x64 ** 2).sum() / ((x64 - xq.cpu().double().numpy()) ** 2).sum()), rel=1e-9)
    assert _state(mods) == before
    # convs=False: the keys and the skip reasons of the report as it was
    old = qnn.mx_native_report(images, act_fmt=fmt, batch=2)
    same = qnn.mx_native_report(images, act_fmt=fmt, batch=2, convs=False)
    assert list(same) == list(old) and same["skipped"] == old["skipped"] and list(same["modules"]) == list(old["modules"])
    assert list(old) ==["modules", "skipped", "act_fmt", "n", "batch"]
    assert list(old["modules"]) == ["4"] and list(old["skipped"]) == ["0", "2"]
    assert set(old["modules"]["4"]) == {"unit", "rows", "K", "N", "w_fmt", "act_fmt", "max_abs_diff", "rel_l2", "act_sqnr_db"}
    for name in ("0", "2"):
        assert old["skipped"][name] == mx.native_refusal(mods[int(name) // 2]) and "kernel (3, 3)" in old["skipped"][name]
    # the 1x1 conv measured the conv way sees the same input and the same operand (the emulation may take another kernel for [B, H, W])
    for key in ("unit", "rows", "K", "N", "w_fmt", "act_fmt", "act_sqnr_db"):
        assert one[key] == old["modules"]["4"][key], key
    assert _state(mods) == before
    # the model is left as found also when a forward raises
    def boom(mod, args):
        raise RuntimeError("a forward raised")
    h = mods[0].register_forward_pre_hook(boom)
    try:
        with pytest.raises(RuntimeError, match="a forward raised"):
            qnn.mx_native_report(images, batch=1, convs=True)
    finally:
        h.remove()
    assert _state(mods) == before
