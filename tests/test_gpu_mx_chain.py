"""GPU checks of the packed-output MX kernels (include/rdo_ptq_mxchain.h): the codes and scale bytes against float64 products that are
exact in fp32 (tests/mx_conv_reference.py) pushed through numpy's float32 activation and tests/mx_reference.py's quantiser; the packed
bytes against the un-fused path -- fp32 entry, `ops.lrelu`, `ops.mx_quant_pack` -- on heavy-tailed data for the GEMM, the convolution
and the transposed convolution; and `QuantRB` / `QuantRBWS` blocks chained against un-chained.  Every comparison is for equal bits."""
import numpy as np
import pytest
import torch

import mx_conv_reference as CR
import mx_gemm_reference as G
import mx_reference as R
from test_mx_chain_args import block_model

pytestmark = pytest.mark.gpu

ACTS = {"none": lambda v: v, "relu": lambda v: np.where(v > 0, v, np.float32(0)), "lrelu": lambda v: np.where(v > 0, v, np.float32(0.01) * v)}
# (B, H, W, C, N, k, stride, pad): M = 70 with a 6-row last tile and one wave column; M = 20 < 32 and N = 96, a half-filled second
# column of tiles
GEOMETRIES = ((2, 5, 7, 32, 32, 3, 1, 1), (1, 7, 9, 64, 96, 3, 2, 1))
EXACT = [("mxfp4", "mxfp4", o, a) for o in R.NAMES for a in ACTS] + [("mxfp8_e4m3", "mxfp6_e2m3", "mxfp8_e4m3", "lrelu")]
_CASES = {}


def _operand(codes, scales, fmt):
    from hipops import ops
    return ops.mx_pack_codes(G.to_torch(codes).cuda(), G.to_torch(scales).cuda(), fmt)


def _exact_case(fx, fw, geometry):
    """the exact-product inputs, made once per (pair, geometry) and shared unchanged"""
    key = (fx, fw, geometry)
    if key not in _CASES:
        c = CR.exact_conv_case(fx, fw, geometry, seed=700 + sum(geometry))
        _CASES[key] = (c, _operand(c["x_codes"], c["x_scales"], fx), _operand(c["w_codes"], c["w_scales"], fw))
    return _CASES[key]


def _check_exact(fx, fw, out_fmt, act, geometry, bias=None):
    from hipops import ops
    B, H, W, _, N, k, stride, pad = geometry
    c, x, w = _exact_case(fx, fw, geometry)
    ref = c["ref"] if bias is None else c["ref"] - c["bias"].astype(np.float64)[None, :] + bias.astype(np.float64)[None, :]
    v = ref.astype(np.float32)
    assert (v.astype(np.float64) == ref).all()                                          # the accumulator + bias: exact in fp32
    want = R.quantize(torch.from_numpy(ACTS[act](v)), out_fmt)
    got = ops.mx_conv2d(x, w, (B, H, W), k, stride, pad, G.to_torch(c["bias"] if bias is None else bias).cuda(), out_fmt=out_fmt, act=act)
    assert (got.fmt, got.rows, got.K) == (out_fmt, ref.shape[0], N)
    assert torch.equal(got.scales.cpu(), want["scales"]) and torch.equal(ops.mx_unpack_codes(got).cpu(), want["codes"])
    return got


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("fx,fw,out_fmt,act", EXACT)
def test_codes_and_scales_of_exact_products(fx, fw, out_fmt, act, geometry):
    _check_exact(fx, fw, out_fmt, act, geometry)


def test_relu_of_a_negative_block_is_scale_zero_and_zero_codes():
    from hipops import ops
    c, _, _ = _exact_case("mxfp4", "mxfp4", GEOMETRIES[1])
    bias = c["bias"].copy()
    bias[:32] = -2.0 ** 17                                                              # |conv| <= 144 K = 82944: channels 0 .. 31 < 0
    got = _check_exact("mxfp4", "mxfp4", "mxfp6_e3m2", "relu", GEOMETRIES[1], bias)
    assert not got.scales[:, 0].any() and not ops.mx_unpack_codes(got)[:, :32].any() and got.scales[:, 1:].any()


# ----------------------------------------------------------------------------- heavy-tailed data: the bytes of the two-launch path
PAIRS = (("mxfp4", "mxfp4", "mxfp4"), ("mxfp8_e4m3", "mxfp6_e3m2", "mxfp6_e2m3"))       # (x, w, out)
# gemm [M, K] x [N, K]; conv and tconv (B, H, W, C, N, k, stride, pad[, output padding]): tconv with all four phases and border taps,
# and k = 1 at stride 2, whose tapless phases hold act(bias)
SHAPES = {"gemm": (70, 192, 96), "conv": (2, 6, 7, 64, 64, 3, 1, 1), "tconv": (2, 4, 3, 32, 32, 5, 2, 2, 1), "tconv1": (2, 4, 3, 32, 32, 1, 2, 0, 1)}


def _random_case(kind, fx, fw):
    from hipops import ops
    key = (kind, fx, fw)
    if key not in _CASES:
        s = SHAPES[kind]
        rows, K, N, wk = (s[0], s[1], s[2], s[1]) if kind == "gemm" else (s[0] * s[1] * s[2], s[3], s[4], s[5] * s[5] * s[3])
        torch.manual_seed(17 + sum(s))
        t = torch.distributions.StudentT(3.0)
        x = ops.mx_quant_pack((t.sample((rows, K)) * 0.05).float().cuda().contiguous(), fx)
        q = ops.mx_fakequant((t.sample((N, wk)) * 0.05).float().cuda().contiguous(), fw, want=("codes", "scales"))
        _CASES[key] = (x, ops.mx_pack_codes(q["codes"], q["scales"], fw), (torch.randn(N) * 0.05).cuda())
    return _CASES[key]


@pytest.mark.parametrize("act", ("none", "lrelu"))
@pytest.mark.parametrize("fx,fw,out_fmt", PAIRS)
@pytest.mark.parametrize("kind", SHAPES)
def test_packed_bytes_equal_the_two_launch_path(kind, fx, fw, out_fmt, act):
    from hipops import ops
    x, w, bias = _random_case(kind, fx, fw)
    s = SHAPES[kind]
    if kind == "gemm":
        call = lambda **kw: ops.mx_gemm(x, w, bias, **kw)
    elif kind == "conv":
        call = lambda **kw: ops.mx_conv2d(x, w, s[:3], s[5], s[6], s[7], bias, **kw)
    else:
        call = lambda **kw: ops.mx_conv_transpose2d(x, w, s[:3], s[5], s[6], s[7], s[8], bias, **kw)
    y = call()
    want = ops.mx_quant_pack((ops.lrelu(y) if act == "lrelu" else y).reshape(-1, y.shape[-1]), out_fmt)
    got = call(out_fmt=out_fmt, act=act)
    assert (got.rows, got.K) == (want.rows, want.K) and float(y.min()) < 0 < float(y.max())
    assert torch.equal(got.scales, want.scales) and torch.equal(got.packed, want.packed)


# ----------------------------------------------------------------------------- the blocks
def test_chained_blocks_give_the_bits_of_the_unchained_ones():
    qnn = block_model().cuda()
    qnn.set_weight_format("mxfp4")
    qnn.set_quant_state(True, False)
    torch.manual_seed(43)
    x = torch.randn(2, 32, 6, 7).cuda()
    outs = {}
    for chain in (False, True):
        rep = qnn.set_mx_activations("mxfp8_e4m3", "native", chain=chain)
        assert dict(rep.get("chained", {})) == ({"0": ("0.conv1", "0.conv2"), "1": ("1.conv1", "1.conv2")} if chain else {})
        with torch.no_grad():
            outs[chain] = (qnn.model[0](x).clone(), qnn.model[1](x).clone())
    assert tuple(outs[True][1].shape) == (2, 32, 3, 4)
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
    # the block's activation quantiser active between the convs: the present path, whatever `mx_chain` says
    for b in qnn.model:
        b.trained = True
    qnn.set_quant_state(True, True)
    with torch.no_grad():
        active = qnn.model[0](x).clone()
        qnn.set_mx_activations("mxfp8_e4m3", "native", chain=False)
        assert torch.equal(active, qnn.model[0](x)) and not torch.equal(active, outs[True][0])
