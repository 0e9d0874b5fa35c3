"""CPU checks of the MX convolution: include/rdo_ptq_mxconv.h against `EXPORTS_MXCONV` and the built library, `rdo_mx_conv2d_out_pixels`,
the refusals of the C entry (RDO_EINVAL without touching a device) and of `ops.mx_conv2d`, the eligibility table of
`mx.native_conv_refusal`, `native_conv` and `mx_native_report(convs=...)` up to the point where a kernel would run, and the reference's
own convolution (tests/mx_conv_reference.py) against torch's float64 conv2d."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import mx_conv_reference as CR
import mx_gemm_reference as G
import mx_reference as R

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rdo_mx_conv2d_out_pixels", "rdo_mx_conv2d"}
WQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
AQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}


def three_layer_model():
    """a stem that is not eligible (3 channels), an eligible 3x3 conv and an eligible 1x1 conv"""
    from quantization import QuantModel
    torch.manual_seed(13)
    net = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv2d(32, 32, 3, padding=1), nn.LeakyReLU(0.01),
                        nn.Conv2d(32, 16, 1))
    return QuantModel(net.eval(), WQ, AQ).eval()


# ----------------------------------------------------------------------------- the header, the exports
def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxconv.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXCONV) == NAMES
    assert '#include "rdo_ptq_mxgemm.h"' in hdr
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_BIAS, L.EXPORTS_BITS, L.EXPORTS_PACK, L.EXPORTS_SUBPEL, L.EXPORTS_ACTBITS, L.EXPORTS_ATTNQ,
              L.EXPORTS_MX, L.EXPORTS_MXROUND, L.EXPORTS_MXGEMM)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert len(L.EXPORTS) == 124 and len(L.EXPORTS_MXGEMM) == 5


def test_out_pixels():
    from hipops import _lib as L
    f = L.lib().rdo_mx_conv2d_out_pixels
    for B, H, W, _, _, k, stride, pad in (CR.PAIRS_GEOMETRY,) + CR.GEOMETRIES + CR.MODULE_GEOMETRIES:
        want = B * CR.out_size(H, k, stride, pad) * CR.out_size(W, k, stride, pad)
        assert f(B, H, W, k, stride, pad) == want == CR.im2col_index(B, H, W, k, stride, pad).shape[0]
    assert f(4, 128, 128, 3, 1, 1) == 4 * 128 * 128 and f(4, 128, 128, 5, 2, 2) == 4 * 64 * 64 and f(1, 3, 3, 3, 1, 0) == 1
    assert f(1, 1, 1, 5, 7, 2) == 1 and f(1, 2 ** 15, 2 ** 16 - 1, 1, 1, 0) == 2 ** 31 - 2 ** 15
    zeros = [(0, 4, 4, 3, 1, 1), (-1, 4, 4, 3, 1, 1), (1, 0, 4, 3, 1, 1), (1, 4, -2, 3, 1, 1), (1, 4, 4, 0, 1, 1), (1, 4, 4, 3, 0, 1),
             (1, 4, 4, 3, -1, 1), (1, 4, 4, 3, 1, -1), (1, 2, 4, 3, 1, 0), (1, 4, 2, 3, 1, 0), (1, 4, 4, 7, 1, 1),
             (2, 2 ** 15, 2 ** 15, 1, 1, 0),                                           # B H W = 2^31
             (1, 2 ** 15, 2 ** 15, 1, 1, 2 ** 14),                                     # the input fits, the padded output does not
             (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1, 1, 2 ** 31 - 1)]
    for g in zeros:
        assert f(*g) == 0, g


def test_c_entry_refuses_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    odd = C.c_void_p(C.addressof(buf) + 2)
    names = ["x", "sx", "fx", "w", "sw", "fw", "B", "H", "W", "C", "N", "k", "stride", "pad", "bias", "y"]
    base = dict(x=p, sx=p, fx=0, w=p, sw=p, fw=3, B=2, H=5, W=7, C=64, N=24, k=3, stride=1, pad=1, bias=None, y=p)
    bad = [dict(x=None), dict(sx=None), dict(w=None), dict(sw=None), dict(y=None),
           dict(x=odd), dict(w=odd), dict(bias=odd), dict(y=odd),
           dict(fx=-1), dict(fx=5), dict(fw=-1), dict(fw=5),
           dict(B=0), dict(B=-1), dict(H=0), dict(H=-4), dict(W=0), dict(W=-4), dict(C=0), dict(C=-32), dict(N=0), dict(N=-3),
           dict(k=0), dict(k=-3), dict(stride=0), dict(stride=-1), dict(pad=-1),
           dict(C=40), dict(C=3), dict(C=33),
           dict(H=2, pad=0), dict(W=2, pad=0), dict(k=9), dict(H=1, W=1, k=5, pad=1),
           dict(B=2, H=2 ** 15, W=2 ** 15, k=1, pad=0),                                  # B H W = 2^31
           dict(B=1, H=2 ** 15, W=2 ** 15, k=1, pad=2 ** 14),                            # B Ho Wo > 2^31 - 1
           dict(B=1, H=2 ** 15, W=2 ** 15, C=32 * 2 ** 11, k=1, pad=0),                  # 2^41 blocks in x
           dict(N=2 ** 31 - 1, C=32 * 2 ** 10),                                          # 9 x 2^10 x (2^31 - 1) blocks in w
           dict(H=2 ** 21, W=1, k=2 ** 21, pad=2 ** 20),                                 # a weight row of 2^42 blocks
           dict(B=1, H=2 ** 15, W=2 ** 16 - 1, C=32, N=4160, k=1, pad=0)]                # (2^25 - 2^9) x 65 output tiles
    for kw in bad:
        a = dict(base, **kw)
        assert h.rdo_mx_conv2d(*[a[n] for n in names], None) == RDO_EINVAL, kw
        assert h.rdo_last_error().startswith(b"rdo_mx_conv2d: "), (kw, h.rdo_last_error())


# ----------------------------------------------------------------------------- the wrapper
@pytest.fixture()
def no_library(monkeypatch):
    """any library call or pointer conversion after the argument checks fails the test"""
    from hipops import _lib as L
    from hipops import ops

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(ops, "_ptr", boom)
    return ops


def test_wrapper_refuses_malformed_arguments(no_library):
    ops = no_library
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    x = ops.MXOperand(u8(70, 2 * 16), u8(70, 2), "mxfp4", 70, 64)                       # [2 * 5 * 7, 64]
    w = ops.MXOperand(u8(24, 18 * 32), u8(24, 18), "mxfp8_e4m3", 24, 576)               # [24, 3 * 3 * 64]
    cases = [
        ((u8(70, 32), w, (2, 5, 7), 3), "mx_conv2d: x must be an MXOperand, got Tensor"),
        ((x, None, (2, 5, 7), 3), "mx_conv2d: w must be an MXOperand, got NoneType"),
        ((ops.MXOperand(u8(70, 32), u8(70, 1), "mxfp4", 70, 64), w, (2, 5, 7), 3), "mx_conv2d: x.scales must be a contiguous uint8 \\[70, 2\\]"),
        ((x, ops.MXOperand(u8(24, 18 * 32), u8(24, 18), "mxfp9", 24, 576), (2, 5, 7), 3), "mx_conv2d: unknown MX format 'mxfp9'"),
        ((x, ops.MXOperand(u8(24, 18 * 16), u8(24, 18), "mxfp8_e4m3", 24, 576), (2, 5, 7), 3), "mx_conv2d: w.packed must be a contiguous uint8 \\[24, 576\\]"),
        ((x, w, (2, 5), 3), "mx_conv2d: shape must be \\(B, H, W\\), got \\(2, 5\\)"),
        ((x, w, 70, 3), "mx_conv2d: shape must be \\(B, H, W\\), got 70"),
        ((x, w, (2, 5.0, 7), 3), "mx_conv2d: shape\\[1\\] must be a whole number >= 1, got 5.0"),
        ((x, w, (2, 0, 7), 3), "mx_conv2d: shape\\[1\\] must be a whole number >= 1, got 0"),
        ((x, w, (2, 5, 7), 0), "mx_conv2d: k must be a whole number >= 1, got 0"),
        ((x, w, (2, 5, 7), 3, 0), "mx_conv2d: stride must be a whole number >= 1, got 0"),
        ((x, w, (2, 5, 7), 3, True), "mx_conv2d: stride must be a whole number >= 1, got True"),
        ((x, w, (2, 5, 7), 3, 1, -1), "mx_conv2d: pad must be a whole number >= 0, got -1"),
        ((x, w, (2, 5, 8), 3), "mx_conv2d: x has 70 rows, shape \\(2, 5, 8\\) states 80 pixels"),
        ((x, w, (2, 5, 7), 5), "mx_conv2d: w has K = 576, a 5 x 5 kernel over x's 64 channels needs K = 1600"),
        ((ops.MXOperand(u8(4, 2 * 16), u8(4, 2), "mxfp4", 4, 64), w, (1, 2, 2), 3), "mx_conv2d: a 3 x 3 kernel does not fit the 2 x 2 input under padding 0"),
        ((x, w, (2, 5, 7), 3, 1, 1, torch.zeros(23)), "mx_conv2d: bias must be a contiguous fp32 \\[24\\]"),
        ((x, w, (2, 5, 7), 3, 1, 1, torch.zeros(24).double()), "mx_conv2d: bias must be a contiguous fp32 \\[24\\]"),
        ((x, w, (2, 5, 7), 3, 1, 1, torch.zeros(24)), "mx_conv2d: .*no CPU path"),
        ((x, w, (2, 5, 7), 3, 1, 1), "mx_conv2d: .*no CPU path"),
    ]
    for args, what in cases:
        with pytest.raises(ValueError, match=what):
            ops.mx_conv2d(*args)
    with pytest.raises(ValueError, match="mx_conv2d: w.packed must be a contiguous uint8 \\[24, 576\\] on meta"):
        ops.mx_conv2d(ops.MXOperand(u8(70, 32).to("meta"), u8(70, 2).to("meta"), "mxfp4", 70, 64), w, (2, 5, 7), 3)


# ----------------------------------------------------------------------------- native_conv_refusal, native_conv, the report
def _module(org, q=None):
    from quantization import QuantModule
    m = QuantModule(org, WQ, AQ)
    if q is not None:
        m.weight_quantizer = q
    return m


def test_native_conv_refuses_what_is_not_eligible():
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer, native_conv, native_conv_operand, native_conv_refusal
    not_square = "is not a square-kernel conv with one stride, one zero padding, dilation 1 and groups 1"
    cases = [
        (_module(nn.Conv2d(3, 32, 3, padding=1), MXQuantizer("mxfp4")), "its 3 input channels are no multiple of the MX block size 32"),
        (_module(nn.Conv2d(24, 8, 3, padding=1), MXAdaRoundQuantizer("mxfp6_e2m3")), "its 24 input channels are no multiple"),
        (_module(nn.Conv2d(32, 8, 3, padding=2, dilation=2), MXQuantizer("mxfp4")), f"dilation \\(2, 2\\), groups 1 {not_square}"),
        (_module(nn.Conv2d(64, 8, 3, padding=1, groups=2), MXQuantizer("mxfp4")), f"groups 2 {not_square}"),
        (_module(nn.ConvTranspose2d(32, 8, 3), MXQuantizer("mxfp4", tconv=True)), "a tconv module is not a convolution"),
        (_module(nn.Linear(64, 8), MXQuantizer("mxfp4")), "a linear module is not a convolution"),
        (_module(nn.Conv2d(32, 8, 3, padding=1)), "its weight quantiser is a UniformAffineQuantizer"),
        (_module(nn.Conv2d(32, 8, 3, stride=(2, 1), padding=1), MXQuantizer("mxfp4")), f"stride \\(2, 1\\).* {not_square}"),
        (_module(nn.Conv2d(32, 8, (3, 1)), MXQuantizer("mxfp4")), f"kernel \\(3, 1\\).* {not_square}"),
        (_module(nn.Conv2d(32, 8, 3, padding=(1, 0)), MXQuantizer("mxfp4")), f"padding \\(1, 0\\).* {not_square}"),
        # the order: kind, geometry, channels, quantiser
        (_module(nn.Conv2d(24, 8, 3, padding=1, dilation=2)), f"dilation \\(2, 2\\).* {not_square}"),
        (_module(nn.Conv2d(24, 8, 3, padding=1)), "its 24 input channels are no multiple"),
    ]
    for m, why in cases:
        assert re.search(why, native_conv_refusal(m)), (why, native_conv_refusal(m))
        with pytest.raises(ValueError, match=f"native_conv_operand: module QuantModule\\({m.kind}, .*{why}"):
            native_conv_operand(m)
        with pytest.raises(ValueError, match="native_conv_operand: module"):
            native_conv(m, torch.zeros(2, 32, 6, 7), "mxfp8_e4m3")
    # what is eligible goes on to the kernels, which have no CPU path
    for org, q, x in ((nn.Conv2d(64, 24, 3, padding=1), MXQuantizer("mxfp4"), torch.zeros(2, 64, 6, 7)),
                      (nn.Conv2d(32, 16, 5, stride=2, padding=2), MXAdaRoundQuantizer("mxfp8_e5m2"), torch.zeros(2, 32, 6, 7)),
                      (nn.Conv2d(32, 8, 1), MXQuantizer("mxfp6_e3m2"), torch.zeros(2, 32, 3, 3))):
        m = _module(org, q)
        assert native_conv_refusal(m) is None
        with pytest.raises(ValueError, match="mx_fakequant: .*no CPU path"):
            native_conv(m, x, "mxfp8_e4m3")
        assert m._pack_memo == {}
    m = _module(nn.Conv2d(64, 24, 3, padding=1), MXQuantizer("mxfp4"))
    with pytest.raises(ValueError, match="native_conv_operand: module"):
        native_conv(_module(nn.Linear(64, 8), MXQuantizer("mxfp4")), torch.zeros(2, 64), "mxfp4")


def test_report_refuses_a_convs_that_is_no_bool_before_any_gpu_work(monkeypatch):
    from hipops import ops
    qnn = three_layer_model()
    monkeypatch.setattr(ops, "_ptr", lambda *a, **k: (_ for _ in ()).throw(AssertionError("reached the library")))
    qnn.set_weight_format("mxfp4")
    images = torch.rand(2, 3, 16, 16)
    assert list(qnn.units()) == ["0", "2", "4"]
    for convs in ("yes", 1, None):
        with pytest.raises(ValueError, match="mx_native_report: convs must be True or False, got"):
            qnn.mx_native_report(images, convs=convs)
    # the named-unit refusal follows the flag: the 3x3 conv is eligible only with convs=True, the stem never
    with pytest.raises(ValueError, match="mx_native_report: unit '2' holds no eligible module: .*kernel \\(3, 3\\)"):
        qnn.mx_native_report(images, units=["2"])
    with pytest.raises(ValueError, match="mx_native_report: unit '0' holds no eligible module: .*its 3 input channels"):
        qnn.mx_native_report(images, units=["0"], convs=True)


# ----------------------------------------------------------------------------- the reference
def test_reference_index_and_operand():
    idx = CR.im2col_index(1, 3, 3, 3, 1, 1)
    assert idx.shape == (9, 9) and idx.dtype == np.int64
    assert idx[0].tolist() == [-1, -1, -1, -1, 0, 1, -1, 3, 4] and idx[4].tolist() == list(range(9)) and idx[8].tolist() == [4, 5, -1, 7, 8, -1, -1, -1, -1]
    idx = CR.im2col_index(2, 4, 5, 3, 2, 0)                                             # Ho = 1, Wo = 2: no padding, the second image
    assert idx.shape == (4, 9) and idx[3].tolist() == [22, 23, 24, 27, 28, 29, 32, 33, 34]
    codes = np.arange(1, 1 + 9 * 32, dtype=np.uint8).reshape(9, 32)
    scales = np.arange(100, 109, dtype=np.uint8).reshape(9, 1)
    c, s = CR.im2col_operand(codes, scales, CR.im2col_index(1, 3, 3, 3, 1, 1))
    assert c.shape == (9, 288) and s.shape == (9, 9) and c.dtype == s.dtype == np.uint8
    assert s[0].tolist() == [127, 127, 127, 127, 100, 101, 127, 103, 104] and (c[0, :128] == 0).all() and (c[0, 128:160] == codes[0]).all()
    assert (CR.im2col(codes.astype(np.float64), CR.im2col_index(1, 3, 3, 3, 1, 1))[8, 32:64] == codes[5]).all()


@pytest.mark.parametrize("geometry", (CR.PAIRS_GEOMETRY,) + CR.GEOMETRIES + CR.MODULE_GEOMETRIES)
def test_reference_conv64_is_torch_conv2d_in_float64(geometry):
    B, H, W, Cc, N, k, stride, pad = geometry
    fx, fw = "mxfp6_e2m3", "mxfp8_e4m3"
    c = CR.exact_conv_case(fx, fw, geometry, seed=sum(geometry))
    x = torch.from_numpy(G.decode(c["x_codes"], c["x_scales"], fx)).reshape(B, H, W, Cc).permute(0, 3, 1, 2)
    w = torch.from_numpy(G.decode(c["w_codes"], c["w_scales"], fw)).reshape(N, k, k, Cc).permute(0, 3, 1, 2)
    want = torch.nn.functional.conv2d(x, w, torch.from_numpy(c["bias"]).double(), stride=stride, padding=pad)
    assert want.dtype == torch.float64
    want = want.permute(0, 2, 3, 1).reshape(-1, N).numpy()
    # the exact case: every sum is exact in float64 whatever its order
    assert c["ref"].shape == want.shape and (c["ref"] == want).all()
    assert (c["ref"] * 16 == np.round(c["ref"] * 16)).all() and np.abs(c["ref"]).max() < 2.0 ** 20
    assert (c["x_codes"] != 0).any(axis=1).all()                                        # non-zero data at every pixel
    no_bias = CR.conv64(c["x_codes"], c["x_scales"], fx, c["w_codes"], c["w_scales"], fw, geometry)
    assert (no_bias == c["ref"] - c["bias"].astype(np.float64)[None, :]).all()


def test_exact_case_refuses_a_k_whose_sums_could_round():
    with pytest.raises(AssertionError):
        CR.exact_conv_case("mxfp4", "mxfp4", (1, 16, 16, 320, 8, 5, 1, 2), seed=0)      # K = 8000 > 7281
    assert all(2304 * g[5] * g[5] * g[3] + 128 < 2 ** 24 for g in (CR.PAIRS_GEOMETRY,) + CR.GEOMETRIES)
