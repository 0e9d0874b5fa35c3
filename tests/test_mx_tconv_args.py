"""CPU checks of the MX transposed convolution and of the MX-activation forward mode: include/rdo_ptq_mxtconv.h against
`EXPORTS_MXTCONV` and the built library, `rdo_mx_conv_transpose2d_out_pixels`, the refusals of the C entry (RDO_EINVAL without touching
a device) and of `ops.mx_conv_transpose2d`, the eligibility table of `mx.native_tconv_refusal`, `native_tconv`,
`mx_native_report(tconvs=...)` and `QuantModel.set_mx_activations` up to the point where a kernel would run, the reconstruction
refusal, and the reference's own transposed convolution (tests/mx_tconv_reference.py) against torch's float64 conv_transpose2d."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import mx_gemm_reference as G
import mx_tconv_reference as TR

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rdo_mx_conv_transpose2d_out_pixels", "rdo_mx_conv_transpose2d"}
WQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
AQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}


class ForwardNet(nn.Module):
    """the model of the forward-mode tests: a 3-channel stem that is not eligible, an eligible 3x3 conv, a 5x5 stride-2 transposed conv,
    a 1x1 conv, and a Linear branch on the channel means"""

    def __init__(self):
        super().__init__()
        self.stem, self.act0 = nn.Conv2d(3, 32, 3, padding=1), nn.LeakyReLU(0.01)
        self.conv, self.act1 = nn.Conv2d(32, 32, 3, padding=1), nn.LeakyReLU(0.01)
        self.up = nn.ConvTranspose2d(32, 32, 5, stride=2, padding=2, output_padding=1)
        self.head = nn.Conv2d(32, 16, 1)
        self.fc = nn.Linear(32, 32)

    def forward(self, x):
        h = self.act1(self.conv(self.act0(self.stem(x))))
        return self.head(self.up(h)), self.fc(h.mean(dim=(2, 3)))


def forward_model():
    from quantization import QuantModel
    torch.manual_seed(31)
    return QuantModel(ForwardNet().eval(), WQ, AQ).eval()


# ----------------------------------------------------------------------------- the header, the exports
def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxtconv.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXTCONV) == NAMES
    assert '#include "rdo_ptq_mxgemm.h"' in hdr
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_BIAS, L.EXPORTS_BITS, L.EXPORTS_PACK, L.EXPORTS_SUBPEL, L.EXPORTS_ACTBITS, L.EXPORTS_ATTNQ,
              L.EXPORTS_MX, L.EXPORTS_MXROUND, L.EXPORTS_MXGEMM, L.EXPORTS_MXCONV)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert len(L.EXPORTS) == 124 and len(L.EXPORTS_MXGEMM) == 5 and len(L.EXPORTS_MXCONV) == 2


def test_out_pixels():
    from hipops import _lib as L
    f = L.lib().rdo_mx_conv_transpose2d_out_pixels
    for B, H, W, _, _, k, s, pad, op in TR.ALL_GEOMETRIES:
        want = B * TR.out_size(H, k, s, pad, op) * TR.out_size(W, k, s, pad, op)
        assert f(B, H, W, k, s, pad, op) == want == sum(len(p["pixels"]) for p in TR.phases(B, H, W, k, s, pad, op))
    assert f(4, 64, 64, 5, 2, 2, 1) == 4 * 128 * 128 and f(1, 1, 1, 1, 1, 0, 0) == 1 and f(1, 1, 1, 1, 4, 0, 3) == 16
    assert f(1, 3, 3, 3, 1, 1, 0) == 9 and f(1, 2 ** 15, 2 ** 16 - 1, 1, 1, 0, 0) == 2 ** 31 - 2 ** 15
    zeros = [(0, 4, 4, 3, 2, 1, 1), (-1, 4, 4, 3, 2, 1, 1), (1, 0, 4, 3, 2, 1, 1), (1, 4, -2, 3, 2, 1, 1), (1, 4, 4, 0, 2, 1, 1),
             (1, 4, 4, 3, 0, 1, 0), (1, 4, 4, 3, -1, 1, 0), (1, 4, 4, 3, 2, -1, 1), (1, 4, 4, 3, 2, 1, -1), (1, 4, 4, 3, 2, 1, 2),
             (1, 4, 4, 3, 1, 1, 1),
             (1, 1, 4, 1, 1, 1, 0), (1, 4, 1, 2, 1, 1, 0), (1, 2, 2, 3, 2, 3, 1),          # Ho or Wo <= 0
             (2, 2 ** 15, 2 ** 15, 1, 1, 0, 0),                                            # B H W = 2^31
             (1, 2 ** 15, 2 ** 15, 1, 2, 0, 0),                                            # the input fits, the output does not
             (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0)]
    for g in zeros:
        assert f(*g) == 0, g


def test_c_entry_refuses_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    odd = C.c_void_p(C.addressof(buf) + 2)
    names = ["x", "sx", "fx", "w", "sw", "fw", "B", "H", "W", "C", "N", "k", "stride", "pad", "opad", "bias", "y"]
    base = dict(x=p, sx=p, fx=0, w=p, sw=p, fw=3, B=2, H=4, W=5, C=64, N=37, k=5, stride=2, pad=2, opad=1, bias=None, y=p)
    bad = [dict(x=None), dict(sx=None), dict(w=None), dict(sw=None), dict(y=None),
           dict(x=odd), dict(w=odd), dict(bias=odd), dict(y=odd),
           dict(fx=-1), dict(fx=5), dict(fw=-1), dict(fw=5),
           dict(B=0), dict(B=-1), dict(H=0), dict(H=-4), dict(W=0), dict(W=-4), dict(C=0), dict(C=-32), dict(N=0), dict(N=-3),
           dict(k=0), dict(k=-3), dict(stride=0), dict(stride=-1), dict(pad=-1),
           dict(opad=-1), dict(opad=2), dict(opad=3), dict(stride=1, opad=1),
           dict(C=40), dict(C=3), dict(C=33),
           dict(H=1, pad=3), dict(W=1, pad=3), dict(H=1, W=1, k=1, stride=1, pad=1, opad=0),   # no output
           dict(B=2, H=2 ** 15, W=2 ** 15, k=1, stride=1, pad=0, opad=0),                  # B H W = 2^31
           dict(B=1, H=2 ** 15, W=2 ** 15, k=1, stride=2, pad=0, opad=0),                  # B Ho Wo > 2^31 - 1
           dict(B=1, H=2 ** 15, W=2 ** 15, C=32 * 2 ** 11, k=1, stride=1, pad=0, opad=0),  # 2^41 blocks in x
           dict(N=2 ** 31 - 1, C=32 * 2 ** 10),                                            # 25 x 2^10 x (2^31 - 1) blocks in w
           dict(H=1, W=1, k=2 ** 21, stride=1, pad=2 ** 20 - 1, opad=0),                   # a weight row of 2^42 blocks
           dict(B=1, H=2 ** 15, W=2 ** 16 - 1, C=32, N=4160, k=1, stride=1, pad=0, opad=0),    # (2^25 - 2^9) x 65 output tiles
           dict(B=1, H=1, W=1, C=32, N=64, k=1, stride=2 ** 16, pad=0, opad=0)]            # 2^32 phases of one tile
    for kw in bad:
        a = dict(base, **kw)
        assert h.rdo_mx_conv_transpose2d(*[a[n] for n in names], None) == RDO_EINVAL, kw
        assert h.rdo_last_error().startswith(b"rdo_mx_conv_transpose2d: "), (kw, h.rdo_last_error())


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
    x = ops.MXOperand(u8(40, 2 * 16), u8(40, 2), "mxfp4", 40, 64)                       # [2 * 4 * 5, 64]
    w = ops.MXOperand(u8(37, 50 * 32), u8(37, 50), "mxfp8_e4m3", 37, 1600)              # [37, 5 * 5 * 64]
    what = "mx_conv_transpose2d"
    cases = [
        ((u8(40, 32), w, (2, 4, 5), 5), f"{what}: x must be an MXOperand, got Tensor"),
        ((x, None, (2, 4, 5), 5), f"{what}: w must be an MXOperand, got NoneType"),
        ((ops.MXOperand(u8(40, 32), u8(40, 1), "mxfp4", 40, 64), w, (2, 4, 5), 5), f"{what}: x.scales must be a contiguous uint8 \\[40, 2\\]"),
        ((x, ops.MXOperand(u8(37, 50 * 32), u8(37, 50), "mxfp9", 37, 1600), (2, 4, 5), 5), f"{what}: unknown MX format 'mxfp9'"),
        ((x, ops.MXOperand(u8(37, 50 * 16), u8(37, 50), "mxfp8_e4m3", 37, 1600), (2, 4, 5), 5), f"{what}: w.packed must be a contiguous uint8 \\[37, 1600\\]"),
        ((x, w, (2, 4), 5), f"{what}: shape must be \\(B, H, W\\), got \\(2, 4\\)"),
        ((x, w, 40, 5), f"{what}: shape must be \\(B, H, W\\), got 40"),
        ((x, w, (2, 4.0, 5), 5), f"{what}: shape\\[1\\] must be a whole number >= 1, got 4.0"),
        ((x, w, (2, 0, 5), 5), f"{what}: shape\\[1\\] must be a whole number >= 1, got 0"),
        ((x, w, (2, 4, 5), 0), f"{what}: k must be a whole number >= 1, got 0"),
        ((x, w, (2, 4, 5), 5, 0), f"{what}: stride must be a whole number >= 1, got 0"),
        ((x, w, (2, 4, 5), 5, True), f"{what}: stride must be a whole number >= 1, got True"),
        ((x, w, (2, 4, 5), 5, 2, -1), f"{what}: pad must be a whole number >= 0, got -1"),
        ((x, w, (2, 4, 5), 5, 2, 2, -1), f"{what}: output_padding must be a whole number >= 0, got -1"),
        ((x, w, (2, 4, 5), 5, 2, 2, 2), f"{what}: output_padding 2 must be below the stride 2"),
        ((x, w, (2, 4, 5), 5, 1, 2, 1), f"{what}: output_padding 1 must be below the stride 1"),
        ((x, w, (2, 4, 6), 5, 2, 2, 1), f"{what}: x has 40 rows, shape \\(2, 4, 6\\) states 48 pixels"),
        ((x, w, (2, 4, 5), 3, 2, 1, 1), f"{what}: w has K = 1600, a 3 x 3 kernel over x's 64 channels needs K = 576"),
        ((x, w, (2, 4, 5), 5, 1, 5), f"{what}: a 5 x 5 kernel at stride 1, padding 5 and output padding 0 leaves no output of the 4 x 5 input"),
        ((x, w, (2, 4, 5), 5, 2, 2, 1, torch.zeros(36)), f"{what}: bias must be a contiguous fp32 \\[37\\]"),
        ((x, w, (2, 4, 5), 5, 2, 2, 1, torch.zeros(37).double()), f"{what}: bias must be a contiguous fp32 \\[37\\]"),
        ((x, w, (2, 4, 5), 5, 2, 2, 1, torch.zeros(37)), f"{what}: .*no CPU path"),
        ((x, w, (2, 4, 5), 5, 2, 2, 1), f"{what}: .*no CPU path"),
    ]
    for args, why in cases:
        with pytest.raises(ValueError, match=why):
            ops.mx_conv_transpose2d(*args)
    with pytest.raises(ValueError, match=f"{what}: w.packed must be a contiguous uint8 \\[37, 1600\\] on meta"):
        ops.mx_conv_transpose2d(ops.MXOperand(u8(40, 32).to("meta"), u8(40, 2).to("meta"), "mxfp4", 40, 64), w, (2, 4, 5), 5)


# ----------------------------------------------------------------------------- native_tconv_refusal, native_tconv, the report
def _module(org, q=None):
    from quantization import QuantModule
    m = QuantModule(org, WQ, AQ)
    if q is not None:
        m.weight_quantizer = q
    return m


def test_native_tconv_refuses_what_is_not_eligible():
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer, native_tconv, native_tconv_operand, native_tconv_refusal
    T = lambda fmt="mxfp4": MXQuantizer(fmt, tconv=True)
    not_square = "is not a square-kernel transposed conv with one stride, one padding, one output padding, dilation 1 and groups 1"
    cases = [
        (_module(nn.ConvTranspose2d(48, 8, 5, stride=2, padding=2, output_padding=1), T()), "its 48 input channels are no multiple of the MX block size 32"),
        (_module(nn.ConvTranspose2d(3, 32, 3), MXAdaRoundQuantizer("mxfp6_e2m3", tconv=True)), "its 3 input channels are no multiple"),
        (_module(nn.ConvTranspose2d(32, 8, 3, stride=(2, 1)), T()), f"stride \\(2, 1\\).* {not_square}"),
        (_module(nn.ConvTranspose2d(32, 8, (3, 1)), T()), f"kernel \\(3, 1\\).* {not_square}"),
        (_module(nn.ConvTranspose2d(32, 8, 3, padding=(1, 0)), T()), f"padding \\(1, 0\\).* {not_square}"),
        (_module(nn.ConvTranspose2d(32, 8, 3, stride=2, output_padding=(1, 0)), T()), f"output padding \\(1, 0\\).* {not_square}"),
        (_module(nn.ConvTranspose2d(32, 8, 3, dilation=2), T()), f"dilation \\(2, 2\\), groups 1 {not_square}"),
        (_module(nn.ConvTranspose2d(64, 8, 3, groups=2), T()), f"groups 2 {not_square}"),
        (_module(nn.Conv2d(32, 8, 3, padding=1), MXQuantizer("mxfp4")), "a conv module is not a transposed convolution"),
        (_module(nn.Linear(64, 8), MXQuantizer("mxfp4")), "a linear module is not a transposed convolution"),
        (_module(nn.ConvTranspose2d(32, 8, 3)), "its weight quantiser is a UniformAffineQuantizer"),
        (_module(nn.ConvTranspose2d(32, 8, 3), MXQuantizer("mxfp4")), "its MXQuantizer was made with tconv=False"),
        # the order: kind, geometry, channels, quantiser -- 8 output channels are no obstacle, 48 input channels are
        (_module(nn.ConvTranspose2d(48, 8, 3, stride=(2, 1))), f"stride \\(2, 1\\).* {not_square}"),
        (_module(nn.ConvTranspose2d(48, 8, 3)), "its 48 input channels are no multiple"),
        (_module(nn.ConvTranspose2d(48, 32, 3)), "its 48 input channels are no multiple"),
    ]
    for m, why in cases:
        assert re.search(why, native_tconv_refusal(m)), (why, native_tconv_refusal(m))
        with pytest.raises(ValueError, match=f"native_tconv_operand: module QuantModule\\({m.kind}, .*{why}"):
            native_tconv_operand(m)
        with pytest.raises(ValueError, match="native_tconv_operand: module"):
            native_tconv(m, torch.zeros(2, 32, 3, 4), "mxfp8_e4m3")
    # what is eligible goes on to the kernels, which have no CPU path
    for org, q, x in ((nn.ConvTranspose2d(32, 16, 5, stride=2, padding=2, output_padding=1), T(), torch.zeros(2, 32, 3, 4)),
                      (nn.ConvTranspose2d(64, 24, 3, stride=1, padding=1), MXAdaRoundQuantizer("mxfp8_e5m2", tconv=True), torch.zeros(2, 64, 3, 4)),
                      (nn.ConvTranspose2d(32, 8, 1, stride=2, output_padding=1), T("mxfp6_e3m2"), torch.zeros(1, 32, 3, 3))):
        m = _module(org, q)
        assert native_tconv_refusal(m) is None
        with pytest.raises(ValueError, match="mx_fakequant: .*no CPU path"):
            native_tconv(m, x, "mxfp8_e4m3")
        assert m._pack_memo == {}
    m = _module(nn.ConvTranspose2d(32, 16, 5, stride=2, padding=2, output_padding=1), T())
    with pytest.raises(ValueError, match="native_tconv: the input must be \\[B, 32, H, W\\]"):
        native_tconv(m, torch.zeros(2, 16, 3, 4), "mxfp4")


def test_report_refuses_a_tconvs_that_is_no_bool_before_any_gpu_work(monkeypatch):
    from hipops import ops
    qnn = forward_model()
    monkeypatch.setattr(ops, "_ptr", lambda *a, **k: (_ for _ in ()).throw(AssertionError("reached the library")))
    qnn.set_weight_format("mxfp4")
    images = torch.rand(2, 3, 8, 8)
    assert list(qnn.units()) == ["stem", "conv", "up", "head", "fc"]
    for tconvs in ("yes", 1, None):
        with pytest.raises(ValueError, match="mx_native_report: tconvs must be True or False, got"):
            qnn.mx_native_report(images, tconvs=tconvs)
    # the named-unit refusal follows the flag: the transposed conv is eligible only with tconvs=True
    with pytest.raises(ValueError, match="mx_native_report: unit 'up' holds no eligible module: .*a tconv module is not GEMM-shaped"):
        qnn.mx_native_report(images, units=["up"])
    with pytest.raises(ValueError, match="mx_native_report: unit 'up' holds no eligible module: .*a tconv module is not GEMM-shaped"):
        qnn.mx_native_report(images, units=["up"], convs=True)


# ----------------------------------------------------------------------------- set_mx_activations, the forward mode, reconstruction
def test_set_mx_activations_checks_its_arguments_and_reports_what_it_set():
    from quantization import QuantModule
    from quantization import mx
    qnn = forward_model()
    qnn.set_weight_format("mxfp4")
    mods = {n: m for n, m in qnn.model.named_modules() if isinstance(m, QuantModule)}
    assert all(getattr(m, "mx_activations", None) is None for m in mods.values())
    refused = [
        (dict(act_fmt="mxfp9"), "set_mx_activations: unknown MX format 'mxfp9'"),
        (dict(act_fmt=4), "set_mx_activations: unknown MX format"),
        (dict(act_fmt="mxfp4", mode="fast"), "set_mx_activations: mode must be one of \\['native', 'emulated'\\], got 'fast'"),
        (dict(act_fmt=None, mode=None), "set_mx_activations: mode must be one of"),
        (dict(act_fmt="mxfp4", units=["conv", "nope"]), "set_mx_activations: unknown unit name\\(s\\) \\['nope'\\]"),
        (dict(act_fmt="mxfp4", units="conv"), "set_mx_activations: units must be None or a list of unit names"),
        (dict(act_fmt="mxfp4", units=["conv", "stem"]), "set_mx_activations: unit 'stem' holds no eligible module: .*its 3 input channels"),
    ]
    for kw, why in refused:
        with pytest.raises(ValueError, match=why):
            qnn.set_mx_activations(**kw)
        assert all(getattr(m, "mx_activations", None) is None for m in mods.values()), kw      # nothing was written
    rep = qnn.set_mx_activations("mxfp8_e4m3")
    assert list(rep) == ["native", "left"]
    assert list(rep["native"].items()) == [("conv", "conv"), ("up", "tconv"), ("head", "conv"), ("fc", "linear")]
    assert list(rep["left"]) == ["stem"] and rep["left"]["stem"] == mx.native_conv_refusal(mods["stem"])
    assert {n: m.mx_activations for n, m in mods.items()} == {"stem": None, "conv": ("mxfp8_e4m3", "native"), "up": ("mxfp8_e4m3", "native"),
                                                               "head": ("mxfp8_e4m3", "native"), "fc": ("mxfp8_e4m3", "native")}
    # a unit at a time, the other mode; trained units are served alike
    mods["up"].trained = True
    rep = qnn.set_mx_activations("mxfp4", mode="emulated", units=["up"])
    assert dict(rep["native"]) == {"up": "tconv"} and dict(rep["left"]) == {}
    assert mods["up"].mx_activations == ("mxfp4", "emulated") and mods["conv"].mx_activations == ("mxfp8_e4m3", "native")
    # None clears the chosen units, named or all; clearing needs no eligible module
    rep = qnn.set_mx_activations(None, units=["conv", "stem"])
    assert dict(rep["native"]) == {"conv": "conv"} and list(rep["left"]) == ["stem"]
    assert mods["conv"].mx_activations is None and mods["up"].mx_activations == ("mxfp4", "emulated")
    qnn.set_mx_activations(None)
    assert all(m.mx_activations is None for m in mods.values())
    # a weight that is in no MX format is left for that reason
    qnn.set_weight_format({"head": "int"})
    rep = qnn.set_mx_activations("mxfp4")
    assert "its weight quantiser is a UniformAffineQuantizer" in rep["left"]["head"] and mods["head"].mx_activations is None
    assert list(rep["native"]) == ["conv", "up", "fc"]


def test_switched_modules_refuse_cpu_inputs_and_keep_the_quantiser_refusal():
    from quantization.mx import MXQuantizer
    qnn = forward_model()
    qnn.set_weight_format("mxfp4")
    qnn.set_mx_activations("mxfp4")
    qnn.set_quant_state(True, False)
    with pytest.raises(RuntimeError, match="QuantModule.forward runs on librdoptq_hip only"):
        qnn(torch.rand(2, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="MXQuantizer\\(mxfp4\\): MX activations are not built into the quantisers"):
        MXQuantizer("mxfp4")(torch.zeros(4, 32), act=True)


def test_reconstruction_refuses_a_model_on_mx_activations(monkeypatch):
    from quantization import block_reconstruction, layer_reconstruction, recon
    qnn = forward_model()
    qnn.set_weight_format("mxfp4", rounding="learned")
    monkeypatch.setattr(recon, "_reconstruct", lambda *a, **k: (_ for _ in ()).throw(AssertionError("reached the calibration")))
    qnn.set_mx_activations("mxfp8_e4m3", units=["up"])
    cali = torch.rand(2, 3, 8, 8)
    why = "reconstruct: module 'model.up' runs on MX activations \\(mxfp8_e4m3, native\\): calibration under MX activations is not built"
    for fn in (layer_reconstruction, block_reconstruction):
        with pytest.raises(NotImplementedError, match=why):
            fn(qnn, qnn.model.conv, "conv", cali)                                       # any unit of such a model, switched or not
    qnn.set_mx_activations(None)
    for fn in (layer_reconstruction, block_reconstruction):
        with pytest.raises(AssertionError, match="reached the calibration"):
            fn(qnn, qnn.model.conv, "conv", cali)


def test_the_attribute_defaults_to_off_for_models_made_before_it_existed():
    import pickle
    from quantization import QuantModule
    m = _module(nn.Conv2d(32, 8, 3, padding=1))
    assert "mx_activations" not in m.__dict__ and getattr(m, "mx_activations", None) is None
    m2 = pickle.loads(pickle.dumps(m))
    assert isinstance(m2, QuantModule) and getattr(m2, "mx_activations", None) is None


# ----------------------------------------------------------------------------- the reference
def test_reference_phases_and_operands():
    ph = TR.phases(1, 3, 3, 3, 2, 1, 1)                                                 # Ho = Wo = 6
    assert [(p["ry"], p["rx"]) for p in ph] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [len(p["taps"]) for p in ph] == [4, 2, 2, 1] and ph[0]["taps"] == [(0, 0), (0, 2), (2, 0), (2, 2)]
    assert sorted(np.concatenate([p["pixels"] for p in ph]).tolist()) == list(range(36))
    # phase (1, 1): oy, ox in {0, 2, 4}, tap (1, 1), input pixel (oy / 2, ox / 2)
    assert ph[3]["pixels"].tolist() == [0, 2, 4, 12, 14, 16, 24, 26, 28] and ph[3]["index"][:, 0].tolist() == list(range(9))
    # phase (0, 0): oy, ox in {1, 3, 5}; output (1, 1) reads input (1, 1), (1, 0), (0, 1), (0, 0) for taps (0, 0), (0, 2), (2, 0), (2, 2)
    assert ph[0]["pixels"][0] == 7 and ph[0]["index"][0].tolist() == [4, 3, 1, 0]
    assert ph[0]["index"][8].tolist() == [-1, -1, -1, 8]                                # output (5, 5): only tap (2, 2) is inside
    # k < s: three phases without a tap; output padding rows are in a tapless phase or outside the image
    ph = TR.phases(1, 3, 3, 1, 2, 0, 1)
    assert [len(p["taps"]) for p in ph] == [1, 0, 0, 0] and [p["index"].shape for p in ph] == [(9, 1), (9, 0), (9, 0), (9, 0)]
    ph = TR.phases(1, 3, 3, 3, 3, 0, 2)                                                 # Ho = 11: rows 9, 10 read input row 3
    rows = {int(px) // 11: idx for p in ph for px, idx in zip(p["pixels"], p["index"])}
    assert all((rows[r] == -1).all() for r in (9, 10)) and (rows[8] >= 0).any()
    codes = np.arange(1, 1 + 9 * 32, dtype=np.uint8).reshape(9, 32)
    scales = np.arange(100, 109, dtype=np.uint8).reshape(9, 1)
    c, s = TR.gathered_activation(codes, scales, TR.phases(1, 3, 3, 3, 2, 1, 1)[0])
    assert c.shape == (9, 128) and s.shape == (9, 4) and s[0].tolist() == [104, 103, 101, 100] and s[8].tolist() == [127, 127, 127, 108]
    assert (c[8, :96] == 0).all() and (c[8, 96:] == codes[8]).all()
    w = np.arange(2 * 9 * 4).reshape(2, 36)
    assert TR.gathered_weight(w, TR.phases(1, 3, 3, 3, 2, 1, 1)[1], 3, 4)[1].tolist() == [40, 41, 42, 43, 64, 65, 66, 67]   # taps (0, 1), (2, 1)
    assert TR.gathered_weight(w, TR.phases(1, 3, 3, 1, 2, 0, 1)[1], 3, 4).shape == (2, 0)


@pytest.mark.parametrize("geometry", TR.ALL_GEOMETRIES)
def test_reference_tconv64_is_torch_conv_transpose2d_in_float64(geometry):
    B, H, W, Cc, N, k, s, pad, op = geometry
    fx, fw = "mxfp6_e2m3", "mxfp8_e4m3"
    rng = np.random.default_rng(sum(geometry))
    # decoded random operands: every finite code, scales over +-3
    xc = rng.choice(G.finite_codes(fx), (B * H * W, Cc)).astype(np.uint8)
    wc = rng.choice(G.finite_codes(fw), (N, k * k * Cc)).astype(np.uint8)
    xs = rng.integers(124, 131, (B * H * W, Cc // 32)).astype(np.uint8)
    ws = rng.integers(124, 131, (N, k * k * Cc // 32)).astype(np.uint8)
    bias = rng.standard_normal(N)
    got = TR.tconv64(xc, xs, fx, wc, ws, fw, geometry, bias)
    x = torch.from_numpy(G.decode(xc, xs, fx)).reshape(B, H, W, Cc).permute(0, 3, 1, 2)
    w = torch.from_numpy(G.decode(wc, ws, fw)).reshape(N, k, k, Cc).permute(3, 0, 1, 2)     # [Cin, Cout, kh, kw]: W[c, n, kh, kw]
    want = torch.nn.functional.conv_transpose2d(x, w, torch.from_numpy(bias), stride=s, padding=pad, output_padding=op)
    assert want.dtype == torch.float64 and tuple(want.shape) == (B, N, TR.out_size(H, k, s, pad, op), TR.out_size(W, k, s, pad, op))
    want = want.permute(0, 2, 3, 1).reshape(-1, N).numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert (TR.values64(G.decode(xc, xs, fx), G.decode(wc, ws, fw), geometry, bias) == got).all()
    # the exact case: every sum is exact in float64 whatever its order
    c = TR.exact_tconv_case(fx, fw, geometry, seed=sum(geometry))
    x = torch.from_numpy(G.decode(c["x_codes"], c["x_scales"], fx)).reshape(B, H, W, Cc).permute(0, 3, 1, 2)
    w = torch.from_numpy(G.decode(c["w_codes"], c["w_scales"], fw)).reshape(N, k, k, Cc).permute(3, 0, 1, 2)
    want = torch.nn.functional.conv_transpose2d(x, w, torch.from_numpy(c["bias"]).double(), stride=s, padding=pad, output_padding=op)
    assert (c["ref"] == want.permute(0, 2, 3, 1).reshape(-1, N).numpy()).all()
    assert (c["ref"] * 16 == np.round(c["ref"] * 16)).all() and (c["x_codes"] != 0).any(axis=1).all()


def test_exact_case_refuses_a_k_whose_sums_could_round():
    with pytest.raises(AssertionError):
        TR.exact_tconv_case("mxfp4", "mxfp4", (1, 4, 4, 320, 8, 5, 2, 2, 1), seed=0)    # K = 8000 > 7281
    assert all(2304 * g[5] * g[5] * g[3] + 128 < 2 ** 24 for g in TR.ALL_GEOMETRIES)
