"""CPU checks of the one-launch MX residual unit: include/rdo_ptq_mxresunit.h against `EXPORTS_MXRESUNIT` and the built library, the
refusals of the C entry (RDO_EINVAL without touching a device), of `ops.mx_residual_unit` before a pointer is taken, the reasons of
`mx.native_residual_unit_refusal` in their order, and `set_mx_activations(..., residual_units=...)` with its report and its clearing."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from test_mx_conv_args import AQ, RDO_EINVAL, ROOT, WQ, no_library  # noqa: F401  (no_library is a fixture)

NAME = "rdo_mx_residual_unit"
UNITS = [f"conv_{ab}.{i}" for ab in "ab" for i in range(3)]


def attention_model(N=64):
    """a toy model: one `AttentionBlock(N)` of Cheng2020-attn -- six residual units and the trailing 1x1"""
    import lic
    from quantization import QuantModel
    torch.manual_seed(49)
    return QuantModel(lic.AttentionBlock(N).eval(), WQ, AQ).eval()


def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxresunit.h")).read()
    assert set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M)) == set(L.EXPORTS_MXRESUNIT) == {NAME}
    fn = getattr(L.lib(), NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 25
    tables = [v for k, v in vars(L).items() if k.startswith("EXPORTS") and k != "EXPORTS_MXRESUNIT"]
    assert not any(NAME in t or any(n in NAME for n in t) for t in tables)
    assert int(re.search(r"#define RDO_MXRESUNIT_MAX_N (\d+)", hdr).group(1)) == L.MXRESUNIT_MAX_N >= 320 and L.MXRESUNIT_MAX_N % 64 == 0


def test_c_entry_refuses_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    base_addr = (C.addressof(buf) + 15) & ~15
    p, odd, by4 = C.c_void_p(base_addr), C.c_void_p(base_addr + 2), C.c_void_p(base_addr + 4)
    names = ["x", "B", "H", "W", "N", "fa", "w1", "s1", "b1", "w2", "s2", "b2", "w3", "s3", "b3", "fw", "out", "xp", "xs", "h1", "h1s", "h2", "h2s",
             "branch"]
    base = dict(x=p, B=2, H=9, W=17, N=192, fa=3, w1=p, s1=p, b1=p, w2=p, s2=p, b2=p, w3=p, s3=p, b3=p, fw=0, out=p, xp=None, xs=None, h1=None,
                h1s=None, h2=None, h2s=None, branch=None)
    bad = [dict(x=None), dict(w1=None), dict(s1=None), dict(w2=None), dict(s2=None), dict(w3=None), dict(s3=None), dict(out=None), dict(B=0),
           dict(H=0), dict(W=-3), dict(N=0), dict(B=2 ** 15, H=2 ** 15, W=2), dict(N=32), dict(N=96), dict(N=L.MXRESUNIT_MAX_N + 64), dict(fa=5),
           dict(fa=-1), dict(fw=5), dict(xp=p), dict(xs=p), dict(h1=p), dict(h1s=p), dict(h2=p), dict(h2s=p), dict(x=by4), dict(out=by4),
           dict(branch=by4), dict(w1=odd), dict(w2=odd), dict(w3=odd), dict(b1=odd), dict(b2=odd), dict(b3=odd), dict(xp=odd, xs=p),
           dict(h1=odd, h1s=p), dict(h2=odd, h2s=p)]
    for kw in bad:
        a = dict(base, **kw)
        assert getattr(h, NAME)(*[a[n] for n in names], None) == RDO_EINVAL, kw
        assert h.rdo_last_error().startswith(NAME.encode() + b": "), (kw, h.rdo_last_error())


def test_wrapper_refuses_malformed_arguments(no_library):
    ops = no_library
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    w = lambda n, k, fmt="mxfp4", bits=4: ops.MXOperand(u8(n, k // 32 * 4 * bits), u8(n, k // 32), fmt, n, k)
    x, half, full = torch.zeros(2 * 5 * 3, 64), torch.ones(32), torch.ones(64)
    cases = [(dict(x=torch.zeros(2, 15, 64)), "x"), (dict(shape=(2, 5)), "shape must be \\(B, H, W\\)"), (dict(shape=(2, 5, 4)), "x has 30 rows"),
             (dict(shape=(2, 0, 3)), "shape\\[1\\]"), (dict(x=torch.zeros(30, 96)), "N = 96 is no multiple of 64"),
             (dict(x=torch.zeros(30, 384)), "N = 384 is above 320"), (dict(w1=u8(32, 64)), "w1 must be an MXOperand"),
             (dict(w1=w(32, 96)), "w1 is \\[32, 96\\]"), (dict(w2=w(32, 256)), "w2 \\[32, 256\\]"), (dict(w3=w(32, 64)), "w3 \\[32, 64\\]"),
             (dict(w2=w(32, 288, "mxfp8_e4m3", 8)), "one weight format"), (dict(b1=full), "b1"), (dict(b2=full), "b2"), (dict(b3=half), "b3"),
             (dict(act_fmt="fp8"), "unknown MX format 'fp8'"), (dict(out=torch.zeros(30, 32)), "out"), (dict(want="h1"), "want must be a sequence"),
             (dict(want=("h1", "h1")), "distinct names"), (dict(want=("pre",)), "distinct names"), (dict(), "no CPU path")]
    for kw, why in cases:
        k = dict(dict(x=x, shape=(2, 5, 3), w1=w(32, 64), b1=half, w2=w(32, 288), b2=half, w3=w(64, 32), b3=full, act_fmt="mxfp8_e4m3"), **kw)
        with pytest.raises(ValueError, match=f"mx_residual_unit: .*{why}"):
            ops.mx_residual_unit(*[k.pop(n) for n in ("x", "shape", "w1", "b1", "w2", "b2", "w3", "b3", "act_fmt")], **k)


def test_refusal_reasons_in_their_order():
    from quantization.mx import native_residual_unit_refusal as refusal
    qnn = attention_model()
    unit = qnn.model.conv_a[0]
    c1, c2, c3 = unit.conv[0], unit.conv[2], unit.conv[4]
    # the faults together; each repair uncovers the next reason (`set_weight_format` refuses a trained module: that fault comes later)
    c2.fwd_kwargs["padding"] = (0, 0)
    c1.se_module = nn.Identity()
    assert refusal(unit).startswith("conv.2 has weight (32, 32, 3, 3), stride")
    c2.fwd_kwargs["padding"] = (1, 1)
    assert refusal(unit).startswith("conv.0: its weight quantiser is a UniformAffineQuantizer")
    qnn.set_weight_format({f"{UNITS[0]}.conv.0": "mxfp4", f"{UNITS[0]}.conv.2": "mxfp8_e4m3", f"{UNITS[0]}.conv.4": "mxfp4"})
    assert refusal(unit) == "its weights are in mxfp4, mxfp8_e4m3 and mxfp4: the kernel takes one weight format"
    qnn.set_weight_format("mxfp4")
    c3.trained = c3.use_act_quant = True
    assert refusal(unit) == "one of its convs has an se_module"
    c1.se_module = None
    c2.activation_function = nn.LeakyReLU(0.01)
    assert refusal(unit).startswith("its activation functions are ReLU, LeakyReLU and StraightThrough")
    c2.activation_function = nn.ReLU()
    assert refusal(unit) == "an activation quantiser is active on one of its three convs"
    c3.trained = c3.use_act_quant = False
    assert refusal(unit) is None and refusal(qnn.model.conv_b) == "a Sequential does not hold the three convs of a residual unit"
    # N: ragged (96 / 2 is no whole number of blocks), then above the maximum
    for N, why in ((96, "its 96 channels are no multiple of 64"), (384, "its 384 channels are above 320")):
        wide = attention_model(N)
        wide.set_weight_format("mxfp4")
        assert refusal(wide.model.conv_a[0]).startswith(why)


def test_set_mx_activations_residual_units_switch_report_and_clearing():
    qnn = attention_model()
    qnn.set_weight_format("mxfp4")
    units = [m for m in qnn.modules() if type(m).__name__ == "_ResidualUnit"]
    for kw in (dict(mode="emulated", residual_units=True), dict(residual_units=1), dict(residual_units=None)):
        with pytest.raises(ValueError, match="set_mx_activations: residual_units must be True or False, and True in mode 'native' only"):
            qnn.set_mx_activations("mxfp4", **kw)
        assert not any(hasattr(m, "mx_resunit") or getattr(m, "mx_activations", None) for m in qnn.modules())
    assert "residual_units" not in qnn.set_mx_activations("mxfp8_e4m3") and not any(u.mx_resunit for u in units)
    rep = qnn.set_mx_activations("mxfp8_e4m3", residual_units=True)
    assert dict(rep["residual_units"]) == {u: tuple(f"{u}.conv.{i}" for i in (0, 2, 4)) for u in UNITS} and not rep["left"]
    assert all(u.mx_resunit is True for u in units) and rep["native"]["conv_b.3"] == "conv"
    # a refused unit goes under 'left' with its reason; a unit whose convs are not all chosen likewise
    units[1].conv[2].trained = units[1].conv[2].use_act_quant = True
    rep = qnn.set_mx_activations("mxfp8_e4m3", residual_units=True)
    assert list(rep["residual_units"]) == UNITS[:1] + UNITS[2:] and rep["left"][UNITS[1]].startswith("an activation quantiser is active")
    assert not units[1].mx_resunit and units[0].mx_resunit
    units[1].conv[2].trained = units[1].conv[2].use_act_quant = False
    rep = qnn.set_mx_activations("mxfp8_e4m3", units=[f"{UNITS[0]}.conv.0", f"{UNITS[0]}.conv.2"], residual_units=True)
    assert not rep["residual_units"] and rep["left"][UNITS[0]] == "its three convs are not all among the chosen units and switched"
    assert not units[0].mx_resunit and units[2].mx_resunit
    # residual_units=False and act_fmt=None clear the attribute
    qnn.set_mx_activations("mxfp8_e4m3", residual_units=True)
    assert "residual_units" not in qnn.set_mx_activations("mxfp8_e4m3") and not any(u.mx_resunit for u in units)
    qnn.set_mx_activations("mxfp8_e4m3", residual_units=True)
    qnn.set_mx_activations(None)
    assert not any(u.mx_resunit for u in units)
