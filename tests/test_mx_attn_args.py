"""CPU checks of the MX window attention: include/rdo_ptq_mxattn.h against `EXPORTS_MXATTN` and the built library, the refusals of the C
entry (RDO_EINVAL without touching a device), of `ops.mx_window_attention` before a pointer is taken, and of
`set_mx_activations(..., attention=...)` with the report of the switch and the reasons of `mx.native_attention_refusal`."""
import ctypes as C
import os
import re

import pytest
import torch

from test_mx_conv_args import RDO_EINVAL, ROOT, no_library  # noqa: F401  (no_library is a fixture)
from test_mx_swin_args import BLOCKS, swin_model


def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxattn.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXATTN) == {"rdo_mx_window_attention"}
    assert hasattr(L.lib(), "rdo_mx_window_attention") and not any("rdo_mx_window_attention" in t for t in (L.EXPORTS, L.EXPORTS_MXSWIN))


def test_c_entry_refuses_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    base_addr = (C.addressof(buf) + 15) & ~15
    p, odd, by4 = C.c_void_p(base_addr), C.c_void_p(base_addr + 2), C.c_void_p(base_addr + 4)
    good = dict(B=1, H=8, W=8, C=48, heads=2, window=8, shift=0)
    geoms = [dict(heads=8), dict(heads=5), dict(H=12), dict(window=16, H=16, W=16), dict(shift=8), dict(B=0), dict(C=160, heads=2)]
    args = [dict(qkv=None), dict(bias=None), dict(out=None), dict(fmt=5), dict(fmt=-1), dict(pfmt=5), dict(qkv=by4), dict(out=by4),
            dict(bias=odd), dict(scores=odd), dict(probs=odd)]
    base = dict(qkv=p, bias=by4, fmt=0, pfmt=3, out=p, scores=None, probs=by4)
    cases = [(dict(good, **g), base) for g in geoms] + [(good, dict(base, **a)) for a in args] + [(None, base)]
    for g, a in cases:
        d = None if g is None else C.byref(L.AttnDesc(g["B"], g["H"], g["W"], g["C"], g["heads"], g["window"], g["shift"], 0.25))
        assert h.rdo_mx_window_attention(d, a["qkv"], a["bias"], a["fmt"], a["pfmt"], a["out"], a["scores"], a["probs"], None) == RDO_EINVAL, (g, a)
        assert h.rdo_last_error().startswith(b"rdo_mx_window_attention: "), (g, a, h.rdo_last_error())


def test_wrapper_refuses_malformed_arguments(no_library):
    ops = no_library
    d = ops.attn_desc(1, 8, 8, 48, 2, 8, 0)
    qkv, bias = torch.zeros(1, 8, 8, 144), torch.zeros(2, 64, 64)
    cases = [(dict(d=ops.attn_desc(1, 8, 8, 48, 8, 8, 0)), "head dim 6 .* is no multiple of 4"), (dict(d=ops.attn_desc(1, 8, 12, 48, 2, 8, 0)), "not divisible by window"),
             (dict(d=(1, 8, 8)), "expected an attn_desc"), (dict(qkv=torch.zeros(1, 8, 8, 96)), "qkv holds 6144 elements, expected 9216"),
             (dict(qkv=qkv.double()), "qkv must be an fp32 tensor"), (dict(qkv=qkv.transpose(1, 2)), "qkv must be contiguous"),
             (dict(bias=torch.zeros(2, 64, 63)), "bias holds"), (dict(fmt="mxfp5"), "unknown MX format 'mxfp5'"),
             (dict(p_fmt="fp8"), "unknown MX format 'fp8'"), (dict(out=torch.zeros(1, 8, 8, 47)), "out must be a contiguous fp32 \\[1, 8, 8, 48\\]"),
             (dict(want="probs"), "want must be a sequence"), (dict(want=("probs", "probs")), "distinct names"), (dict(want=("out",)), "distinct names"),
             (dict(), "no CPU path")]
    for kw, why in cases:
        k = dict(dict(d=d, qkv=qkv, bias=bias, fmt="mxfp4"), **kw)
        with pytest.raises(ValueError, match=f"mx_window_attention: .*{why}"):
            ops.mx_window_attention(k.pop("d"), k.pop("qkv"), k.pop("bias"), k.pop("fmt"), **k)


def test_set_mx_activations_attention_switch_report_and_refusals():
    from quantization.mx import native_attention, native_attention_refusal
    qnn = swin_model()
    qnn.set_weight_format("mxfp4")
    qnn.set_quant_state(True, False)
    for kw in (dict(mode="emulated", attention=True), dict(attention=1), dict(p_fmt="mxfp4"), dict(attention=True, p_fmt="mxfp5")):
        with pytest.raises(ValueError, match="set_mx_activations: "):
            qnn.set_mx_activations("mxfp8_e4m3", **kw)
        assert not any(hasattr(m, "mx_attention") or getattr(m, "mx_activations", None) for m in qnn.modules())
    attns = [b.attn for b in qnn.model.rstb.residual_group.blocks]
    rep = qnn.set_mx_activations("mxfp8_e4m3", attention=True, p_fmt="mxfp6_e2m3", swin=True)
    assert dict(rep["attention"]) == {f"{BLOCKS}{i}.attn": ("mxfp8_e4m3", "mxfp6_e2m3") for i in "01"} and len(rep["swin"]) == 2 and not rep["left"]
    assert all(a.mx_attention == ("mxfp8_e4m3", "mxfp6_e2m3") and a._mx_attention_formats() == a.mx_attention for a in attns)
    # an attention whose quantiser rounds the probabilities keeps its two-launch split; p_fmt defaults to act_fmt
    attns[1].trained = attns[1].use_act_quant = True
    rep = qnn.set_mx_activations("mxfp4", attention=True)
    assert dict(rep["attention"]) == {BLOCKS + "0.attn": ("mxfp4", "mxfp4")} and attns[1].mx_attention is None
    assert rep["left"][BLOCKS + "1.attn"].startswith("its activation quantiser rounds the probabilities")
    attns[1].trained = attns[1].use_act_quant = False
    # attention=False and act_fmt=None clear it; a qkv on other operands than (fmt, 'native') leaves the fp32 core in charge
    assert "attention" not in qnn.set_mx_activations("mxfp4") and not any(a.mx_attention for a in attns)
    qnn.set_mx_activations("mxfp4", attention=True)
    attns[0].qkv.mx_activations = ("mxfp4", "emulated")
    assert attns[0]._mx_attention_formats() is None and attns[1]._mx_attention_formats() == ("mxfp4", "mxfp4")
    qnn.set_mx_activations(None)
    assert not any(a.mx_attention for a in attns)
    # the other reasons
    assert native_attention_refusal(attns[0].qkv) == "a QuantModule is no QuantWindowAttention"
    attns[0].num_heads = 3
    assert "is no multiple of 4" in native_attention_refusal(attns[0])
    with pytest.raises(ValueError, match="native_attention: its head dim 10"):
        native_attention(attns[0], torch.zeros(1, 16, 96), 1, 4, 4, 4, 0, "mxfp4")
    attns[0].num_heads = 2
    qnn.set_weight_format({"rstb": "int"})
    rep = qnn.set_mx_activations("mxfp4", attention=True)
    assert rep["left"][BLOCKS + "0.attn"].startswith("qkv keeps its fp32 operands: its weight quantiser is a UniformAffineQuantizer")
