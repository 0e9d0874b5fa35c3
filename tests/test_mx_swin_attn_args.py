"""CPU checks of the one-launch attention half of an MX Swin block: include/rdo_ptq_mxswinattn.h against `EXPORTS_MXSWINATTN` and the built
library, the refusals of the C entry (RDO_EINVAL without touching a device), of `ops.mx_swin_attn` before a pointer is taken, the reasons
of `mx.native_swin_attn_refusal` in their order, and `set_mx_activations(..., fused_attention=...)` with its report."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from test_mx_conv_args import RDO_EINVAL, ROOT, no_library  # noqa: F401  (no_library is a fixture)
from test_mx_swin_args import BLOCKS, swin_model

GOOD = dict(B=1, H=8, W=8, C=64, heads=2, window=8, shift=0)
NAMES = ["x", "lw", "lb", "eps", "fa", "wqkv", "sqkv", "bqkv", "wproj", "sproj", "bproj", "fw", "bias", "out", "ln", "qkv", "attn", "branch"]


def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxswinattn.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXSWINATTN) == {"rdo_mx_swin_attn"}
    fn = L.lib().rdo_mx_swin_attn
    assert fn.restype is C.c_int and len(fn.argtypes) == 20 and fn.argtypes[4] is C.c_float
    assert not any("rdo_mx_swin_attn" in t for t in (L.EXPORTS, L.EXPORTS_MXSWIN, L.EXPORTS_MXATTN))
    assert int(re.search(r"#define RDO_MXSWINATTN_MAX_C (\d+)", hdr).group(1)) == L.MXSWINATTN_MAX_C >= 192


@pytest.mark.parametrize("geom,args", [(dict(heads=8, C=48), {}), (dict(heads=5), {}), (dict(H=12), {}), (dict(window=16, H=16, W=16), {}),
                                       (dict(shift=8), {}), (dict(B=0), {}), (dict(C=160, heads=2), {}), (dict(C=48), {}),
                                       (dict(C=352, heads=11), {}), (None, {})] +
                         [({}, a) for a in (dict(fa=5), dict(fa=-1), dict(fw=5), dict(x=None), dict(wqkv=None), dict(sqkv=None), dict(wproj=None),
                                            dict(sproj=None), dict(bias=None), dict(out=None), dict(x="by4"), dict(lw="by4"), dict(lb="by4"),
                                            dict(bqkv="by4"), dict(bproj="by4"), dict(out="by4"), dict(ln="by4"), dict(qkv="by4"),
                                            dict(attn="by4"), dict(branch="by4"), dict(bias="odd"), dict(wqkv="odd"), dict(wproj="odd"))])
def test_c_entry_refuses_bad_arguments_without_a_device(geom, args):
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    base_addr = (C.addressof(buf) + 15) & ~15
    ptr = {"p": C.c_void_p(base_addr), "odd": C.c_void_p(base_addr + 2), "by4": C.c_void_p(base_addr + 4)}
    a = dict(dict({n: "p" for n in NAMES}, eps=C.c_float(1e-5), fa=0, fw=3, bias="by4", ln=None), **args)
    a = {n: ptr.get(v, v) if isinstance(v, str) else v for n, v in a.items()}
    g = None if geom is None else dict(GOOD, **geom)
    d = None if g is None else C.byref(L.AttnDesc(g["B"], g["H"], g["W"], g["C"], g["heads"], g["window"], g["shift"], 0.25))
    assert h.rdo_mx_swin_attn(d, *[a[n] for n in NAMES], None) == RDO_EINVAL
    assert h.rdo_last_error().startswith(b"rdo_mx_swin_attn: "), h.rdo_last_error()


def _operand(ops, n, k, fmt="mxfp4", bits=4):
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    return ops.MXOperand(u8(n, k // 32 * 4 * bits), u8(n, k // 32), fmt, n, k)


@pytest.mark.parametrize("kw,why", [
    (dict(d=(1, 8, 8)), "expected an attn_desc"), (dict(geom=dict(H=12)), "not divisible by window"),
    (dict(geom=dict(C=48, heads=8)), "head dim 6 .* is no multiple of 4"), (dict(geom=dict(C=48)), "C = 48 is no multiple of the MX block size 32"),
    (dict(geom=dict(C=352, heads=11)), "C = 352 is above 320"), (dict(x=torch.zeros(1, 8, 8, 32)), "x holds 2048 elements, expected 4096"),
    (dict(x=torch.zeros(64, 64).double()), "x must be an fp32 tensor"), (dict(x=torch.zeros(64, 64).t()), "x must be contiguous"),
    (dict(x=torch.zeros(128, 32)), "x must be \\[..., 64\\]"), (dict(ln_weight=torch.ones(32)), "ln_weight"), (dict(ln_bias=torch.ones(64).double()), "ln_bias"),
    (dict(act_fmt="fp8"), "unknown MX format 'fp8'"), (dict(wqkv=torch.zeros(192, 64)), "wqkv must be an MXOperand"),
    (dict(wqkv=(128, 64)), "wqkv is \\[128, 64\\] and wproj \\[64, 64\\]"), (dict(wproj=(64, 96)), "wproj \\[64, 96\\]"),
    (dict(wproj=(64, 64, "mxfp8_e4m3", 8)), "one weight format"), (dict(bqkv=torch.ones(64)), "bqkv"), (dict(bproj=torch.ones(192)), "bproj"),
    (dict(bias=torch.zeros(2, 64, 63)), "bias holds"), (dict(out=torch.zeros(64, 63)), "out must be a contiguous fp32 \\[64, 64\\]"),
    (dict(want="ln"), "want must be a sequence"), (dict(want=("ln", "ln")), "distinct names"), (dict(want=("out",)), "distinct names"),
    (dict(), "no CPU path")])
def test_wrapper_refuses_malformed_arguments(no_library, kw, why):
    ops = no_library
    kw = dict(kw)
    g = dict(GOOD, **kw.pop("geom", {}))
    k = dict(d=ops.attn_desc(*[g[n] for n in ("B", "H", "W", "C", "heads", "window", "shift")]), x=torch.zeros(64, 64), ln_weight=torch.ones(64),
             ln_bias=torch.ones(64), wqkv=(192, 64), bqkv=torch.ones(192), wproj=(64, 64), bproj=torch.ones(64), bias=torch.zeros(2, 64, 64),
             act_fmt="mxfp8_e4m3")
    k.update(kw)
    k.update({n: _operand(ops, *k[n]) for n in ("wqkv", "wproj") if isinstance(k[n], tuple)})
    with pytest.raises(ValueError, match=f"mx_swin_attn: .*{why}"):
        ops.mx_swin_attn(*[k.pop(n) for n in ("d", "x", "ln_weight", "ln_bias", "wqkv", "bqkv", "wproj", "bproj", "bias", "act_fmt")], **k)


def _swin_gelu(b, monkeypatch):
    b.mlp.act = nn.GELU(approximate="tanh")


def _attn_quant(b, monkeypatch):
    b.attn.trained = b.attn.use_act_quant = True


def _proj_int(b, monkeypatch):
    from quantization.quantizer import UniformAffineQuantizer
    b.attn.proj.weight_quantizer = UniformAffineQuantizer(n_bits=8, channel_wise=True, scale_method="max")


def _proj_fmt(b, monkeypatch):
    from quantization.mx import MXQuantizer
    b.attn.proj.weight_quantizer = MXQuantizer("mxfp8_e4m3")


def _cap(b, monkeypatch):
    from hipops import _lib as L
    monkeypatch.setattr(L, "MXSWINATTN_MAX_C", 16)


def _proj_act(b, monkeypatch):
    b.attn.proj.activation_function = nn.ReLU()


def _qkv_quant(b, monkeypatch):
    b.attn.qkv.trained = b.attn.qkv.use_act_quant = True


# each change alone, on top of ALL the later ones: the reason reported is the first in the stated order
REASONS = [(_swin_gelu, "not the exact-erf nn.GELU"), (_attn_quant, "its activation quantiser rounds the probabilities"),
           (_proj_int, "attn.proj: its weight quantiser is a UniformAffineQuantizer"), (_proj_fmt, "qkv's weights are in mxfp4 and proj's in mxfp8_e4m3"),
           (_cap, "its 32 channels are above 16"), (_proj_act, "attn.proj has an se_module or an activation function"),
           (_qkv_quant, "an activation quantiser is active on qkv or proj")]


@pytest.mark.parametrize("first", range(len(REASONS)))
def test_native_swin_attn_refusal_reasons_in_order(first, monkeypatch):
    from quantization.mx import native_swin_attn, native_swin_attn_refusal
    qnn = swin_model()
    qnn.set_weight_format("mxfp4")
    b = qnn.model.rstb.residual_group.blocks[0]
    assert native_swin_attn_refusal(b) is None
    for change, _ in reversed(REASONS[first:]):                                 # (the earlier of two changes to one attribute wins)
        change(b, monkeypatch)
    assert REASONS[first][1] in native_swin_attn_refusal(b)
    with pytest.raises(ValueError, match="native_swin_attn: "):
        native_swin_attn(b, torch.zeros(1, 64, 32), 8, 8, "mxfp4")


def test_set_mx_activations_fused_attention_switch_and_report():
    qnn = swin_model()
    qnn.set_weight_format("mxfp4")
    qnn.set_quant_state(True, False)
    for kw in (dict(fused_attention=True), dict(fused_attention=True, swin=True), dict(fused_attention=True, attention=True),
               dict(fused_attention=1, swin=True, attention=True), dict(fused_attention=True, swin=True, attention=True, p_fmt="mxfp4")):
        with pytest.raises(ValueError, match="set_mx_activations: fused_attention must be True or False, and True only with swin=True, attention=True"):
            qnn.set_mx_activations("mxfp8_e4m3", **kw)
        assert not any(hasattr(m, "mx_swin_attn") or getattr(m, "mx_activations", None) for m in qnn.modules())
    blocks = qnn.model.rstb.residual_group.blocks
    on = dict(swin=True, attention=True, fused_attention=True)
    rep = qnn.set_mx_activations("mxfp8_e4m3", p_fmt="mxfp8_e4m3", **on)
    assert dict(rep["swin_attn"]) == {BLOCKS + i: tuple(f"{BLOCKS}{i}.{n}" for n in ("norm1", "attn.qkv", "attn.proj")) for i in "01"}
    assert not rep["left"] and all(b.mx_swin_attn is True and b._mx_swin_attn_on("mxfp8_e4m3") for b in blocks)
    # a refused block keeps the five launches; another state of proj leaves them in charge without a new call
    blocks[1].attn.proj.trained = blocks[1].attn.proj.use_act_quant = True
    rep = qnn.set_mx_activations("mxfp8_e4m3", **on)
    assert list(rep["swin_attn"]) == [BLOCKS + "0"] and list(rep["swin"]) == [BLOCKS + "0", BLOCKS + "1"] and not blocks[1].mx_swin_attn
    assert rep["left"][BLOCKS + "1"] == "the attention half keeps its five launches: an activation quantiser is active on qkv or proj"
    blocks[1].attn.proj.trained = blocks[1].attn.proj.use_act_quant = False
    blocks[0].attn.proj.mx_activations = ("mxfp8_e4m3", "emulated")
    assert not blocks[0]._mx_swin_attn_on("mxfp8_e4m3")
    # cleared like mx_swin
    assert "swin_attn" not in qnn.set_mx_activations("mxfp8_e4m3", swin=True, attention=True) and not any(b.mx_swin_attn for b in blocks)
    qnn.set_mx_activations("mxfp8_e4m3", **on)
    qnn.set_mx_activations(None)
    assert not any(b.mx_swin_attn or b.mx_swin for b in blocks)
