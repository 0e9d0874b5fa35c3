"""CPU checks of the MX Swin kernels: include/rdo_ptq_mxswin.h against `EXPORTS_MXSWIN` and the built library, the refusals of the two C
entries (RDO_EINVAL without touching a device), of `ops.mx_layer_norm_pack` / `ops.mx_swin_mlp` before a pointer is taken, and of
`set_mx_activations(..., swin=...)` with the report of the switch and the reasons of `mx.native_swin_refusal`."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from test_mx_conv_args import AQ, RDO_EINVAL, ROOT, WQ, no_library  # noqa: F401  (no_library is a fixture)

BLOCKS = "rstb.residual_group.blocks."


class _OneRSTB(nn.Module):
    def __init__(self):
        import lic
        super().__init__()
        self.rstb = lic.RSTB(dim=32, input_resolution=(8, 8), depth=2, num_heads=2, window_size=4, mlp_ratio=2.0)

    def forward(self, x):
        return self.rstb(x, x.shape[2:])


def swin_model():
    """a toy Lu2022-style model: one RSTB of two Swin blocks (the second on shifted windows), embed 32, window 4, hidden width 64"""
    from quantization import QuantModel
    torch.manual_seed(47)
    return QuantModel(_OneRSTB().eval(), WQ, AQ).eval()


def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxswin.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXSWIN) == {"rdo_mx_layer_norm_pack", "rdo_mx_swin_mlp"}
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_MX, L.EXPORTS_MXGEMM, L.EXPORTS_MXCONV, L.EXPORTS_MXTCONV, L.EXPORTS_MXFILE, L.EXPORTS_MXCHAIN,
              L.EXPORTS_MXGDN)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert int(re.search(r"#define RDO_MXSWIN_MAX_C (\d+)", hdr).group(1)) == L.MXSWIN_MAX_C >= 320
    assert int(re.search(r"#define RDO_MXSWIN_MAX_HIDDEN (\d+)", hdr).group(1)) == L.MXSWIN_MAX_HIDDEN >= 640


def test_c_entries_refuse_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    base_addr = (C.addressof(buf) + 15) & ~15
    p, odd, by4 = C.c_void_p(base_addr), C.c_void_p(base_addr + 2), C.c_void_p(base_addr + 4)
    ln_names = ["a", "b", "w", "bias", "rows", "C", "eps", "fmt", "op", "os", "sum", "ln"]
    mlp_names = ["a", "b", "w", "bias", "eps", "rows", "C", "Hd", "fmt", "w1", "s1", "b1", "w2", "s2", "b2", "fw", "out", "ln", "pre", "hid", "hs"]
    shared = [dict(a=None), dict(rows=0), dict(C=0), dict(C=-32), dict(C=48), dict(C=L.MXSWIN_MAX_C + 32), dict(fmt=5), dict(fmt=-1),
              dict(a=by4), dict(b=by4), dict(w=by4), dict(bias=by4), dict(ln=by4)]
    entries = {"rdo_mx_layer_norm_pack": (ln_names, [dict(op=None), dict(os=None), dict(op=odd), dict(b=None, sum=p), dict(sum=by4)]),
               "rdo_mx_swin_mlp": (mlp_names, [dict(w1=None), dict(s1=None), dict(w2=None), dict(s2=None), dict(out=None), dict(Hd=0), dict(Hd=48),
                                               dict(Hd=L.MXSWIN_MAX_HIDDEN + 32), dict(fw=5), dict(hid=p), dict(hs=p), dict(hid=odd, hs=p),
                                               dict(w1=odd), dict(w2=odd), dict(b1=by4), dict(b2=by4), dict(out=by4), dict(pre=by4)])}
    for entry, (names, own) in entries.items():
        base = dict(a=p, b=p, w=p, bias=p, rows=70, C=96, Hd=160, eps=C.c_float(1e-5), fmt=3, fw=0, op=p, os=p, sum=None, ln=None, w1=p, s1=p, b1=p,
                    w2=p, s2=p, b2=p, out=p, pre=None, hid=None, hs=None)
        for kw in shared + own:
            a = dict(base, **kw)
            assert getattr(h, entry)(*[a[n] for n in names], None) == RDO_EINVAL, (entry, kw)
            assert h.rdo_last_error().startswith(entry.encode() + b": "), (entry, kw, h.rdo_last_error())


def test_wrappers_refuse_malformed_arguments(no_library):
    ops = no_library
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    w = lambda n, k, fmt="mxfp4", bits=4: ops.MXOperand(u8(n, k // 32 * 4 * bits), u8(n, k // 32), fmt, n, k)
    a, vec = torch.zeros(70, 64), torch.ones(64)
    ln_cases = [(dict(a=torch.zeros(70, 48)), "K = 48 is no multiple of the MX block size 32"), (dict(a=torch.zeros(2, 5, 64)), "a"),
                (dict(a=torch.zeros(4, 544), b=None, weight=None, bias=None), "C = 544 is above 512"), (dict(b=torch.zeros(70, 32)), "b"),
                (dict(weight=torch.ones(32)), "weight"), (dict(bias=vec.double()), "bias"), (dict(fmt="mxfp9"), "unknown MX format 'mxfp9'"),
                (dict(b=None, want_sum=True), "want_sum without a second addend"), (dict(), "no CPU path")]
    for kw, why in ln_cases:
        k = dict(dict(a=a, b=a, weight=vec, bias=vec, fmt="mxfp8_e4m3"), **kw)
        with pytest.raises(ValueError, match=f"mx_layer_norm_pack: .*{why}"):
            ops.mx_layer_norm_pack(k.pop("a"), k.pop("b"), k.pop("weight"), k.pop("bias"), k.pop("fmt"), **k)
    mlp_cases = [(dict(a=torch.zeros(70, 48)), "K = 48 is no multiple"), (dict(w1=u8(128, 32)), "w1 must be an MXOperand"),
                 (dict(w1=w(128, 96)), "w1 is \\[128, 96\\] and w2 \\[64, 128\\]"), (dict(w2=w(64, 160)), "w2 \\[64, 160\\]"),
                 (dict(w1=w(1056, 64), w2=w(64, 1056)), "Hd = 1056 is above 1024"), (dict(w2=w(64, 128, "mxfp8_e4m3", 8)), "one weight format"),
                 (dict(b1=torch.ones(64)), "b1"), (dict(b2=torch.ones(128)), "b2"), (dict(act_fmt="fp8"), "unknown MX format 'fp8'"),
                 (dict(want="ln"), "want must be a sequence"), (dict(want=("ln", "ln")), "distinct names"), (dict(want=("y",)), "distinct names"),
                 (dict(), "no CPU path")]
    for kw, why in mlp_cases:
        k = dict(dict(a=a, b=a, ln_weight=vec, ln_bias=vec, w1=w(128, 64), b1=torch.ones(128), w2=w(64, 128), b2=vec, act_fmt="mxfp8_e4m3"), **kw)
        with pytest.raises(ValueError, match=f"mx_swin_mlp: .*{why}"):
            ops.mx_swin_mlp(*[k.pop(n) for n in ("a", "b", "ln_weight", "ln_bias", "w1", "b1", "w2", "b2", "act_fmt")], **k)


def test_set_mx_activations_swin_switch_report_and_refusals():
    from quantization.mx import native_swin_refusal
    qnn = swin_model()
    qnn.set_weight_format("mxfp4")
    for kw in (dict(mode="emulated", swin=True), dict(swin=1), dict(swin=None)):
        with pytest.raises(ValueError, match="set_mx_activations: swin must be True or False, and True in mode 'native' only"):
            qnn.set_mx_activations("mxfp4", **kw)
        assert not any(hasattr(m, "mx_swin") or getattr(m, "mx_activations", None) for m in qnn.modules())
    blocks = qnn.model.rstb.residual_group.blocks
    rep = qnn.set_mx_activations("mxfp8_e4m3", swin=True)
    assert dict(rep["swin"]) == {BLOCKS + i: tuple(f"{BLOCKS}{i}.{n}" for n in ("norm2", "mlp.fc1", "mlp.fc2")) for i in "01"}
    assert all(rep["native"][f"{BLOCKS}{i}.{n}"] == "layernorm" for i in "01" for n in ("norm1", "norm2")) and not rep["left"]
    assert all(b.mx_swin is True and getattr(b.norm2, "mx_activations", None) is None for b in blocks)
    # an active output quantiser on norm2: the block keeps its forward, its LayerNorms stay under 'left'
    blocks[1].norm2.trained = blocks[1].norm2.use_act_quant = True
    rep = qnn.set_mx_activations("mxfp8_e4m3", swin=True)
    assert list(rep["swin"]) == [BLOCKS + "0"] and rep["left"][BLOCKS + "1"].startswith("an activation quantiser is active on norm1, norm2")
    assert f"{BLOCKS}1.norm2" in rep["left"] and blocks[0].mx_swin and not blocks[1].mx_swin
    blocks[1].norm2.trained = blocks[1].norm2.use_act_quant = False
    # swin=False and act_fmt=None clear the attribute; the LayerNorms are back under 'left'
    rep = qnn.set_mx_activations("mxfp8_e4m3")
    assert "swin" not in rep and f"{BLOCKS}0.norm1" in rep["left"] and not any(b.mx_swin for b in blocks)
    qnn.set_mx_activations("mxfp8_e4m3", swin=True)
    qnn.set_mx_activations(None)
    assert not any(b.mx_swin for b in blocks)
    # the other reasons
    b = blocks[0]
    b.mlp.act = nn.GELU(approximate="tanh")
    assert "not the exact-erf nn.GELU" in native_swin_refusal(b)
    b.mlp.act = nn.GELU()
    qnn.set_weight_format({"rstb": "int"})
    assert native_swin_refusal(b).startswith("attn.qkv: its weight quantiser is a UniformAffineQuantizer")
