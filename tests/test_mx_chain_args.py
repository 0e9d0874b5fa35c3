"""CPU checks of the packed-output MX kernels: include/rdo_ptq_mxchain.h against `EXPORTS_MXCHAIN` and the built library, the refusals
of the three C entries (RDO_EINVAL without touching a device), of the `ops` wrappers' `out_fmt` / `act`, of
`set_mx_activations(..., chain=True)` and the reasons of `mx.native_chain_refusal`."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from test_mx_conv_args import AQ, RDO_EINVAL, ROOT, WQ, _module, no_library  # noqa: F401  (no_library is a fixture)

NAMES = {"rdo_mx_gemm_packed", "rdo_mx_conv2d_packed", "rdo_mx_conv_transpose2d_packed"}


def block_model():
    """a ResidualBlock and a strided ResidualBlockWithStride of 32 -> 32 channels"""
    import lic
    from quantization import QuantModel
    torch.manual_seed(41)
    return QuantModel(nn.Sequential(lic.ResidualBlock(32, 32), lic.ResidualBlockWithStride(32, 32, stride=2)).eval(), WQ, AQ).eval()


def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxchain.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXCHAIN) == NAMES
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_MX, L.EXPORTS_MXGEMM, L.EXPORTS_MXCONV, L.EXPORTS_MXTCONV, L.EXPORTS_MXFILE)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    ids = dict(re.findall(r"#define RDO_MX_ACT_([A-Z]+) (\d)", hdr))
    assert {k.lower(): int(v) for k, v in ids.items()} == L.MX_ACTS


def test_c_entries_refuse_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p, odd = C.c_void_p(C.addressof(buf)), C.c_void_p(C.addressof(buf) + 2)
    tail = ["bias", "fo", "act", "yp", "ys"]
    conv = ["x", "sx", "fx", "w", "sw", "fw", "B", "H", "W", "C", "N", "k", "stride", "pad"]
    entries = {
        "rdo_mx_gemm_packed": (["x", "sx", "fx", "w", "sw", "fw", "M", "N", "K"] + tail, dict(M=70, K=192),
                               [dict(M=0), dict(K=40), dict(K=0)]),
        "rdo_mx_conv2d_packed": (conv + tail, dict(B=2, H=5, W=7, C=64, k=3, stride=1, pad=1), [dict(C=40), dict(k=9), dict(stride=0)]),
        "rdo_mx_conv_transpose2d_packed": (conv + ["opad"] + tail, dict(B=2, H=5, W=7, C=64, k=3, stride=2, pad=1, opad=1),
                                           [dict(C=40), dict(opad=2), dict(pad=-1)]),
    }
    shared = [dict(x=None), dict(sw=None), dict(w=odd), dict(bias=odd), dict(fx=5), dict(fw=-1), dict(N=0),      # the fp32 twin's
              dict(fo=-1), dict(fo=5), dict(act=-1), dict(act=3), dict(N=48), dict(N=24), dict(yp=None), dict(ys=None), dict(yp=odd)]
    for entry, (names, sizes, own) in entries.items():
        base = dict(x=p, sx=p, fx=0, w=p, sw=p, fw=3, N=96, bias=None, fo=0, act=1, yp=p, ys=p, **sizes)
        for kw in shared + own:
            a = dict(base, **kw)
            assert getattr(h, entry)(*[a[n] for n in names], None) == RDO_EINVAL, (entry, kw)
            assert h.rdo_last_error().startswith(entry.encode() + b": "), (entry, kw, h.rdo_last_error())


def test_wrappers_refuse_out_fmt_and_act_before_the_library(no_library):
    ops = no_library
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    x = ops.MXOperand(u8(70, 2 * 16), u8(70, 2), "mxfp4", 70, 64)                       # [2 * 5 * 7, 64]
    calls = {"mx_gemm": lambda n, **kw: ops.mx_gemm(x, ops.MXOperand(u8(n, 32), u8(n, 2), "mxfp4", n, 64), **kw),
             "mx_conv2d": lambda n, **kw: ops.mx_conv2d(x, ops.MXOperand(u8(n, 18 * 16), u8(n, 18), "mxfp4", n, 576), (2, 5, 7), 3, 1, 1, **kw),
             "mx_conv_transpose2d": lambda n, **kw: ops.mx_conv_transpose2d(x, ops.MXOperand(u8(n, 18 * 16), u8(n, 18), "mxfp4", n, 576),
                                                                            (2, 5, 7), 3, 2, 1, 1, **kw)}
    for what, call in calls.items():
        for n, kw, why in ((32, dict(act="lrelu"), "act 'lrelu' needs out_fmt"), (32, dict(out_fmt="mxfp4", act="gelu"), "unknown act 'gelu'"),
                           (32, dict(act=1), "unknown act 1"), (32, dict(out_fmt="mxfp9"), "unknown MX format 'mxfp9'"),
                           (24, dict(out_fmt="mxfp4"), "N = 24 is no multiple of the MX block size 32"),
                           (32, dict(out_fmt="mxfp8_e4m3", act="relu"), "no CPU path"), (24, dict(), "no CPU path")):
            with pytest.raises(ValueError, match=f"{what}: .*{why}"):
                call(n, **kw)


def test_chain_refusals_and_the_chain_flag():
    from quantization import mx
    from quantization.mx import MXQuantizer, native_chain, native_chain_refusal
    conv = lambda cin, cout, **kw: _module(nn.Conv2d(cin, cout, 3, padding=1, **kw), MXQuantizer("mxfp4"))
    tconv = _module(nn.ConvTranspose2d(32, 64, 5, stride=2, padding=2, output_padding=1), MXQuantizer("mxfp4", tconv=True))
    with_se, with_act, with_q = conv(32, 32), conv(32, 32), conv(32, 32)
    with_se.se_module = nn.Identity()
    with_act.activation_function = nn.ReLU()
    with_q.use_act_quant = with_q.trained = True
    cases = [((conv(32, 32), conv(32, 32)), None), ((tconv, conv(64, 32)), None), ((conv(32, 64), tconv), "first's 64 output channels are not second's 32"),
             ((_module(nn.Linear(32, 32), MXQuantizer("mxfp4")), conv(32, 32)), "first: a linear module is not a convolution"),
             ((conv(32, 32), conv(32, 32, dilation=2)), "second: a conv with kernel .* dilation \\(2, 2\\)"),
             ((with_se, conv(32, 32)), "first has an se_module"), ((with_act, conv(32, 32)), "first has an activation function of its own \\(ReLU\\)"),
             ((with_q, conv(32, 32)), "first has an active output quantiser"),
             ((conv(32, 16), conv(32, 32)), "first's 16 output channels are no multiple of the MX block size 32")]
    for pair, why in cases:
        got = native_chain_refusal(*pair)
        assert (got is None) if why is None else re.search(why, got), (why, got)
        if why is not None:
            with pytest.raises(ValueError, match="native_chain: modules QuantModule\\(.* -> QuantModule\\("):
                native_chain(*pair, torch.zeros(2, 32, 6, 7), "mxfp4")
    assert native_chain_refusal(conv(32, 48), conv(48, 32)) == "second: its 48 input channels are no multiple of the MX block size 32"
    qnn = block_model()
    qnn.set_weight_format("mxfp4")
    for kw in (dict(mode="emulated", chain=True), dict(chain=1), dict(chain=None)):
        with pytest.raises(ValueError, match="set_mx_activations: chain must be True or False, and True in mode 'native' only"):
            qnn.set_mx_activations("mxfp4", **kw)
        assert not any(hasattr(m, "mx_chain") or getattr(m, "mx_activations", None) for m in qnn.modules())
    rep = qnn.set_mx_activations("mxfp8_e4m3", chain=True)
    assert dict(rep["chained"]) == {"0": ("0.conv1", "0.conv2"), "1": ("1.conv1", "1.conv2")}
    assert qnn.model[0].mx_chain is True and qnn.model[1].mx_chain is True
    assert list(qnn.set_mx_activations("mxfp8_e4m3", units=["1"])) == ["native", "left"] and qnn.model[0].mx_chain and not qnn.model[1].mx_chain
    qnn.set_mx_activations(None)
    assert not qnn.model[0].mx_chain and mx.native_chain_refusal(qnn.model[0].conv1, qnn.model[0].conv2) is None
