"""CPU checks of the one-launch MX GDN / IGDN: include/rdo_ptq_mxgdn.h against `EXPORTS_MXGDN` and the built library, the refusals of the
two C entries (RDO_EINVAL without touching a device), of `ops.mx_gdn`, of `mx.native_gdn_refusal` / `native_gdn_chain_refusal`, and the
`gdn` flag of `set_mx_activations`."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from test_mx_conv_args import AQ, RDO_EINVAL, ROOT, WQ, _module, no_library  # noqa: F401  (no_library is a fixture)

NAMES = {"rdo_mx_gdn", "rdo_mx_gdn_packed"}


def gdn_model():
    """conv 32 -> 64, GDN(64), conv 64 -> 32, IGDN(32): both GDNs eligible, each followed or preceded by an eligible conv"""
    import lic
    from quantization import QuantModel
    torch.manual_seed(43)
    net = nn.Sequential(nn.Conv2d(32, 64, 3, padding=1), lic.GDN(64), nn.Conv2d(64, 32, 3, stride=2, padding=1), lic.GDN(32, inverse=True))
    return QuantModel(net.eval(), WQ, AQ).eval()


def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxgdn.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXGDN) == NAMES
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_MX, L.EXPORTS_MXGEMM, L.EXPORTS_MXCONV, L.EXPORTS_MXTCONV, L.EXPORTS_MXFILE, L.EXPORTS_MXCHAIN)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert int(re.search(r"#define RDO_MXGDN_MAX_C (\d+)", hdr).group(1)) == L.MXGDN_MAX_C >= 320


def test_c_entries_refuse_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    base_addr = (C.addressof(buf) + 15) & ~15
    p, odd, by4 = C.c_void_p(base_addr), C.c_void_p(base_addr + 2), C.c_void_p(base_addr + 4)
    head = ["x", "rows", "C", "fx", "g", "sg", "fg", "beta", "inverse"]
    entries = {"rdo_mx_gdn": (head + ["y", "norm"], [dict(y=None), dict(y=by4)]),
               "rdo_mx_gdn_packed": (head + ["fo", "yp", "ys", "norm"], [dict(fo=-1), dict(fo=5), dict(yp=None), dict(ys=None), dict(yp=odd)])}
    shared = [dict(x=None), dict(g=None), dict(sg=None), dict(beta=None), dict(rows=0), dict(C=0), dict(C=-32), dict(C=48),
              dict(C=L.MXGDN_MAX_C + 32), dict(fx=5), dict(fx=-1), dict(fg=5), dict(g=odd), dict(beta=odd), dict(inverse=2), dict(inverse=-1),
              dict(x=by4), dict(norm=by4)]
    for entry, (names, own) in entries.items():
        base = dict(x=p, rows=70, C=96, fx=3, g=p, sg=p, fg=0, beta=p, inverse=0, y=p, norm=None, fo=0, yp=p, ys=p)
        for kw in shared + own:
            a = dict(base, **kw)
            assert getattr(h, entry)(*[a[n] for n in names], None) == RDO_EINVAL, (entry, kw)
            assert h.rdo_last_error().startswith(entry.encode() + b": "), (entry, kw, h.rdo_last_error())


def test_wrapper_refuses_malformed_arguments(no_library):
    ops = no_library
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    g = lambda c, fmt="mxfp4", bits=4: ops.MXOperand(u8(c, c // 32 * 4 * bits), u8(c, c // 32), fmt, c, c)
    x, beta = torch.zeros(70, 64), torch.ones(64)
    cases = [(dict(x2d=torch.zeros(70, 48)), "K = 48 is no multiple of the MX block size 32"), (dict(x2d=torch.zeros(2, 5, 64)), "x2d"),
             (dict(x2d=torch.zeros(70, 64).t()), "x2d"), (dict(x2d=torch.zeros(0, 64)), "x2d is empty"), (dict(fmt="mxfp9"), "unknown MX format 'mxfp9'"),
             (dict(x2d=torch.zeros(4, 544), g=g(544), beta=torch.ones(544)), "C = 544 is above 512"), (dict(g=u8(64, 32)), "g must be an MXOperand"),
             (dict(g=g(96)), "g is \\[96, 96\\], x2d's 64 channels need \\[64, 64\\]"), (dict(beta=torch.ones(32)), "beta"),
             (dict(beta=torch.ones(64, dtype=torch.float64)), "beta"), (dict(out_fmt="fp8"), "unknown MX format 'fp8'"), (dict(), "no CPU path")]
    for kw, why in cases:
        a = dict(dict(x2d=x, g=g(64), beta=beta, fmt="mxfp8_e4m3"), **kw)
        with pytest.raises(ValueError, match=f"mx_gdn: .*{why}"):
            ops.mx_gdn(a.pop("x2d"), a.pop("g"), a.pop("beta"), a.pop("fmt"), **a)


def test_gdn_refusals_in_their_order_and_the_gdn_flag():
    import lic
    from quantization import mx
    from quantization.mx import MXQuantizer, native_gdn, native_gdn_chain, native_gdn_chain_refusal, native_gdn_refusal
    gdn = lambda c, q=True, **kw: _module(lic.GDN(c, **kw), MXQuantizer("mxfp4") if q else None)
    conv = lambda cin: _module(nn.Conv2d(cin, 32, 3, padding=1), MXQuantizer("mxfp4"))
    # the order: kind, C % 32, C above the limit, the quantiser -- each module below also fails every later test but the one named
    cases = [(_module(nn.Conv2d(48, 32, 1)), "a conv module is not a GDN"), (gdn(48, q=False), "its 48 channels are no multiple of the MX block size 32"),
             (gdn(544, q=False), "its 544 channels are above 512"), (gdn(64, q=False), "its weight quantiser is a UniformAffineQuantizer, not an MX"),
             (gdn(64), None), (gdn(512, inverse=True), None)]
    for m, why in cases:
        got = native_gdn_refusal(m)
        assert (got is None) if why is None else re.search(why, got), (why, got)
        if why is not None:
            with pytest.raises(ValueError, match="native_gdn_operand: module QuantModule\\("):
                native_gdn(m, torch.zeros(1, 64, 4, 4), "mxfp4")
    with_act, with_q = gdn(64), gdn(64)
    with_act.activation_function = nn.ReLU()
    with_q.use_act_quant = with_q.trained = True
    for pair, why in (((gdn(64), conv(64)), None), ((gdn(48), conv(64)), "gdn: its 48 channels"), ((gdn(64), conv(48)), "second: its 48 input channels"),
                      ((with_act, conv(64)), "gdn has an activation function of its own \\(ReLU\\)"), ((with_q, conv(64)), "gdn has an active output quantiser"),
                      ((gdn(64), conv(32)), "gdn's 64 channels are not second's 32 input channels")):
        got = native_gdn_chain_refusal(*pair)
        assert (got is None) if why is None else re.search(why, got), (why, got)
        if why is not None:
            with pytest.raises(ValueError, match="native_gdn_chain: modules QuantModule\\(.* -> QuantModule\\("):
                native_gdn_chain(*pair, torch.zeros(1, 64, 4, 4), "mxfp4")
    qnn = gdn_model()
    qnn.set_weight_format("mxfp4")
    left = "a gdn module is not GEMM-shaped: the native path serves Linears and 1x1 stride-1 convs"
    rep = qnn.set_mx_activations("mxfp8_e4m3")
    assert dict(rep["left"]) == {"1": left, "3": left} and dict(rep["native"]) == {"0": "conv", "2": "conv"}
    assert qnn.model[1].mx_activations is None and mx.native_kind(qnn.model[1]) == (None, left)
    with pytest.raises(ValueError, match="set_mx_activations: gdn must be True or False"):
        qnn.set_mx_activations("mxfp8_e4m3", gdn=1)
    rep = qnn.set_mx_activations("mxfp8_e4m3", "emulated", gdn=True)
    assert dict(rep["native"]) == {"0": "conv", "1": "gdn", "2": "conv", "3": "gdn"} and not rep["left"]
    assert qnn.model[3].mx_activations == ("mxfp8_e4m3", "emulated")
    with pytest.raises(NotImplementedError, match="runs on MX activations"):
        qnn.model[1]._refuse_mx_grad()
    with pytest.raises(NotImplementedError, match="reconstruct: module '.*' runs on MX activations"):
        mx.refuse_mx_activations("reconstruct", qnn.named_modules(), "calibration under MX activations is not built")
    qnn.set_mx_activations(None)
    assert all(getattr(m, "mx_activations", None) is None for m in qnn.modules())
