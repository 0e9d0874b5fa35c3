"""The MX Swin kernels (include/rdo_ptq_mxswin.h) on the GPU: `ops.mx_layer_norm_pack` and `ops.mx_swin_mlp` against the launches they
replace, bit for bit, and against float64 stage by stage from the kernel's own optional outputs.  rows 70 (a ragged second tile) and 20
(fewer than a 32-row unit); (C, Hd) = (32, 64) and (96, 160): in the second pair neither K is a multiple of 128 and C / 4 = 24 leaves
lanes of the row phase idle; FP8 activations at C = 320 / Hd = 640 (70 016 B of LDS a workgroup) and at the maxima 512 / 1024 (108 032 B),
the launches above 64 KiB.  Heavy-tailed finite inputs
(test_gpu_mx_gemm._student).  The float64 bound is test_gpu_mx_gemm._bound's expression, K 2^-23 (sum |a b| + |bias|); the residual add
gives one more half ulp of |out|, with s the fp32 sum the contract states (`ops.add`).  Module level: the toy RSTB of
test_mx_swin_args.swin_model switched against un-switched, for equal bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mx_gemm_reference as G
from test_gpu_mx_gemm import _bound, _student
from test_gpu_swin_kernels import _rel
from test_mx_swin_args import swin_model

pytestmark = pytest.mark.gpu

PAIRS = [("mxfp4", "mxfp4"), ("mxfp6_e2m3", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp6_e3m2")]      # (activations, weights)
SHAPES = [(70, 32, 64), (20, 32, 64), (70, 96, 160), (20, 96, 160)]


def _case(rows, C, Hd, w_fmt):
    from hipops import ops
    g = torch.Generator().manual_seed(rows + C + Hd)
    t = dict(a=_student(rows, C) * 100, b=_student(rows + 1, C)[1:].contiguous() * 100, lw=1 + 0.3 * torch.randn(C, generator=g),
             lb=0.1 * torch.randn(C, generator=g), b1=0.1 * torch.randn(Hd, generator=g), b2=0.1 * torch.randn(C, generator=g))
    t = {k: v.cuda() for k, v in t.items()}
    t["w1"] = ops.mx_quant_pack((_student(Hd, C) * 10).cuda(), w_fmt)
    t["w2"] = ops.mx_quant_pack((_student(C, Hd) * 10).cuda(), w_fmt)
    return t


def _decode(op):
    from hipops import ops
    return G.decode(ops.mx_unpack_codes(op).cpu().numpy(), op.scales.cpu().numpy(), op.fmt)


def _same_operand(x, y):
    assert torch.equal(x.packed, y.packed) and torch.equal(x.scales, y.scales) and (x.fmt, x.rows, x.K) == (y.fmt, y.rows, y.K)


@pytest.mark.parametrize("fmt", ["mxfp4", "mxfp6_e2m3", "mxfp8_e5m2"])
@pytest.mark.parametrize("rows,C", [(70, 32), (20, 96), (70, 320), (33, 512)])
@pytest.mark.parametrize("addend,params", [(True, True), (False, True), (True, False)])
def test_layer_norm_pack_equals_add_layer_norm_then_quant_pack(fmt, rows, C, addend, params):
    from hipops import ops
    t = _case(rows, C, 32, "mxfp4")
    b, lw, lb = (t["b"] if addend else None), (t["lw"] if params else None), (t["lb"] if params else None)
    ln_ref = ops.add_layer_norm(t["a"], b, lw, lb)
    got = ops.mx_layer_norm_pack(t["a"], b, lw, lb, fmt, want_sum=addend, want_ln=True)
    _same_operand(got[0], ops.mx_quant_pack(ln_ref, fmt))
    assert torch.equal(got[-1], ln_ref)
    if addend:
        assert torch.equal(got[1], ops.add(t["a"], t["b"]))
    _same_operand(ops.mx_layer_norm_pack(t["a"], b, lw, lb, fmt), got[0])


@pytest.mark.parametrize("rows,C", [(513, 192), (65, 320)])
def test_layer_norm_pack_ln_against_float64(rows, C):
    """the statistic and the input distribution test_gpu_swin_kernels holds add_layer_norm to"""
    from hipops import ops
    g = torch.Generator().manual_seed(rows + C)
    a, b = torch.randn(rows, C, generator=g) * 2 + 0.3, torch.randn(rows, C, generator=g)
    w, bias = 1 + 0.3 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    y64 = F.layer_norm(a.double() + b.double(), (C,), w.double(), bias.double())
    _, ln = ops.mx_layer_norm_pack(a.cuda(), b.cuda(), w.cuda(), bias.cuda(), "mxfp8_e4m3", want_ln=True)
    assert _rel(ln.cpu().double(), y64) < 3e-6


@pytest.mark.parametrize("act_fmt,w_fmt,rows,C,Hd", [p + s for p in PAIRS for s in SHAPES] +
                         [("mxfp8_e4m3", "mxfp8_e4m3", 70, 320, 640), ("mxfp8_e5m2", "mxfp4", 70, 512, 1024)])
def test_swin_mlp_equals_the_eight_launches_bit_for_bit(act_fmt, w_fmt, rows, C, Hd):
    from hipops import ops
    t = _case(rows, C, Hd, w_fmt)
    s = ops.add(t["a"], t["b"])
    ln = ops.add_layer_norm(t["a"], t["b"], t["lw"], t["lb"])
    pre = ops.mx_gemm(ops.mx_quant_pack(ln, act_fmt), t["w1"], t["b1"])
    hidden = ops.mx_quant_pack(ops.gelu(pre), act_fmt)
    ref = ops.add(s, ops.mx_gemm(hidden, t["w2"], t["b2"]))
    out, ln_k, pre_k, hid_k = ops.mx_swin_mlp(t["a"], t["b"], t["lw"], t["lb"], t["w1"], t["b1"], t["w2"], t["b2"], act_fmt,
                                              want=("ln", "pre", "hidden"))
    assert torch.equal(ln_k, ln) and torch.equal(pre_k, pre)
    _same_operand(hid_k, hidden)
    assert torch.equal(out, ref)
    assert torch.equal(ops.mx_swin_mlp(t["a"], t["b"], t["lw"], t["lb"], t["w1"], t["b1"], t["w2"], t["b2"], act_fmt), ref)
    # no addend, no LayerNorm parameters, no biases
    ln0 = ops.add_layer_norm(t["a"], None, None, None)
    h0 = ops.mx_quant_pack(ops.gelu(ops.mx_gemm(ops.mx_quant_pack(ln0, act_fmt), t["w1"])), act_fmt)
    assert torch.equal(ops.mx_swin_mlp(t["a"], None, None, None, t["w1"], None, t["w2"], None, act_fmt), ops.add(t["a"], ops.mx_gemm(h0, t["w2"])))


@pytest.mark.parametrize("act_fmt,w_fmt", PAIRS)
@pytest.mark.parametrize("rows,C,Hd", SHAPES)
def test_swin_mlp_stages_against_float64(act_fmt, w_fmt, rows, C, Hd):
    from hipops import ops
    t = _case(rows, C, Hd, w_fmt)
    out, ln, pre, hidden = ops.mx_swin_mlp(t["a"], t["b"], t["lw"], t["lb"], t["w1"], t["b1"], t["w2"], t["b2"], act_fmt, want=("ln", "pre", "hidden"))
    w1, w2, b1, b2 = _decode(t["w1"]), _decode(t["w2"]), t["b1"].cpu().numpy(), t["b2"].cpu().numpy()
    a1 = _decode(ops.mx_quant_pack(ln, act_fmt))
    err = np.abs(pre.cpu().numpy().astype(np.float64) - G.product64(a1, w1, b1))
    print("pre: worst error / bound", float((err / _bound(a1, w1, b1, C)).max()))
    assert (err <= _bound(a1, w1, b1, C)).all()
    _same_operand(hidden, ops.mx_quant_pack(ops.gelu(pre), act_fmt))
    a2, o64 = _decode(hidden), out.cpu().numpy().astype(np.float64)
    ref = ops.add(t["a"], t["b"]).cpu().numpy().astype(np.float64) + G.product64(a2, w2, b2)
    tol = _bound(a2, w2, b2, Hd) + 2.0 ** -24 * np.abs(o64)
    print("out: worst error / bound", float((np.abs(o64 - ref) / tol).max()))
    assert (np.abs(o64 - ref) <= tol).all()


def test_switched_swin_blocks_give_the_bits_of_the_module_by_module_forward(monkeypatch, tmp_path):
    """`ops.layer_norm` (elementwise.hip: one wave a row) sums a row in another order than `add_layer_norm` (16 lanes a row), whose bits
    the fused launches keep.  The reference is therefore the same model with swin=False whose norm1 / norm2 forward goes through
    `ops.add_layer_norm` with no addend; everything else of it is the module-by-module forward as it stands."""
    from hipops import ops
    monkeypatch.setattr(ops, "layer_norm", lambda x, w, b, eps=1e-5, out=None: ops.add_layer_norm(x, None, w, b, eps))
    qnn = swin_model().cuda()
    qnn.set_weight_format("mxfp4")
    qnn.set_quant_state(True, False)
    x = torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(48)).cuda()
    outs = {}
    for swin in (False, True):
        rep = qnn.set_mx_activations("mxfp8_e4m3", "native", swin=swin)
        assert len(rep.get("swin", {})) == (2 if swin else 0)
        with torch.no_grad():
            outs[swin] = qnn(x).clone()
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])
    with pytest.raises(NotImplementedError, match="runs on MX activations .* and its input requires grad"):
        qnn(x.clone().requires_grad_())
    path = str(tmp_path / "swin.rdomx")
    qnn.save_mx_packed(path)
    fresh = swin_model().cuda()
    fresh.load_mx_packed(path)
    fresh.set_quant_state(True, False)
    assert not any(getattr(m, "mx_swin", False) for m in fresh.modules())
    with torch.no_grad():
        assert torch.equal(fresh(x), outs[True])
