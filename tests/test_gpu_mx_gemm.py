"""GPU checks of the MX codes on the block-scaled matrix instruction (include/rdo_ptq_mxgemm.h) against tests/mx_gemm_reference.py:
the packed operand byte for byte, the fused quantise-and-pack against `mx_fakequant` + `mx_pack_codes` bit for bit, the GEMM on exact
data for all 25 format pairs (operand layout, scale-to-lane map, M / N / K tails), every element code through an identity, random
products, `mx.native_linear` on a Linear and a 1x1 conv (round to nearest and learned rounding) and `QuantModel.mx_native_report`.

The allowed difference of a random product is derived, nothing in it is measured: with exact products a_k b_k, y is a sum of K exact
terms and the bias formed by at most K fp32 additions in some order; each addition, under round to nearest or truncation, errs by at
most 2^-23 of its result, which no partial sum's magnitude exceeds sum |a_k b_k| + |bias| (1 + K 2^-23 is absorbed by the slack between
the unit roundoff 2^-24 of round to nearest and 2^-23).

The premise -- exact products, fp32 additions -- is the instruction's own for FP4 and FP6 elements.  Given eight neighbouring FP8
products it adds them aligned to the largest and drops what lies more than about 14 bits below it (448 + 2^-5 comes out exact,
448 + 2^-6 comes out 448; the same for E5M2), and a first kernel that issued one instruction per K step missed the bound on the two
cases with mxfp8_e4m3 activations (7.70e-05 and 2.55e-05 of sum |a b|: 3.06 and 1.08 times the bound).  The kernel therefore issues
eight instructions per K step for a pair with an FP8 operand, each with one element of every eight kept.  Measured on the MI355X,
max |y - ref| / sum |a b| of the random products next to the reference's k-ordered fp32 chain:
  mxfp8_e4m3 x mxfp8_e4m3   4.65e-08 (chain 4.68e-08)      mxfp4 weights x mxfp8_e4m3 activations   3.71e-08 (chain 3.71e-08)
  mxfp6_e2m3 x mxfp6_e2m3   3.60e-08 (chain 3.60e-08)      mxfp4 x mxfp4                            3.71e-08 (chain 3.71e-08)
The module and report tests put the activations on mxfp6_e2m3; the report test also runs the default mxfp8_e4m3 and prints its row."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mx_gemm_reference as G
import mx_reference as R
from test_mx_gemm_args import AQ, WQ, two_layer_model

pytestmark = pytest.mark.gpu


def _student(rows, inner):
    """heavy-tailed rows: Student-t(3) x 0.01, seeded"""
    torch.manual_seed(1000 * rows + inner)
    return (torch.distributions.StudentT(3.0).sample((rows, inner)) * 0.01).float().contiguous()


def _operand(codes, scales, fmt):
    from hipops import ops
    return ops.mx_pack_codes(G.to_torch(codes).cuda(), G.to_torch(scales).cuda(), fmt)


def _bound(a64, b64, bias, K):
    tol = G.abs_product64(a64, b64)
    if bias is not None:
        tol = tol + np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return K * 2.0 ** -23 * tol


# ----------------------------------------------------------------------------- 1. pack
@pytest.mark.parametrize("fmt", R.NAMES)
@pytest.mark.parametrize("K", [32, 96])
def test_pack_equals_the_reference_and_unpack_inverts_it(fmt, K):
    from hipops import ops
    rng = np.random.default_rng(K + R.FORMATS[fmt][0])
    codes = rng.integers(0, 1 << R.element_bits(fmt), (3, K)).astype(np.uint8)
    scales = rng.integers(100, 150, (3, K // 32)).astype(np.uint8)
    op = _operand(codes, scales, fmt)
    assert (op.rows, op.K, op.fmt) == (3, K, fmt) and op.packed.dtype == torch.uint8
    assert (op.packed.cpu().numpy() == G.pack(codes, fmt)).all()
    assert (op.scales.cpu().numpy() == scales).all()
    assert (ops.mx_unpack_codes(op).cpu().numpy() == codes).all()


# ----------------------------------------------------------------------------- 2. quantise and pack
@pytest.mark.parametrize("fmt", R.NAMES)
def test_quant_pack_equals_fakequant_then_pack_bit_for_bit(fmt):
    from hipops import ops
    x = _student(5, 160).clone()
    x[1, 32:64] = 0.0                                                                   # an all-zero block
    x[2, 5], x[2, 6], x[3, 64:96] = 1e-41, -3e-45, x[3, 64:96] * 1e-36                  # fp32 subnormals, a block of them
    x[4, 0] = -0.0
    xg = x.cuda()
    ref = ops.mx_fakequant(xg, fmt, want=("wq", "scales", "codes"))
    want = ops.mx_pack_codes(ref["codes"], ref["scales"], fmt)
    op, xq = ops.mx_quant_pack(xg, fmt, want_xq=True)
    assert torch.equal(op.packed, want.packed) and torch.equal(op.scales, ref["scales"])
    assert torch.equal(xq.view(torch.int32), ref["wq"].view(torch.int32))
    only = ops.mx_quant_pack(xg, fmt)
    assert torch.equal(only.packed, want.packed) and torch.equal(only.scales, ref["scales"])
    # ... and both are the CPU reference
    q = R.quantize(x, fmt)
    assert (op.packed.cpu().numpy() == G.pack(q["codes"].numpy(), fmt)).all() and torch.equal(op.scales.cpu(), q["scales"])


# ----------------------------------------------------------------------------- 3. exact product
def _exact(fa, fb, M, N, K, seed):
    from hipops import ops
    c = G.exact_case(fa, fb, M, N, K, seed)
    y = ops.mx_gemm(_operand(c["a_codes"], c["a_scales"], fa), _operand(c["b_codes"], c["b_scales"], fb), G.to_torch(c["bias"]).cuda())
    assert y.shape == (M, N) and y.dtype == torch.float32
    got = y.cpu().numpy().astype(np.float64)
    wrong = np.argwhere(got != c["ref"])
    assert wrong.size == 0, (fa, fb, M, N, K, len(wrong), wrong[:8].tolist())
    y0 = ops.mx_gemm(_operand(c["a_codes"], c["a_scales"], fa), _operand(c["b_codes"], c["b_scales"], fb))
    assert (y0.cpu().numpy().astype(np.float64) == c["ref"] - c["bias"].astype(np.float64)[None, :]).all()


@pytest.mark.parametrize("fb", R.NAMES)
@pytest.mark.parametrize("fa", R.NAMES)
def test_exact_product_for_every_format_pair(fa, fb):
    _exact(fa, fb, 16, 16, 128, seed=R.NAMES.index(fa) * 5 + R.NAMES.index(fb))


@pytest.mark.parametrize("shape", G.EXACT_SHAPES)
@pytest.mark.parametrize("pair", G.EXACT_PAIRS)
def test_exact_product_with_tails(pair, shape):
    _exact(*pair, *shape, seed=25 + G.EXACT_PAIRS.index(pair) * 4 + G.EXACT_SHAPES.index(shape))


# ----------------------------------------------------------------------------- 4. every element code
@pytest.mark.parametrize("fmt", R.NAMES)
def test_every_finite_element_code_decodes_as_the_project_decodes_it(fmt):
    from hipops import ops
    n = 1 << R.element_bits(fmt)
    fin = G.finite_codes(fmt)
    a = np.zeros((n, 32), np.uint8)
    a[fin, fin % 32] = fin
    eye = np.zeros((32, 32), np.uint8)
    eye[np.arange(32), np.arange(32)] = G.code_of(1.0, fmt)
    b = _operand(eye, np.full((32, 1), 127, np.uint8), fmt)
    for s in (127, 120, 134):
        sc = np.full((n, 1), s, np.uint8)
        y = ops.mx_gemm(_operand(a, sc, fmt), b).cpu().numpy().astype(np.float64)
        want = G.decode(a, sc, fmt)                                                 # the identity picks column k = n
        assert (y == want).all(), (fmt, s, np.argwhere(y != want)[:8].tolist())


# ----------------------------------------------------------------------------- 5. random product
@pytest.mark.parametrize("w_fmt,a_fmt", [("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp6_e2m3"), ("mxfp4", "mxfp4"), ("mxfp4", "mxfp8_e4m3")])
def test_random_product_stays_within_the_derived_bound(w_fmt, a_fmt):
    from hipops import ops
    x, w = _student(70, 192), _student(45, 192) * 3.0
    torch.manual_seed(2)
    bias = (torch.randn(45) * 0.01).float()
    a, xq = ops.mx_quant_pack(x.cuda(), a_fmt, want_xq=True)
    q = ops.mx_fakequant(w.cuda(), w_fmt, want=("codes", "scales", "wq"))
    b = ops.mx_pack_codes(q["codes"], q["scales"], w_fmt)
    y = ops.mx_gemm(a, b, bias.cuda()).cpu().numpy().astype(np.float64)
    a64 = G.decode(ops.mx_unpack_codes(a).cpu().numpy(), a.scales.cpu().numpy(), a_fmt)
    b64 = G.decode(q["codes"].cpu().numpy(), q["scales"].cpu().numpy(), w_fmt)
    assert (a64 == xq.cpu().double().numpy()).all() and (b64 == q["wq"].cpu().double().numpy()).all()
    ref = G.product64(a64, b64, bias.numpy())
    tol = _bound(a64, b64, bias.numpy(), 192)
    s = G.abs_product64(a64, b64)
    chain = G.chain32(a64, b64, bias.numpy()).astype(np.float64)
    print(f"mx_gemm {w_fmt} x {a_fmt}: max |y - ref| / sum|ab| = {np.max(np.abs(y - ref) / s):.3e}, "
          f"k-ordered fp32 chain {np.max(np.abs(chain - ref) / s):.3e}")
    assert np.isfinite(y).all() and (np.abs(y - ref) <= tol).all(), float(np.max(np.abs(y - ref) / tol))


# ----------------------------------------------------------------------------- 6. module level
def _module(org, fmt, learned):
    from quantization import QuantModule
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer
    m = QuantModule(org, WQ, AQ).cuda()
    m.weight_quantizer = (MXAdaRoundQuantizer if learned else MXQuantizer)(fmt).cuda()
    m.set_quant_state(True, False)
    return m


@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_native_linear_on_a_module(kind, learned):
    from hipops import ops
    from quantization.mx import native_linear, native_operand
    torch.manual_seed(17)
    w_fmt, a_fmt = "mxfp6_e2m3", "mxfp6_e2m3"                                           
    if kind == "linear":
        m, x, K, N = _module(nn.Linear(96, 40), w_fmt, learned), torch.randn(2, 9, 96).cuda(), 96, 40
        rows = x.reshape(-1, K)
    else:
        m, x, K, N = _module(nn.Conv2d(64, 24, 1), w_fmt, learned), torch.randn(2, 64, 5, 7).cuda(), 64, 24
        rows = x.permute(0, 2, 3, 1).reshape(-1, K).contiguous()
    if learned:
        g = torch.Generator().manual_seed(5)
        m.weight_quantizer.alpha = (torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1).cuda()     # a random sign pattern: up or down
    y = native_linear(m, x, a_fmt)
    assert tuple(y.shape) == ((2, 9, 40) if kind == "linear" else (2, 24, 5, 7))
    y2 = (y.reshape(-1, N) if kind == "linear" else y.permute(0, 2, 3, 1).reshape(-1, N)).cpu().numpy().astype(np.float64)
    # the forwarded weight: what the module's own quantised forward multiplies with
    wf = m.weight_quantizer(m.weight).detach().reshape(N, K).cpu().double().numpy()
    if learned:
        rtn = ops.mx_fakequant(m.weight.detach().reshape(N, K).contiguous(), w_fmt)["wq"].cpu().double().numpy()
        assert 0.2 < float((wf != rtn).mean()) < 0.8                                  # the learned rounding moved about half of them
    op = native_operand(m)
    assert (G.decode(ops.mx_unpack_codes(op).cpu().numpy(), op.scales.cpu().numpy(), w_fmt) == wf).all()
    assert native_operand(m) is op                                                      # memoised ...
    m.drop_weight_pack()
    assert native_operand(m) is not op                                                  # ... and dropped with the weight pack
    _, xq = ops.mx_quant_pack(rows, a_fmt, want_xq=True)
    a64 = xq.cpu().double().numpy()
    bias = m.bias.detach().cpu().numpy()
    ref = G.product64(a64, wf, bias)
    assert (np.abs(y2 - ref) <= _bound(a64, wf, bias, K)).all()


def test_native_linear_refuses_a_linear_whose_input_is_no_multiple_of_the_block():
    from quantization.mx import native_linear
    m = _module(nn.Linear(40, 8), "mxfp4", False)
    with pytest.raises(ValueError, match="native_operand: module QuantModule\\(linear, .*its 40 input channels are no multiple of the MX block size 32"):
        native_linear(m, torch.zeros(3, 40).cuda(), "mxfp8_e4m3")


# ----------------------------------------------------------------------------- 7. the report
def test_report_on_a_two_layer_model():
    from hipops import _lib as L
    from hipops import ops
    from quantization import QuantModule
    from quantization import mx
    qnn = two_layer_model().cuda()
    qnn.set_weight_format("mxfp6_e2m3")
    qnn.set_quant_state(True, False)
    mods = [m for m in qnn.modules() if isinstance(m, QuantModule)]
    before = [(id(m.weight_quantizer), id(m.act_quantizer), m.use_weight_quant, m.use_act_quant, m.trained, len(m._forward_pre_hooks),
               len(m._forward_hooks)) for m in mods]
    torch.manual_seed(23)
    images = torch.rand(2, 3, 32, 32)
    # the same tensors, taken by a hook of the test's own
    seen = []
    last = mods[-1]
    h = last.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    try:
        rep = qnn.mx_native_report(images, act_fmt="mxfp6_e2m3", batch=2)
    finally:
        h.remove()
    assert list(rep["modules"]) == ["2"] and list(rep["skipped"]) == ["0"] and "kernel (3, 3)" in rep["skipped"]["0"]
    assert (rep["act_fmt"], rep["n"], rep["batch"]) == ("mxfp6_e2m3", 2, 2)
    row = rep["modules"]["2"]
    assert (row["unit"], row["rows"], row["K"], row["N"], row["w_fmt"], row["act_fmt"]) == ("2", 2 * 32 * 32, 32, 16, "mxfp6_e2m3", "mxfp6_e2m3")
    assert np.isfinite(row["rel_l2"]) and np.isfinite(row["max_abs_diff"]) and 10.0 < row["act_sqnr_db"] < 60.0
    # the bound, from the same tensors: K 2^-23 |sum |a b|| / |emulated| = 2^-18 of the products' mass at K = 32; the native sum is one
    # step of the instruction and the bias, the emulation an fp32-accurate kernel: both lie a few 2^-24 from the exact product
    assert len(seen) == 1
    rows = seen[0].permute(0, 2, 3, 1).reshape(-1, 32).contiguous()
    a, xq = ops.mx_quant_pack(rows, "mxfp6_e2m3", want_xq=True)
    b = mx.native_operand(last)
    a64 = xq.cpu().double().numpy()
    b64 = G.decode(ops.mx_unpack_codes(b).cpu().numpy(), b.scales.cpu().numpy(), "mxfp6_e2m3")
    bias = last.bias.detach().cpu().numpy()
    exact = G.product64(a64, b64, bias)
    wdec = ops.mx_dequant(ops.mx_unpack_codes(b), b.scales, b.K, b.fmt)
    emulated = ops.conv2d_fwd_pack(xq.reshape(1, 1, -1, 32), ops.WeightPack(wdec.reshape(16, 1, 1, 32), last.bias.detach().contiguous()), 1, 0,
                                   epilogue=L.EPI_NONE).reshape(-1, 16).cpu().double().numpy()
    native = ops.mx_gemm(a, b, last.bias.detach().contiguous()).cpu().double().numpy()
    assert row["rel_l2"] == pytest.approx(np.linalg.norm(native - emulated) / np.linalg.norm(emulated), rel=1e-9, abs=1e-300)
    assert row["max_abs_diff"] == float(np.abs(native - emulated).max())
    cap = 32 * 2.0 ** -23 * np.linalg.norm(G.abs_product64(a64, b64)) / np.linalg.norm(emulated)
    print(f"mx_native_report: rel_l2 {row['rel_l2']:.3e}, cap {cap:.3e}, emulated vs exact {np.linalg.norm(emulated - exact) / np.linalg.norm(emulated):.3e}")
    assert row["rel_l2"] <= cap
    x64 = rows.cpu().double().numpy()
    assert row["act_sqnr_db"] == pytest.approx(10 * np.log10((x64 ** 2).sum() / ((x64 - a64) ** 2).sum()), rel=1e-9)
    fp8 = qnn.mx_native_report(images, batch=2)["modules"]["2"]                           # the default act_fmt, for the record
    print(f"mx_native_report: mxfp8_e4m3 activations rel_l2 {fp8['rel_l2']:.3e}, act_sqnr_db {fp8['act_sqnr_db']:.2f} (mxfp6_e2m3: {row['act_sqnr_db']:.2f})")
    assert fp8["act_fmt"] == "mxfp8_e4m3" and np.isfinite(fp8["rel_l2"]) and np.isfinite(fp8["act_sqnr_db"])
    after = [(id(m.weight_quantizer), id(m.act_quantizer), m.use_weight_quant, m.use_act_quant, m.trained, len(m._forward_pre_hooks),
              len(m._forward_hooks)) for m in mods]
    assert after == before
    # the model is left as found also when a forward raises
    def boom(mod, args):
        raise RuntimeError("a forward raised")
    h = mods[0].register_forward_pre_hook(boom)
    try:
        with pytest.raises(RuntimeError, match="a forward raised"):
            qnn.mx_native_report(images, batch=1)
    finally:
        h.remove()
    assert [(id(m.weight_quantizer), id(m.act_quantizer), m.use_weight_quant, m.use_act_quant, m.trained, len(m._forward_pre_hooks),
             len(m._forward_hooks)) for m in mods] == before
