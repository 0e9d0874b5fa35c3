"""The one-launch MX residual unit (include/rdo_ptq_mxresunit.h) on the GPU: `ops.mx_residual_unit` against the launches it replaces, bit for
bit, and against float64 stage by stage from the kernel's own optional outputs.  (B, H, W, N) = (1, 8, 8, 64): one tile, every border,
K = 288 of the 3x3; (2, 11, 13, 64): ragged tiles both ways, tile seams, the seam between the images of the batch; (1, 5, 3, 192):
smaller than a tile, N / 2 = 96 so the K steps of 128 straddle taps and the last one is short; (2, 9, 17, 192): all of that together;
FP8 at `MXRESUNIT_MAX_N`, the largest LDS images.  Heavy-tailed finite inputs (test_gpu_mx_gemm._student); biases of either sign, so
relu(b1) != 0 where the 3x3 must see zero padding.  The float64 bound is test_gpu_mx_gemm._bound's expression, K 2^-23 (sum |a b| +
|bias|); the residual add gives one more half ulp of |out|.  h1 and h2 leave the kernel packed, so their products are held to float64
through the fp32 result of the un-fused launch on the kernel's own operand, whose quantisation the packed output must equal (after
torch.relu: the packed epilogue's ReLU gives +0 where `ops.relu` gives 0 * v = -0, another code).  Module
level: the toy attention block of test_mx_resunit_args.attention_model switched against un-switched, for equal bits."""
import functools

import numpy as np
import pytest
import torch

import mx_conv_reference as CR
import mx_gemm_reference as G
from test_gpu_mx_gemm import _bound, _student
from test_gpu_mx_swin import PAIRS, _decode, _same_operand
from test_mx_resunit_args import UNITS, attention_model

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8, 64), (2, 11, 13, 64), (1, 5, 3, 192), (2, 9, 17, 192)]
CASES = [p + s for p in PAIRS for s in SHAPES] + [("mxfp8_e4m3", "mxfp8_e4m3", 1, 9, 10, 0)]      # N = 0: `MXRESUNIT_MAX_N`
WANT = ("xp", "h1", "h2", "branch")


@functools.lru_cache(maxsize=None)
def _case(B, H, W, N, w_fmt):
    """(x, w1, b1, w2, b2, w3, b3), left unchanged by every test"""
    from hipops import _lib as L
    from hipops import ops
    N = N or L.MXRESUNIT_MAX_N
    g = torch.Generator().manual_seed(B + H + W + N)
    x = (_student(B * H * W, N) * 100).cuda()
    ws = [ops.mx_quant_pack((_student(n, k) * 10).cuda(), w_fmt) for n, k in ((N // 2, N), (N // 2, 9 * N // 2), (N, N // 2))]
    bs = [(0.5 * torch.randn(n, generator=g)).cuda() for n in (N // 2, N // 2, N)]
    return x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2]


@pytest.mark.parametrize("act_fmt,w_fmt,B,H,W,N", CASES)
def test_residual_unit_equals_the_un_fused_sequence_bit_for_bit(act_fmt, w_fmt, B, H, W, N):
    from hipops import ops
    x, w1, b1, w2, b2, w3, b3 = _case(B, H, W, N, w_fmt)

    def sequence(b1, b2, b3):
        xp = ops.mx_quant_pack(x, act_fmt)
        h1 = ops.mx_gemm(xp, w1, b1, out_fmt=act_fmt, act="relu")
        h2 = ops.mx_conv2d(h1, w2, (B, H, W), 3, 1, 1, b2, out_fmt=act_fmt, act="relu")
        branch = ops.mx_gemm(h2, w3, b3)
        return ops.relu(ops.add(x, branch)), xp, h1, h2, branch

    ref = sequence(b1, b2, b3)
    got = ops.mx_residual_unit(x, (B, H, W), w1, b1, w2, b2, w3, b3, act_fmt, want=WANT)
    for r, k in zip(ref[1:4], got[1:4]):
        _same_operand(k, r)
    assert torch.equal(got[4], ref[4]) and torch.equal(got[0], ref[0]) and torch.isfinite(got[0]).all()
    assert torch.equal(ops.mx_residual_unit(x, (B, H, W), w1, b1, w2, b2, w3, b3, act_fmt), ref[0])
    assert torch.equal(ops.mx_residual_unit(x, (B, H, W), w1, None, w2, None, w3, None, act_fmt), sequence(None, None, None)[0])


@pytest.mark.parametrize("act_fmt,w_fmt,B,H,W,N", CASES)
def test_residual_unit_stages_against_float64(act_fmt, w_fmt, B, H, W, N):
    from hipops import ops
    x, w1, b1, w2, b2, w3, b3 = _case(B, H, W, N, w_fmt)
    N = x.shape[1]
    out, xp, h1, h2, branch = ops.mx_residual_unit(x, (B, H, W), w1, b1, w2, b2, w3, b3, act_fmt, want=WANT)
    _same_operand(xp, ops.mx_quant_pack(x, act_fmt))

    def held(name, y, a64, w, bias, K):
        b = bias.cpu().numpy()
        err, tol = np.abs(y.cpu().numpy().astype(np.float64).reshape(a64.shape[0], -1) - G.product64(a64, _decode(w), b)), _bound(a64, _decode(w), b, K)
        print(f"{name}: worst error / bound", float((err / tol).max()))
        assert (err <= tol).all()

    y1 = ops.mx_gemm(xp, w1, b1)
    held("h1", y1, _decode(xp), w1, b1, N)
    _same_operand(h1, ops.mx_quant_pack(torch.relu(y1), act_fmt))
    y2 = ops.mx_conv2d(h1, w2, (B, H, W), 3, 1, 1, b2)
    a2 = CR.im2col(_decode(h1), CR.im2col_index(B, H, W, 3, 1, 1))              # zeros in the padding, whatever relu(b1) is
    held("h2", y2, a2, w2, b2, 9 * N // 2)
    _same_operand(h2, ops.mx_quant_pack(torch.relu(y2.reshape(-1, N // 2)), act_fmt))
    held("branch", branch, _decode(h2), w3, b3, N // 2)
    o64 = out.cpu().numpy().astype(np.float64)
    ref = np.maximum(x.cpu().numpy().astype(np.float64) + G.product64(_decode(h2), _decode(w3), b3.cpu().numpy()), 0.0)
    tol = _bound(_decode(h2), _decode(w3), b3.cpu().numpy(), N // 2) + 2.0 ** -24 * np.abs(o64)
    print("out: worst error / bound", float((np.abs(o64 - ref) / np.maximum(tol, 1e-300)).max()))
    assert (np.abs(o64 - ref) <= tol).all()


def test_switched_residual_units_give_the_bits_of_the_module_by_module_forward():
    qnn = attention_model().cuda()
    qnn.set_weight_format("mxfp4")
    qnn.set_quant_state(True, False)
    x = torch.randn(2, 64, 11, 13, generator=torch.Generator().manual_seed(50)).cuda()
    outs = {}
    for on in (False, True):
        rep = qnn.set_mx_activations("mxfp8_e4m3", "native", residual_units=on)
        assert list(rep.get("residual_units", {})) == (UNITS if on else [])
        with torch.no_grad():
            outs[on] = qnn(x).clone()
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])
    with pytest.raises(NotImplementedError, match="runs on MX activations .* and its input requires grad"):
        qnn(x.clone().requires_grad_())
