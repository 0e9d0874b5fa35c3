"""The attention half of a Swin block in one MX launch (include/rdo_ptq_mxswinattn.h) on the GPU, stage by stage on the kernel's own data:
every stage output must equal, bit for bit, the existing op applied to the kernel's previous stage output; `qkv` and `branch` are also held
to float64 on the decoded operands (test_gpu_mx_gemm._bound: K 2^-23 (sum |a b| + |bias|)).  Every output starts as NaN and must come back
finite.  Inputs: x and the LayerNorm parameters of attention_cases.ln_inputs (rows far off zero, a constant row, a variance below eps), the
bias of attention_cases.trained_like, Linear weights with Laplace tails and per-output-channel scales over two decades as
helpers.trained_like_nic_ draws them.  Module level: the toy RSTB of test_mx_swin_args.swin_model with fused_attention=True against the
same model on the five launches."""
import numpy as np
import pytest
import torch

import attention_cases as AC
import mx_gemm_reference as G
from oracle import attention_oracle as A
from test_gpu_mx_gemm import _bound
from test_mx_swin_args import BLOCKS, swin_model

pytestmark = pytest.mark.gpu

PAIRS = [("mxfp4", "mxfp4"), ("mxfp6_e2m3", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp6_e3m2")]      # (activations, weights)
# (B, H, W, C, heads, window, shift): hd = 32; hd = 24 (blocks straddle heads), shifted, several windows a workgroup's loop could take;
# N = 16 < 32, hd = 16; N = 9, hd = 48; hd = 64
GEOMS = [(1, 8, 8, 64, 2, 8, 0), (2, 16, 16, 96, 4, 8, 4), (1, 8, 12, 64, 4, 4, 2), (1, 6, 6, 96, 2, 3, 1), (1, 8, 8, 128, 2, 8, 0)]
STAGES = ("ln", "qkv", "attn", "branch")


def _linear(n, k, gen):
    """[n, k] Laplace-tailed, variance-preserving, the rows' scales log-uniform over two decades"""
    u = torch.rand(n, k, generator=gen) - 0.5
    lap = -torch.sign(u) * torch.log1p(-2 * u.abs().clamp(max=0.4999999))
    s = 10.0 ** ((torch.rand(n, generator=gen) - 0.5) * 2.0)
    return lap / 2 ** 0.5 * k ** -0.5 * (s / s.pow(2).mean().sqrt()).view(-1, 1)


def _decode(op):
    from hipops import ops
    return G.decode(ops.mx_unpack_codes(op).cpu().numpy(), op.scales.cpu().numpy(), op.fmt)


def _against_float64(name, y, a, w, b, K):
    a64, w64 = _decode(a), _decode(w)
    tol = _bound(a64, w64, b.cpu().numpy(), K)
    ratio = float((np.abs(y.reshape(-1, w.rows).cpu().numpy().astype(np.float64) - G.product64(a64, w64, b.cpu().numpy())) / tol).max())
    print(f"  {name}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("act_fmt,w_fmt", PAIRS)
@pytest.mark.parametrize("geom", GEOMS)
def test_every_stage_on_the_kernels_own_data(geom, act_fmt, w_fmt):
    from hipops import ops
    print(f"\n{geom} {act_fmt} {w_fmt}")
    g = A.Geom(*geom)
    C, rows, gen = g.C, g.B * g.H * g.W, torch.Generator().manual_seed(sum(geom))
    x, lw, lb, _ = (t.cuda() for t in AC.ln_inputs(rows, C, sum(geom)))
    bias = AC.trained_like(g, sum(geom))[1].cuda()
    wqkv, wproj = ops.mx_quant_pack(_linear(3 * C, C, gen).cuda(), w_fmt), ops.mx_quant_pack(_linear(C, C, gen).cuda(), w_fmt)
    bqkv, bproj = (0.5 * torch.randn(3 * C, generator=gen)).cuda(), (0.5 * torch.randn(C, generator=gen)).cuda()
    d = ops.attn_desc(*g.args(), g.scale)
    out = torch.full((g.B, g.H, g.W, C), float("nan"), device="cuda")
    got = dict(zip(("out",) + STAGES, ops.mx_swin_attn(d, x.view(g.B, g.H, g.W, C), lw, lb, wqkv, bqkv, wproj, bproj, bias, act_fmt,
                                                        want=STAGES, out=out)))
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{name}: {int((~torch.isfinite(t)).sum())} elements not finite (never written?)"
    assert torch.equal(got["ln"].view(rows, C), ops.add_layer_norm(x, None, lw, lb))
    a1 = ops.mx_quant_pack(got["ln"].view(rows, C), act_fmt)
    assert torch.equal(got["qkv"].view(rows, 3 * C), ops.mx_gemm(a1, wqkv, bqkv))
    assert torch.equal(got["attn"], ops.mx_window_attention(d, got["qkv"], bias, act_fmt, act_fmt))
    a2 = ops.mx_quant_pack(got["attn"].view(rows, C), act_fmt)
    assert torch.equal(got["branch"].view(rows, C), ops.mx_gemm(a2, wproj, bproj))
    assert torch.equal(got["out"].view(rows, C), ops.add(x, got["branch"].view(rows, C)))
    _against_float64("qkv", got["qkv"], a1, wqkv, bqkv, C)
    _against_float64("branch", got["branch"], a2, wproj, bproj, C)
    # without the optional outputs, without LayerNorm parameters and biases
    assert torch.equal(ops.mx_swin_attn(d, x.view(g.B, g.H, g.W, C), lw, lb, wqkv, bqkv, wproj, bproj, bias, act_fmt), got["out"])
    o0, q0 = ops.mx_swin_attn(d, x, None, None, wqkv, None, wproj, None, bias, act_fmt, want=("qkv",))
    assert torch.equal(q0, ops.mx_gemm(ops.mx_quant_pack(ops.add_layer_norm(x, None, None, None), act_fmt), wqkv))
    a0 = ops.mx_quant_pack(ops.mx_window_attention(d, q0.view(g.B, g.H, g.W, 3 * C), bias, act_fmt).view(rows, C), act_fmt)
    assert torch.equal(o0, ops.add(x, ops.mx_gemm(a0, wproj)))


def test_fused_attention_blocks_give_the_bits_of_the_five_launches():
    qnn = swin_model().cuda()
    qnn.set_weight_format("mxfp4")
    qnn.set_quant_state(True, False)
    x = torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(50)).cuda()
    outs = {}
    for fused in (False, True):
        rep = qnn.set_mx_activations("mxfp8_e4m3", "native", swin=True, attention=True, fused_attention=fused)
        assert list(rep.get("swin_attn", {})) == ([BLOCKS + "0", BLOCKS + "1"] if fused else [])
        with torch.no_grad():
            outs[fused] = qnn(x).clone()
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])
    with pytest.raises(NotImplementedError, match="runs on MX activations .* and its input requires grad"):
        qnn(x.clone().requires_grad_())
    with pytest.raises(ValueError, match="set_mx_activations: fused_attention .* p_fmt"):
        qnn.set_mx_activations("mxfp8_e4m3", "native", swin=True, attention=True, fused_attention=True, p_fmt="mxfp4")
