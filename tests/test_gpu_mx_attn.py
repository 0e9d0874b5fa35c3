"""The MX window attention (include/rdo_ptq_mxattn.h) on the GPU, stage by stage on the kernel's own data: the scores against
`ops.mx_gemm` on `ops.mx_quant_pack` of the padded q and k tiles, bit for bit; the probabilities against the float64 softmax of those scores
(the unit of oracle/attention_oracle.py with ds = 0, held to 4 x what a CPU fp32 restatement needs); `out` against `ops.mx_gemm` on the
packed probabilities and the packed transposed v, bit for bit, and against float64 on the decoded operands (test_gpu_mx_gemm._bound).
Every output starts as NaN and must come back finite.  Inputs: attention_cases.trained_like."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_cases as AC
import mx_gemm_reference as G
from oracle import attention_oracle as A
from test_gpu_attention import _persistent_condition, _smallest_batch
from test_gpu_mx_gemm import _bound
from test_mx_swin_args import swin_model

pytestmark = pytest.mark.gpu

PAIRS = [("mxfp4", "mxfp4"), ("mxfp6_e2m3", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp6_e3m2")]      # (q / k / v, probabilities)
GEOMS = [(1, 8, 8, 48, 2, 8, 0), (2, 16, 16, 96, 2, 8, 4), (1, 8, 12, 64, 4, 4, 2), (1, 6, 6, 40, 2, 3, 1), (1, 8, 8, 128, 2, 8, 0)]


def _pad32(t):
    """zero-pad the last dimension to a multiple of 32 -> contiguous [rows, K]"""
    return F.pad(t, (0, -t.shape[-1] % 32)).reshape(-1, t.shape[-1] + -t.shape[-1] % 32).contiguous()


def _item(op, i, rows):
    """rows i * rows .. of a packed operand as an operand of its own"""
    from hipops import ops
    return ops.MXOperand(op.packed[i * rows:(i + 1) * rows], op.scales[i * rows:(i + 1) * rows], op.fmt, rows, op.K)


def _decode(op):
    from hipops import ops
    return G.decode(ops.mx_unpack_codes(op).cpu().numpy(), op.scales.cpu().numpy(), op.fmt)


class Run:
    """one launch with both stage outputs, and the operands of the two products as `ops.mx_quant_pack` makes them from the kernel's data"""

    def __init__(self, geom, fmt, p_fmt, seed):
        from hipops import ops
        self.g = g = A.Geom(*geom)
        qkv, bias, _ = AC.trained_like(g, seed)
        self.d = ops.attn_desc(*g.args(), g.scale)
        self.qkv, self.bias, self.fmt, self.p_fmt = qkv.cuda(), bias.cuda(), fmt, p_fmt
        self.out = torch.full((g.B, g.H, g.W, g.C), float("nan"), device="cuda")
        _, self.scores, self.probs = ops.mx_window_attention(self.d, self.qkv, self.bias, fmt, p_fmt, out=self.out, want=("scores", "probs"))
        for name in ("out", "scores", "probs"):
            t = getattr(self, name)
            assert bool(torch.isfinite(t).all()), f"{name}: {int((~torch.isfinite(t)).sum())} elements not finite (never written?)"
        q, k, v = (t.cuda() for t in A.gather(g, qkv, 3))                       # [windows, heads, N, hd]
        self.items, self.Np = g.windows * g.heads, g.N + -g.N % 32
        self.qp, self.kp = ops.mx_quant_pack(_pad32(q), fmt), ops.mx_quant_pack(_pad32(k), fmt)
        self.pp = ops.mx_quant_pack(_pad32(self.probs.permute(0, 3, 1, 2)), p_fmt)
        self.vt = ops.mx_quant_pack(_pad32(v.transpose(-1, -2)), fmt)

    def scores_bit_for_bit(self):
        from hipops import ops
        g = self.g
        start = (self.bias.unsqueeze(0) + A.mask_of(g, torch.float32).cuda()).reshape(self.items, g.N, g.N)
        for i in range(self.items):
            ref = ops.mx_gemm(_item(self.qp, i, g.N), _item(self.kp, i, g.N)) * g.scale + start[i]
            assert torch.equal(self.scores[i // g.heads, :, :, i % g.heads], ref), i

    def probs_against_float64(self):
        s32 = self.scores.cpu()
        s = s32.double()
        mx = s.amax(2, keepdim=True)
        p = torch.softmax(s, 2)
        unit = p * (2 * A.U * (s - mx).abs() + 4 * A.U)
        e = torch.exp(s32 - s32.amax(2, keepdim=True))
        r32 = A.worst_ratio(e * (1.0 / e.sum(2, keepdim=True)), p, unit, A.P_FLOOR)
        got = A.worst_ratio(self.probs, p, unit, A.P_FLOOR)
        print(f"  probs: err / unit  restatement {r32:.3f}  kernel {got:.3f}  allowed {4 * r32:.3f}")
        assert got <= 4 * r32

    def out_bit_for_bit(self):
        from hipops import ops
        g = self.g
        o = torch.stack([ops.mx_gemm(_item(self.pp, i, g.N), _item(self.vt, i, g.hd)) for i in range(self.items)])
        assert torch.equal(self.out.cpu(), A.scatter(g, [o.view(g.windows, g.heads, g.N, g.hd).cpu()], torch.float32))

    def out_against_float64(self):
        g = self.g
        a, b = _decode(self.pp).reshape(self.items, g.N, self.Np), _decode(self.vt).reshape(self.items, g.hd, self.Np)
        ref = np.stack([G.product64(a[i], b[i]) for i in range(self.items)])
        tol = np.stack([_bound(a[i], b[i], None, self.Np) for i in range(self.items)])
        shape = (g.windows, g.heads, g.N, g.hd)
        ref, tol = (A.scatter(g, [torch.from_numpy(t).view(shape)], A.F64) for t in (ref, tol))
        ratio = A.worst_ratio(self.out, ref, tol)
        print(f"  out: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("fmt,p_fmt", PAIRS)
@pytest.mark.parametrize("geom", GEOMS)
def test_every_stage_on_the_kernels_own_data(geom, fmt, p_fmt):
    from hipops import ops
    print(f"\n{geom} {fmt} {p_fmt}")
    r = Run(geom, fmt, p_fmt, seed=sum(geom))
    r.scores_bit_for_bit()
    r.probs_against_float64()
    r.out_bit_for_bit()
    r.out_against_float64()
    assert torch.equal(ops.mx_window_attention(r.d, r.qkv, r.bias, fmt, p_fmt), r.out)       # without the optional outputs


def test_persistent_loop_probs_and_out_against_float64_and_determinism():
    """every workgroup takes at least two items: the prefetch into the other buffer, the table flip and the slot / heads walk of `attn_item`"""
    from hipops import ops
    geom = (3, 128, 128, 192, 6, 8, 4)
    r = Run((_smallest_batch(*geom),) + geom[1:], *PAIRS[1], seed=32)
    print(f"\npersistent: {_persistent_condition(r.g)} items")
    r.probs_against_float64()
    r.out_against_float64()
    assert torch.equal(ops.mx_window_attention(r.d, r.qkv, r.bias, r.fmt, r.p_fmt), r.out)


def test_switched_attention_module(tmp_path):
    from hipops import ops
    qnn = swin_model().cuda()
    qnn.set_weight_format("mxfp4")
    qnn.set_quant_state(True, False)
    attn = qnn.model.rstb.residual_group.blocks[0].attn
    x = torch.randn(3, 16, 32, generator=torch.Generator().manual_seed(49)).cuda()          # three windows of 4 x 4 tokens
    outs = {}
    for on in (False, True):
        rep = qnn.set_mx_activations("mxfp8_e4m3", "native", attention=on)
        assert len(rep.get("attention", {})) == (2 if on else 0)
        with torch.no_grad():
            outs[on] = attn(x).clone()
    with torch.no_grad():
        d = ops.attn_desc(3, 4, 4, 32, attn.num_heads, 4, 0, attn.scale)
        o = ops.mx_window_attention(d, attn.qkv(x).contiguous().view(3, 4, 4, 96), attn.position_bias(), "mxfp8_e4m3", "mxfp8_e4m3")
        ref = attn.proj(o.view(3, 16, 32))
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], ref) and not torch.equal(outs[True], outs[False])
    with pytest.raises(NotImplementedError, match="runs on MX activations .* and its input requires grad"):
        attn(x.clone().requires_grad_())
    path = str(tmp_path / "attn.rdomx")
    qnn.save_mx_packed(path)
    fresh = swin_model().cuda()
    fresh.load_mx_packed(path)
    assert not any(getattr(m, "mx_attention", None) for m in fresh.modules())
