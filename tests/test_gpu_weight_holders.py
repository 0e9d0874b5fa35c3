"""The trainable `_Op` and the frozen `_FpOp` take the kernel layouts of a weight from one place (quantization.engine._Weights):
for the same module both hold the same tensors, and neither owns a plane buffer before a recording asks for one."""
import pytest
import torch

from helpers import AQ, WQ

pytestmark = pytest.mark.gpu

MODULES = {
    "conv": lambda: torch.nn.Conv2d(16, 32, 3, stride=2, padding=1),
    "tconv": lambda: torch.nn.ConvTranspose2d(32, 48, 5, stride=2, padding=2, output_padding=1),
    "linear": lambda: torch.nn.Linear(32, 64),
}


@pytest.mark.parametrize("kind", list(MODULES))
def test_trainable_and_frozen_holders_share_their_layouts(kind):
    from quantization import QuantModule
    from quantization.engine import _Op, _Weights
    from quantization.swin_engine import _FpOp
    torch.manual_seed(0)
    qm = QuantModule(MODULES[kind](), WQ, AQ).cuda()
    a, b = _Op("layer", qm, False), _FpOp(qm)
    assert qm.kind == kind and isinstance(a, _Weights) and isinstance(b, _Weights)
    for n in ("w", "bias"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    for n in ("w4", "stride", "pad", "K", "tconv"):
        assert getattr(a, n) == getattr(b, n), n
    assert a.w4 == tuple(a.w.shape) and a.K == a.w4[1]
    assert a.tconv == ((2, 2, 1) if kind == "tconv" else None)
    assert (a.stride, a.pad) == ((2, 1) if kind == "conv" else (1, 0))
    assert (a.tc_phase is not None) == (b.tc_phase is not None) == (kind == "tconv")
    if kind == "tconv":
        from hipops import ops
        assert tuple(a.wp.shape) == tuple(b.wp.shape) == a.wp4 == b.wp4
        assert torch.equal(a.bias_p, b.bias_p)
        # `wp` is the phase form of the weight the kernels read: the frozen holder's of w, the trainable one's of its SOFT weight wq, which
        # starts up to delta / 2 away from w (1.1e-4 here), so as built the two differ.  Each is the expansion of its own ...
        assert torch.equal(a.wp, ops.tconv_expand(a.wq4(), a.tc_phase)) and torch.equal(b.wp, ops.tconv_expand(b.w, b.tc_phase))
        # ... and given the SAME weight the two holders make the same phase weight, bit for bit
        a.wq.copy_(a.w)
        a.expand_phase()
        assert torch.equal(a.wp, b.wp)
    else:
        assert a.wp is None and b.wp is None and a.bias_p is None and b.bias_p is None
    for h in (a, b):
        assert all(getattr(h, n) is None for n in _Weights.PLANE_BUFFERS), [n for n in _Weights.PLANE_BUFFERS if getattr(h, n) is not None]
        assert h.wbp is None
    assert set(_Weights.PLANE_BUFFERS) == {"wq_planes", "wd_planes", "wp_planes", "wp_h2", "wbp_planes", "lin_fwd", "lin_bwd"}
