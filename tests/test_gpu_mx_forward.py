"""GPU checks of the MX-activation forward mode (`QuantModel.set_mx_activations`) on the model of tests/test_mx_tconv_args.py --
3 -> 32 3x3 + LeakyReLU, 32 -> 32 3x3 + LeakyReLU, ConvTranspose2d(32 -> 32, 5, stride 2), 32 -> 16 1x1 and a Linear(32, 32) branch,
weights in mxfp4, a 2 x 3 x 8 x 8 image: every switched module's output is its own tail applied to `native_*` of its captured input
(mode 'native') or to the stated emulation (mode 'emulated') bit for bit; left modules, cleared modules and modules with weight
quantisation off give the bits of an untouched model; a grad-requiring input is refused; and the whole-model distance between the two
modes is smaller than the distance the activation grid itself makes.

Measured on the MI355X (mxfp4 weights, act_fmt mxfp8_e4m3, outputs (head, fc) concatenated):
  rel_l2(native, emulated) = 0 (equal bits)    rel_l2(native, no MX activations) = 7.304e-03"""
import numpy as np
import pytest
import torch

from test_mx_tconv_args import forward_model

pytestmark = pytest.mark.gpu

W_FMT, ACT_FMT = "mxfp4", "mxfp8_e4m3"
SWITCHED = ("conv", "up", "head", "fc")


def _model():
    qnn = forward_model().cuda()
    qnn.set_weight_format(W_FMT)
    qnn.set_quant_state(True, False)
    return qnn


def _image():
    torch.manual_seed(37)
    return torch.rand(2, 3, 8, 8).cuda()


def _run(qnn, x, capture=()):
    """the model's outputs and, per captured module name, (input, output) of its forward"""
    seen, handles = {}, []
    for name in capture:
        mod = getattr(qnn.model, name)
        handles.append(mod.register_forward_hook(lambda m, args, out, name=name: seen.__setitem__(name, (args[0].detach().clone(), out.detach().clone()))))
    try:
        with torch.no_grad():
            out = qnn(x)
    finally:
        for h in handles:
            h.remove()
    return tuple(o.detach().clone() for o in out), seen


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _tail(mod, pre):
    out = pre if mod.se_module is None else mod.se_module(pre)
    out = mod.activation_function(out.clone())
    if not mod.disable_act_quant and mod.use_act_quant and mod.trained:
        out = mod.act_quantizer(out, True)
    return out


def _emulation(mod, x):
    """xq of ops.mx_quant_pack(rows, act_fmt, want_xq=True), reshaped to the input, through the module's fp32 kernel call with EPI_NONE"""
    from hipops import _lib as L
    from hipops import ops
    pack = mod.weight_pack()
    if mod.kind == "linear":
        K = x.shape[-1]
        _, xq = ops.mx_quant_pack(x.reshape(-1, K).contiguous(), ACT_FMT, want_xq=True)
        y = ops.conv2d_fwd_pack(xq.reshape(1, 1, -1, K), pack, 1, 0, epilogue=L.EPI_NONE)
        return y.reshape(*x.shape[:-1], pack.w.shape[0])
    B, C, H, W = x.shape
    _, xq = ops.mx_quant_pack(x.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), ACT_FMT, want_xq=True)
    xq = xq.reshape(B, H, W, C)
    if mod.kind == "conv":
        stride, pad = mod.conv_geometry()
        y = ops.conv2d_fwd_pack(xq, pack, stride, pad, epilogue=L.EPI_NONE)
    else:
        kw = mod.fwd_kwargs
        y = ops.conv_transpose2d(xq, None, None, kw["stride"][0], kw["padding"][0], kw["output_padding"][0], epilogue=L.EPI_NONE, pack=pack)
    return y.permute(0, 3, 1, 2)


@pytest.mark.parametrize("mode", ["native", "emulated"])
def test_switched_modules_run_their_tail_on_the_mx_pre_activation(mode):
    from quantization import mx
    qnn, x = _model(), _image()
    rep = qnn.set_mx_activations(ACT_FMT, mode=mode)
    assert tuple(rep["native"]) == SWITCHED and tuple(rep["left"]) == ("stem",)
    out, seen = _run(qnn, x, capture=SWITCHED)
    assert tuple(out[0].shape) == (2, 16, 16, 16) and tuple(out[1].shape) == (2, 32)
    native = {"linear": mx.native_linear, "conv": mx.native_conv, "tconv": mx.native_tconv}
    for name in SWITCHED:
        mod = getattr(qnn.model, name)
        xin, got = seen[name]
        with torch.no_grad():
            pre = native[mod.kind](mod, xin, ACT_FMT) if mode == "native" else _emulation(mod, xin)
            want = _tail(mod, pre)
        assert _bits(got, want), (mode, name, float((got - want).abs().max()))
    # the conv carries a LeakyReLU: the tail is applied, un-fused
    assert float(seen["conv"][1].min()) < 0 and type(qnn.model.conv.activation_function).__name__ == "LeakyReLU"
    assert _bits(out[0], seen["head"][1]) and _bits(out[1], seen["fc"][1])


def test_left_cleared_and_unquantised_modules_give_the_bits_of_an_untouched_model():
    x = _image()
    plain = _model()
    want, seen0 = _run(plain, x, capture=("stem",) + SWITCHED)
    qnn = _model()
    qnn.set_mx_activations(ACT_FMT)
    got, seen = _run(qnn, x, capture=("stem",) + SWITCHED)
    assert _bits(seen["stem"][1], seen0["stem"][1])                                     # the stem is left: its forward is its own
    assert not _bits(got[0], want[0]) and not _bits(got[1], want[1])                    # the switched modules are not
    # weight quantisation off (an FP pass): the forward is what it is without the attribute
    plain.set_quant_state(False, False)
    qnn.set_quant_state(False, False)
    fp_want, _ = _run(plain, x)
    fp_got, _ = _run(qnn, x)
    assert _bits(fp_got[0], fp_want[0]) and _bits(fp_got[1], fp_want[1])
    qnn.set_quant_state(True, False)
    # one unit cleared: it runs its own forward on the input it is given
    qnn.set_mx_activations(None, units=["head"])
    _, part = _run(qnn, x, capture=("head",))
    with torch.no_grad():
        own = plain.model.head
        own.set_quant_state(True, False)
        assert _bits(part["head"][1], own(part["head"][0]))
    # all cleared: the untouched model's bits
    qnn.set_mx_activations(None)
    back, _ = _run(qnn, x)
    assert _bits(back[0], want[0]) and _bits(back[1], want[1])


def test_native_and_emulated_differ_less_than_the_activation_grid_changes():
    """rel_l2(native, emulated) against rel_l2(native, no MX activations) over the concatenated outputs: arithmetic order must matter
    less than the activation grid.  Measured: 0 (equal bits) against 7.304e-03 (mxfp4 weights, mxfp8_e4m3 activations)."""
    x = _image()
    qnn = _model()
    base, _ = _run(qnn, x)
    qnn.set_mx_activations(ACT_FMT, mode="native")
    nat, _ = _run(qnn, x)
    qnn.set_mx_activations(ACT_FMT, mode="emulated")
    emu, _ = _run(qnn, x)
    flat = lambda o: torch.cat([t.reshape(-1) for t in o]).double().cpu().numpy()
    n, e, b = flat(nat), flat(emu), flat(base)
    order = np.linalg.norm(n - e) / np.linalg.norm(e)
    grid = np.linalg.norm(n - b) / np.linalg.norm(b)
    print(f"set_mx_activations({ACT_FMT}) on {W_FMT} weights: rel_l2(native, emulated) = {order:.3e}, rel_l2(native, no MX activations) = {grid:.3e}")
    assert np.isfinite(n).all() and np.isfinite(e).all() and grid > 0
    assert order < grid


def test_an_input_that_requires_grad_is_refused():
    qnn, x = _model(), _image()
    qnn.set_mx_activations(ACT_FMT)
    h = torch.randn(2, 32, 8, 8, device="cuda", requires_grad=True)
    for name in ("conv", "up"):
        with pytest.raises(NotImplementedError, match=f"QuantModule\\({getattr(qnn.model, name).kind}, .*no backward is built under MX activations"):
            getattr(qnn.model, name)(h)
        with pytest.raises(NotImplementedError, match="no backward is built under MX activations"):
            getattr(qnn.model, name)._forward_autograd(h)
    with pytest.raises(NotImplementedError, match="no backward is built under MX activations"):
        qnn.model.fc(torch.randn(2, 32, device="cuda", requires_grad=True))
    # the stem was left: it still differentiates
    y = qnn.model.stem(x.clone().requires_grad_(True))
    assert y.requires_grad
    # under no_grad the same input is served
    with torch.no_grad():
        assert tuple(qnn.model.up(h).shape) == (2, 32, 16, 16)
