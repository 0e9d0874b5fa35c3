"""Weight quantisers on the OCP microscaling (MX) block formats (include/rdo_ptq_mx.h): blocks of 32 elements along the GEMM's K
dimension, one shared power-of-two scale per block, FP4 / FP6 / FP8 elements.  `MXQuantizer` rounds to nearest (`ops.mx_fakequant`);
`MXAdaRoundQuantizer` carries learned rounding on the same grids (include/rdo_ptq_mxround.h; `QuantModel.set_weight_format(...,
rounding='learned')`, then `reconstruct`).

The codes on the matrix cores (include/rdo_ptq_mxgemm.h): `native_operand(module)` is a module's weight as a packed operand of the
block-scaled matrix instruction, `native_linear(module, x, act_fmt)` the module's pre-activation output with the input quantised to an MX
format as well -- for token-matrix Linears and 1x1 stride-1 convs whose input channels are a multiple of 32;
`QuantModel.mx_native_report` measures it against the emulation, layer by layer.  The quantisers themselves serve weights only: an
activation is put on an MX grid by `native_linear` (`ops.mx_quant_pack`), not by a quantiser call with act=True.

k x k convolutions (include/rdo_ptq_mxconv.h): `native_conv_operand(module)` is a conv's weight [Cout, k * k * Cin] as a packed operand,
rows in `to_rows`' (kh, kw, in) order, `native_conv(module, x, act_fmt)` its pre-activation output from the NHWC pixels of x quantised
to an MX format -- an implicit GEMM, bit for bit `ops.mx_gemm` on the im2col matrix -- for square kernels with one stride and one zero
padding, dilation 1, groups 1 and input channels a multiple of 32 (`native_conv_refusal`); `mx_native_report(..., convs=True)` measures
them too.

Transposed convs (include/rdo_ptq_mxtconv.h): `native_tconv_operand(module)` is a transposed conv's weight [Cout, k * k * Cin] along
`to_rows(W, tconv=True)` as a packed operand, `native_tconv(module, x, act_fmt)` its pre-activation output -- phase by phase bit for bit
`ops.mx_gemm` on the gathered operands -- for square kernels with one stride, one padding and one output padding, dilation 1, groups 1
and input channels (`weight.shape[0]`) a multiple of 32 (`native_tconv_refusal`); `mx_native_report(..., tconvs=True)` measures them.

MX activations inside the modules' own forward: `QuantModel.set_mx_activations(act_fmt, mode)` sets `mx_activations = (act_fmt, mode)` on
every module one of the three refusals accepts; `QuantModule.forward` (no-grad path, weight quantisation on) then takes its
pre-activation output from `mx_forward`: mode 'native' runs `native_linear` / `native_conv` / `native_tconv`, mode 'emulated' the
module's fp32 kernel on the decoded `xq` of the same producer; the module's tail (se_module, activation function, output quantiser)
follows un-fused.  Not built: GDN and LayerNorm on the native path, fused activation epilogues, a producer fused into the previous
layer's store, calibration or a backward under MX activations (`reconstruct` refuses such a model), data-parallel runs; no
rate-distortion claim is made for any of it.  A model on these quantisers is stored by `mx_packed.save_mx_packed`, the `mx_activations`
pairs included."""
import torch
import torch.nn as nn

from hipops import _lib as L
from hipops import ops

from .quantizer import from_rows, to_rows

MX_FORMATS = tuple(L.MX_FORMATS)
MX_ROUNDINGS = ("nearest", "learned")


def is_mx(q):
    return isinstance(q, MXQuantizer)


def is_mx_learned(q):
    return isinstance(q, MXAdaRoundQuantizer)


def is_mx_any(q):
    """either MX class: what `set_weight_format` swaps back and what has no integer grid to export or pack"""
    return isinstance(q, (MXQuantizer, MXAdaRoundQuantizer))


def refuse_mx(what, named_modules, error, why, learned=True):
    """raise `error` naming the first module of (name, module) pairs whose weight quantiser is an `MXQuantizer` -- or, with `learned`, an
    `MXAdaRoundQuantizer`"""
    for name, m in named_modules:
        q = getattr(m, "weight_quantizer", None)
        if is_mx(q) or (learned and is_mx_learned(q)):
            raise error(f"{what}: module {name!r} holds an {type(q).__name__} ({q.fmt}): {why}")


class _MXFields(nn.Module):
    """What both MX quantisers carry: what `QuantModule._weight_state` reads of a weight quantiser (inited = True, n_bits = the element
    bits, n_levels = 2 ** n_bits, delta = zero_point = None), `fmt`, `tconv`, and `size_bits(weight)` = element bits x elements + 8 x
    blocks.  `QuantModel.weight_bits()` reads n_bits and so counts the element bits only, not the scales."""

    def __init__(self, fmt: str, tconv: bool = False):
        super().__init__()
        _, bits = ops.mx_format(type(self).__name__, fmt)
        self.fmt, self.tconv = fmt, bool(tconv)
        self.n_bits, self.n_levels = bits, 2 ** bits
        self.delta = self.zero_point = None
        self.inited = True

    def _rows(self, x):
        wr = to_rows(x, self.tconv)
        return wr.reshape(wr.shape[0], -1)

    def _refuse_act(self, act):
        if act:
            raise NotImplementedError(f"{type(self).__name__}({self.fmt}): MX activations are not built into the quantisers, which serve weights only; "
                                      "`quantization.mx.native_linear` quantises a Linear's or 1x1 conv's input to an MX format")

    def _nearest(self, x):
        wr = to_rows(x.detach(), self.tconv)
        wq = ops.mx_fakequant(wr.reshape(wr.shape[0], -1), self.fmt)["wq"].reshape(wr.shape)
        return from_rows(wq, x, self.tconv)

    def weight_cost(self, x):
        """(err, energy) float64 [rows] of `x` in this format at round to nearest, on the device: sum (w - wq)^2 and sum w^2 per row of
        `to_rows`"""
        out = ops.mx_fakequant(self._rows(x.detach()), self.fmt, want=("err", "energy"))
        return out["err"], out["energy"]

    def size_bits(self, weight):
        """element bits x elements + 8 x blocks, the blocks counted along the rows of `to_rows(weight)`"""
        rows = 1 if weight.dim() == 1 else int(weight.shape[1] if (self.tconv and weight.dim() == 4) else weight.shape[0])
        inner = int(weight.numel()) // rows
        return self.n_bits * rows * inner + 8 * rows * -(-inner // L.MX_BLOCK)

    def extra_repr(self):
        return f"fmt={self.fmt}, bit={self.n_bits}, tconv={self.tconv}"


class MXQuantizer(_MXFields):
    """Fake-quantises a weight to the MX format `fmt` (a name of `hipops._lib.MX_FORMATS`).  Called on a weight it returns the quantised
    weight in the weight's own shape.  The blocks run along the rows of `to_rows(weight, tconv)` -- conv: one row per output channel in
    (kh, kw, in) order; transposed conv: tconv=True; Linear: as stored; a 1-D weight is one row -- whatever `channel_wise` was on the
    quantiser it replaces: the block structure follows K.  There is no state to initialise: every call derives the scales from the weight.

    It carries what `QuantModule._weight_state` reads of a weight quantiser (inited = True, n_bits = the element bits, n_levels = 2 **
    n_bits, delta = zero_point = None), `fmt`, and `size_bits(weight)` = element bits x elements + 8 x blocks.  `QuantModel.weight_bits()`
    reads n_bits and so counts the element bits only, not the scales.

    Weights only: a call with act=True raises NotImplementedError (MX activations are not built into the quantisers; `native_linear` is the
    path that quantises an input)."""

    def forward(self, x: torch.Tensor, act: bool = False, **kw):
        self._refuse_act(act)
        return self._nearest(x)


class MXAdaRoundQuantizer(_MXFields):
    """A weight on the MX format `fmt` with learned rounding (include/rdo_ptq_mxround.h).  Not an `MXQuantizer`: `is_mx` and the refusals
    that go with it do not see it.  Before calibration `alpha` is None and a call rounds to nearest -- the bits `MXQuantizer` gives.
    `UnitEngine.finish` stores `alpha` (fp32, the layout of `to_rows(weight, tconv)`) and `soft_targets = False`; a call then returns the
    hard weight lo + gap * (alpha >= 0) on the grid of the weight it is given (`ops.mx_neighbours`, `ops.mx_round_fwd`): the block scales
    are those of round to nearest, a pinned element stays at +-max X.  `codes_and_scales(weight)` is the stored form: uint8 element codes
    and E8M0 scale bytes with `ops.mx_dequant(codes, scales, inner, fmt)` the forwarded rows bit for bit.

    Weights only: a call with act=True raises NotImplementedError (MX activations are not built into the quantisers; `native_linear` is the
    path that quantises an input)."""

    def __init__(self, fmt: str, tconv: bool = False):
        super().__init__(fmt, tconv)
        self.register_buffer("alpha", None)
        self.soft_targets = False

    def _hard(self, rows2d, codes):
        lo, gap, scales = ops.mx_neighbours(rows2d, self.fmt, want_scales=True)
        alpha = self.alpha.reshape(rows2d.shape)
        if alpha.device != rows2d.device:
            alpha = alpha.to(rows2d.device)
        d = ops.ada_desc(rows2d, conv_layout=False)
        return ops.mx_round_fwd(d, lo, gap, alpha.contiguous(), False, self.fmt, codes=codes, scales=scales if codes else None), scales

    def forward(self, x: torch.Tensor, act: bool = False, **kw):
        self._refuse_act(act)
        if self.alpha is None:
            return self._nearest(x)
        wr = to_rows(x.detach(), self.tconv)
        wq, _ = self._hard(wr.reshape(wr.shape[0], -1), False)
        return from_rows(wq.reshape(wr.shape), x, self.tconv)

    def codes_and_scales(self, weight):
        """(codes uint8 [rows, inner], scales uint8 [rows, ceil(inner / 32)]) of `weight` as this quantiser forwards it"""
        rows2d = self._rows(weight.detach())
        if self.alpha is None:
            out = ops.mx_fakequant(rows2d, self.fmt, want=("codes", "scales"))
            return out["codes"], out["scales"]
        (_, codes), scales = self._hard(rows2d, True)
        return codes, scales

    def extra_repr(self):
        return super().extra_repr() + f", rounding={'nearest' if self.alpha is None else 'learned'}"


# ---- the codes on the block-scaled matrix instruction (include/rdo_ptq_mxgemm.h) --------------------------------------------------------------
def native_refusal(module):
    """None for a QuantModule `native_operand` serves, else the reason it does not: its weight quantiser is no MX class, or it is neither
    a Linear nor a 1x1 stride-1 unpadded conv (dilation 1, groups 1), or its input channels are no multiple of 32"""
    q = getattr(module, "weight_quantizer", None)
    kind = getattr(module, "kind", None)
    if kind not in ("linear", "conv"):
        return f"a {kind} module is not GEMM-shaped: the native path serves Linears and 1x1 stride-1 convs"
    w = module.weight
    if kind == "conv":
        kw = module.fwd_kwargs
        one = lambda v, want: all(int(a) == want for a in ((v, v) if isinstance(v, int) else tuple(v)))
        if tuple(w.shape[2:]) != (1, 1) or not one(kw["stride"], 1) or not one(kw["padding"], 0) or not one(kw["dilation"], 1) or kw["groups"] != 1:
            return (f"a conv with kernel {tuple(w.shape[2:])}, stride {kw['stride']}, padding {kw['padding']}, dilation {kw['dilation']}, groups "
                    f"{kw['groups']} is not a 1x1 stride-1 unpadded conv")
    K = int(w.shape[1])
    if K % L.MX_BLOCK:
        return f"its {K} input channels are no multiple of the MX block size {L.MX_BLOCK}"
    if not is_mx_any(q):
        return f"its weight quantiser is a {type(q).__name__}, not an MXQuantizer or MXAdaRoundQuantizer"
    return None


def native_operand(module):
    """The `ops.MXOperand` [out, in] of a QuantModule's weight as its MX quantiser forwards it: `mx_fakequant` codes and scales from an
    `MXQuantizer`, `codes_and_scales(weight)` from an `MXAdaRoundQuantizer` (learned rounding included), both along `to_rows`, packed by
    `ops.mx_pack_codes`.  Memoised next to `weight_pack()` (same weight, quantiser and alpha: same operand) and dropped by
    `drop_weight_pack()`.  ValueError naming the module and the reason for a module `native_refusal` gives a reason for."""
    why = native_refusal(module)
    if why is not None:
        raise ValueError(f"native_operand: module {_describe(module)}: {why}")
    return _weight_operand(module, "mx_native")


def _weight_operand(module, slot):
    """the packed operand of a module's weight along `to_rows`, memoised in `_pack_memo[slot]`"""
    q, w = module.weight_quantizer, module.weight
    alpha = getattr(q, "alpha", None)
    key = (slot, id(q), q.fmt, module._tkey(w), module._tkey(alpha))
    memos = module.__dict__.get("_pack_memo")
    if not isinstance(memos, dict):
        memos = module.__dict__["_pack_memo"] = {}
    memo = memos.get(slot)
    if memo is not None and memo[0] == key and memo[2][0] is w and memo[2][1] is alpha:
        return memo[1]
    if is_mx_learned(q):
        codes, scales = q.codes_and_scales(w)
    else:
        out = ops.mx_fakequant(q._rows(w.detach()), q.fmt, want=("codes", "scales"))
        codes, scales = out["codes"], out["scales"]
    op = ops.mx_pack_codes(codes, scales, q.fmt)
    memos[slot] = (key, op, (w, alpha))
    return op


def _describe(module):
    return f"{type(module).__name__}({getattr(module, 'kind', '?')}, weight {tuple(module.weight.shape) if getattr(module, 'weight', None) is not None else None})"


def native_rows(module, x):
    """the activation operand of an eligible module's input as contiguous fp32 [rows, K] -- a Linear's [..., K] flattened, the
    channels-last view of a 1x1 conv's NCHW input: one row per token or pixel -- and the shape of the module's output"""
    K = int(module.weight.shape[1])
    N = int(module.weight.shape[0])
    if module.kind == "linear":
        if x.dim() < 1 or x.shape[-1] != K:
            raise ValueError(f"native_linear: the input must be [..., {K}], got {tuple(x.shape)}")
        return x.reshape(-1, K).contiguous(), lambda y: y.reshape(*x.shape[:-1], N)
    if x.dim() != 4 or x.shape[1] != K:
        raise ValueError(f"native_linear: the input must be [B, {K}, H, W], got {tuple(x.shape)}")
    B, _, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(-1, K).contiguous(), lambda y: y.reshape(B, H, W, N).permute(0, 3, 1, 2)


def native_bias(module):
    """the bias the module's forward uses in its present quant state (None for a module without one)"""
    b = module.bias if module.use_weight_quant else module.org_bias
    return None if b is None else b.detach().contiguous()


def native_linear(module, x, act_fmt):
    """The pre-activation output of an eligible QuantModule (`native_operand`) on the block-scaled matrix instruction: `x` is the
    module's input ([..., K] for a Linear, NCHW for a 1x1 conv), the result has the module's output shape ([..., N]; a channels-last
    view [B, N, H, W]).  The rows of the channels-last view of x are quantised to the MX format `act_fmt` in blocks of 32 along the input
    channels -- the K of the product, along which `to_rows` lays the weight's blocks -- by one `ops.mx_quant_pack` launch; one
    `ops.mx_gemm` launch multiplies them with the weight's codes and adds the bias of the module's present quant state.  Nothing else of
    the module's forward is applied: no activation function or fused epilogue, no `se_module`, no output quantiser."""
    b = native_operand(module)
    rows, shape = native_rows(module, x)
    a = ops.mx_quant_pack(rows, act_fmt)
    return shape(ops.mx_gemm(a, b, native_bias(module)))


# ---- k x k convolutions on the same instruction (include/rdo_ptq_mxconv.h) --------------------------------------------------------------------
def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(a) for a in v)


def conv_geometry(module):
    """(k, stride, pad) of a conv QuantModule `native_conv_refusal` accepts"""
    kw = module.fwd_kwargs
    return int(module.weight.shape[2]), _pair(kw["stride"])[0], _pair(kw["padding"])[0]


def native_conv_refusal(module):
    """None for a QuantModule `native_conv_operand` serves, else the reason it does not, looked for in this order: it is no conv; its
    kernel, stride (>= 1) or padding (>= 0) is not square, or it is dilated or grouped; its input channels are no multiple of 32; its
    weight quantiser is no MX class"""
    q = getattr(module, "weight_quantizer", None)
    kind = getattr(module, "kind", None)
    if kind != "conv":
        return f"a {kind} module is not a convolution: the native conv path serves square k x k convs"
    w, kw = module.weight, module.fwd_kwargs
    (kh, kwid), (sh, sw), (dh, dw), pad = tuple(int(a) for a in w.shape[2:]), _pair(kw["stride"]), _pair(kw["dilation"]), kw["padding"]
    square_pad = not isinstance(pad, str) and _pair(pad)[0] == _pair(pad)[1] and _pair(pad)[0] >= 0
    if kh != kwid or sh != sw or sh < 1 or not square_pad or (dh, dw) != (1, 1) or kw["groups"] != 1:
        return (f"a conv with kernel {(kh, kwid)}, stride {kw['stride']}, padding {kw['padding']}, dilation {kw['dilation']}, groups "
                f"{kw['groups']} is not a square-kernel conv with one stride, one zero padding, dilation 1 and groups 1")
    K = int(w.shape[1])
    if K % L.MX_BLOCK:
        return f"its {K} input channels are no multiple of the MX block size {L.MX_BLOCK}"
    if not is_mx_any(q):
        return f"its weight quantiser is a {type(q).__name__}, not an MXQuantizer or MXAdaRoundQuantizer"
    return None


def native_conv_operand(module):
    """The `ops.MXOperand` [Cout, k * k * Cin] of a conv QuantModule's weight as its MX quantiser forwards it, made along `to_rows` (rows
    in (kh, kw, in) order) exactly as `native_operand` makes it, learned rounding included.  Memoised under a key of its own next to
    `weight_pack()` and dropped by `drop_weight_pack()`; for a 1x1 stride-1 unpadded conv it is the object `native_operand` returns.
    ValueError naming the module and the reason for a module `native_conv_refusal` gives a reason for."""
    why = native_conv_refusal(module)
    if why is not None:
        raise ValueError(f"native_conv_operand: module {_describe(module)}: {why}")
    if native_refusal(module) is None:
        return native_operand(module)
    return _weight_operand(module, "mx_native_conv")


def native_conv(module, x, act_fmt):
    """The pre-activation output of an eligible conv QuantModule (`native_conv_operand`) on the block-scaled matrix instruction: `x` is
    the module's NCHW input, the result a channels-last view [B, N, Ho, Wo].  The rows of the channels-last view of x -- one per pixel --
    are quantised to the MX format `act_fmt` in blocks of 32 along the input channels by one `ops.mx_quant_pack` launch; one
    `ops.mx_conv2d` launch convolves them with the weight's codes at the module's stride and padding and adds the bias of the module's
    present quant state.  Nothing else of the module's forward is applied: no activation function or fused epilogue, no `se_module`, no
    output quantiser."""
    b = native_conv_operand(module)
    C = int(module.weight.shape[1])
    if x.dim() != 4 or x.shape[1] != C:
        raise ValueError(f"native_conv: the input must be [B, {C}, H, W], got {tuple(x.shape)}")
    B, _, H, W = (int(v) for v in x.shape)
    k, stride, pad = conv_geometry(module)
    a = ops.mx_quant_pack(x.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), act_fmt)
    return ops.mx_conv2d(a, b, (B, H, W), k, stride, pad, native_bias(module)).permute(0, 3, 1, 2)


# ---- transposed convolutions on the same instruction (include/rdo_ptq_mxtconv.h) ---------------------------------------------------------------
def tconv_geometry(module):
    """(k, stride, pad, output_padding) of a transposed-conv QuantModule `native_tconv_refusal` accepts"""
    kw = module.fwd_kwargs
    return int(module.weight.shape[2]), _pair(kw["stride"])[0], _pair(kw["padding"])[0], _pair(kw["output_padding"])[0]


def native_tconv_refusal(module):
    """None for a QuantModule `native_tconv_operand` serves, else the reason it does not, looked for in this order: it is no transposed
    conv; its kernel, stride (>= 1), padding (>= 0) or output padding is not square, or it is dilated or grouped; its input channels
    (`weight.shape[0]`) are no multiple of 32; its weight quantiser is no MX class, or one made with tconv=False"""
    q = getattr(module, "weight_quantizer", None)
    kind = getattr(module, "kind", None)
    if kind != "tconv":
        return f"a {kind} module is not a transposed convolution: the native tconv path serves square k x k transposed convs"
    w, kw = module.weight, module.fwd_kwargs
    (kh, kwid), (sh, sw), (dh, dw) = tuple(int(a) for a in w.shape[2:]), _pair(kw["stride"]), _pair(kw["dilation"])
    (ph, pw), (oh, ow) = _pair(kw["padding"]), _pair(kw["output_padding"])
    if kh != kwid or sh != sw or sh < 1 or ph != pw or ph < 0 or oh != ow or (dh, dw) != (1, 1) or kw["groups"] != 1:
        return (f"a transposed conv with kernel {(kh, kwid)}, stride {kw['stride']}, padding {kw['padding']}, output padding "
                f"{kw['output_padding']}, dilation {kw['dilation']}, groups {kw['groups']} is not a square-kernel transposed conv with one "
                "stride, one padding, one output padding, dilation 1 and groups 1")
    K = int(w.shape[0])
    if K % L.MX_BLOCK:
        return f"its {K} input channels are no multiple of the MX block size {L.MX_BLOCK}"
    if not is_mx_any(q):
        return f"its weight quantiser is a {type(q).__name__}, not an MXQuantizer or MXAdaRoundQuantizer"
    if not q.tconv:
        return f"its {type(q).__name__} was made with tconv=False: its blocks do not run along the rows of to_rows(W, tconv=True)"
    return None


def native_tconv_operand(module):
    """The `ops.MXOperand` [Cout, k * k * Cin] of a transposed-conv QuantModule's weight as its MX quantiser forwards it, made along
    `to_rows(W, tconv=True)` (row n, tap (kh, kw), channel c holds W[c, n, kh, kw]; taps un-flipped) exactly as `native_operand` makes
    it, learned rounding included.  Memoised under a key of its own next to `weight_pack()` and dropped by `drop_weight_pack()`.
    ValueError naming the module and the reason for a module `native_tconv_refusal` gives a reason for."""
    why = native_tconv_refusal(module)
    if why is not None:
        raise ValueError(f"native_tconv_operand: module {_describe(module)}: {why}")
    return _weight_operand(module, "mx_native_tconv")


def native_tconv(module, x, act_fmt):
    """The pre-activation output of an eligible transposed-conv QuantModule (`native_tconv_operand`) on the block-scaled matrix
    instruction: `x` is the module's NCHW input, the result a channels-last view [B, N, Ho, Wo].  The rows of the channels-last view of
    x -- one per pixel -- are quantised to the MX format `act_fmt` in blocks of 32 along the input channels by one `ops.mx_quant_pack`
    launch; one `ops.mx_conv_transpose2d` launch applies the weight's codes at the module's stride, padding and output padding and adds
    the bias of the module's present quant state.  Nothing else of the module's forward is applied."""
    why = native_tconv_refusal(module)
    if why is not None:
        raise ValueError(f"native_tconv_operand: module {_describe(module)}: {why}")
    C = int(module.weight.shape[0])
    if x.dim() != 4 or x.shape[1] != C:
        raise ValueError(f"native_tconv: the input must be [B, {C}, H, W], got {tuple(x.shape)}")
    b = native_tconv_operand(module)
    B, _, H, W = (int(v) for v in x.shape)
    k, stride, pad, opad = tconv_geometry(module)
    a = ops.mx_quant_pack(x.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), act_fmt)
    return ops.mx_conv_transpose2d(a, b, (B, H, W), k, stride, pad, opad, native_bias(module)).permute(0, 3, 1, 2)


# ---- MX activations inside the modules' own forward (QuantModel.set_mx_activations) ------------------------------------------------------------
MX_ACT_MODES = ("native", "emulated")


def native_kind(module):
    """('linear' | 'conv' | 'tconv', None) for a module one of the three refusals accepts -- a 1x1 stride-1 conv counts as 'conv' --,
    else (None, the reason of the refusal that speaks for the module's kind)"""
    kind = getattr(module, "kind", None)
    if kind == "tconv":
        why = native_tconv_refusal(module)
    elif kind == "conv":
        why = native_conv_refusal(module)
    else:
        why = native_refusal(module)
    return (kind, None) if why is None else (None, why)


def refuse_mx_activations(what, named_modules, why):
    """NotImplementedError naming the first module of (name, module) pairs that carries `mx_activations`"""
    for name, m in named_modules:
        on = getattr(m, "mx_activations", None)
        if on is not None:
            raise NotImplementedError(f"{what}: module {name!r} runs on MX activations ({on[0]}, {on[1]}): {why}")


def mx_forward(module, x):
    """The pre-activation output of a module whose `mx_activations` = (act_fmt, mode) is set (`QuantModel.set_mx_activations`), from its
    input quantised to act_fmt in blocks of 32 along the input channels.  'native': `native_linear`, `native_conv` or `native_tconv`.
    'emulated': xq of `ops.mx_quant_pack(rows, act_fmt, want_xq=True)`, reshaped to the input, through the module's fp32 forward kernel
    with its quantised weight pack and EPI_NONE."""
    act_fmt, mode = module.mx_activations
    kind = module.kind
    if mode == "native":
        if kind == "linear":
            return native_linear(module, x, act_fmt)
        return (native_conv if kind == "conv" else native_tconv)(module, x, act_fmt)
    pack = module.weight_pack()
    if kind == "linear":
        rows, shape = native_rows(module, x)
        _, xq = ops.mx_quant_pack(rows, act_fmt, want_xq=True)
        return shape(ops.conv2d_fwd_pack(xq.reshape(1, 1, -1, rows.shape[1]), pack, 1, 0, epilogue=L.EPI_NONE))
    C = int(module.weight.shape[0 if kind == "tconv" else 1])
    if x.dim() != 4 or x.shape[1] != C:
        raise ValueError(f"mx_forward: the input must be [B, {C}, H, W], got {tuple(x.shape)}")
    B, _, H, W = (int(v) for v in x.shape)
    _, xq = ops.mx_quant_pack(x.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), act_fmt, want_xq=True)
    xq = xq.reshape(B, H, W, C)
    if kind == "conv":
        _, stride, pad = conv_geometry(module)
        y = ops.conv2d_fwd_pack(xq, pack, stride, pad, epilogue=L.EPI_NONE)
    else:
        _, stride, pad, opad = tconv_geometry(module)
        y = ops.conv_transpose2d(xq, None, None, stride, pad, opad, epilogue=L.EPI_NONE, pack=pack)
    return y.permute(0, 3, 1, 2)
