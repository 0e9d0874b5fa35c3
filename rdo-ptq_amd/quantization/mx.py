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
follows un-fused.  GDN / IGDN (include/rdo_ptq_mxgdn.h): `native_gdn(module, x, act_fmt)` squares, quantises, runs the norm pool on the
instruction and forms x * norm^-+1/2 in one launch, with gamma' re-quantised onto the MX grid (`native_gdn_operand`: a second
rounding); `set_mx_activations(..., gdn=True)` switches eligible GDNs to it, `native_gdn_chain` hands its packed output to a following
conv.  Swin blocks (include/rdo_ptq_mxswin.h): `native_ln_linear(norm, linear, x, act_fmt)` runs norm1 -> qkv in two launches,
`native_swin_mlp(block, x, a, act_fmt)` the half x + a + fc2(gelu(fc1(norm2(x + a)))) in one; `set_mx_activations(..., swin=True)` switches
the blocks `native_swin_refusal` accepts (`mx_swin`, not stored by `save_mx_packed`).  The attention core (include/rdo_ptq_mxattn.h):
`native_attention(attn, qkv, ...)` runs Q K^T, the softmax and P V in one launch with Q, K, P and V on MX grids;
`set_mx_activations(..., attention=True)` switches the attentions `native_attention_refusal` accepts (`mx_attention`, not stored).  The
attention half (include/rdo_ptq_mxswinattn.h): `native_swin_attn(block, x, H, W, act_fmt)` runs norm1, qkv, the attention, proj and the
residual add in one launch; `set_mx_activations(..., swin=True, attention=True, fused_attention=True)` switches the blocks
`native_swin_attn_refusal` accepts (`mx_swin_attn`, not stored): a switched block is two launches.  Not built: calibration or a backward under MX
activations (`reconstruct` refuses such a model), data-parallel runs; no rate-distortion claim is made for any of it.  A model on these quantisers is stored by
`mx_packed.save_mx_packed`, the `mx_activations` pairs included.

Chains (include/rdo_ptq_mxchain.h): `native_chain(first, second, x, act_fmt, act)` runs two convs of the kinds above in three launches
-- `first` writes act(its output) packed in `act_fmt`, the operand `second` reads -- for pairs `native_chain_refusal` accepts;
`set_mx_activations(..., chain=True)` switches the conv1 -> LReLU -> conv2 pair of `QuantRB` / `QuantRBWS` blocks to it (`mx_chain`, not
stored by `save_mx_packed`).  The same bits as the un-chained forward.

The residual unit of the Cheng2020 attention block (include/rdo_ptq_mxresunit.h): `native_residual_unit(unit, x, act_fmt)` runs 1x1,
ReLU, 3x3, ReLU, 1x1, the identity add and the last ReLU of a `lic.layers._ResidualUnit` in one launch for units
`native_residual_unit_refusal` accepts; `set_mx_activations(..., residual_units=True)` switches them (`mx_resunit`, not stored).  The same
bits as the three modules' forwards with the eager add and ReLU."""
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


# ---- two convs chained through a packed MX tensor (include/rdo_ptq_mxchain.h) ---------------------------------------------------------------
def _chain_channels(module):
    """(input channels, output channels) of a conv or transposed-conv QuantModule"""
    w = module.weight
    return (int(w.shape[0]), int(w.shape[1])) if module.kind == "tconv" else (int(w.shape[1]), int(w.shape[0]))


def native_chain_refusal(first, second):
    """None for a pair of QuantModules `native_chain` serves, else the reason it does not, looked for in this order: `first`, then
    `second`, is no module `native_conv_refusal` / `native_tconv_refusal` accepts; `first` has an `se_module`, an activation function of
    its own that is not the identity, or an active output quantiser (the chain applies bias and `act` alone between the two convs);
    its output channels are no multiple of 32 (they are the blocks of `second`'s K); they are not `second`'s input channels"""
    from .quantizer import StraightThrough
    for name, m in (("first", first), ("second", second)):
        why = (native_tconv_refusal if getattr(m, "kind", None) == "tconv" else native_conv_refusal)(m)
        if why is not None:
            return f"{name}: {why}"
    if first.se_module is not None:
        return "first has an se_module between its convolution and its output"
    if not isinstance(first.activation_function, (StraightThrough, nn.Identity)):
        return f"first has an activation function of its own ({type(first.activation_function).__name__}), not the identity"
    if not first.disable_act_quant and first.use_act_quant and first.trained:
        return "first has an active output quantiser"
    n, c = _chain_channels(first)[1], _chain_channels(second)[0]
    if n % L.MX_BLOCK:
        return f"first's {n} output channels are no multiple of the MX block size {L.MX_BLOCK}"
    if n != c:
        return f"first's {n} output channels are not second's {c} input channels"
    return None


def _chain_step(module, a, shape, **out):
    """one conv or transposed conv of a chain on the packed NHWC pixels `a` of a (B, H, W) input -> (result, (B, Ho, Wo))"""
    B, H, W = shape
    if module.kind == "tconv":
        k, stride, pad, opad = tconv_geometry(module)
        y = ops.mx_conv_transpose2d(a, native_tconv_operand(module), shape, k, stride, pad, opad, native_bias(module), **out)
        return y, (B, (H - 1) * stride - 2 * pad + k + opad, (W - 1) * stride - 2 * pad + k + opad)
    k, stride, pad = conv_geometry(module)
    y = ops.mx_conv2d(a, native_conv_operand(module), shape, k, stride, pad, native_bias(module), **out)
    return y, (B, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)


def native_chain(first, second, x, act_fmt, act="lrelu"):
    """The pre-activation output of `second` from the NCHW input `x` of `first` in three launches: `ops.mx_quant_pack` on the NHWC pixels
    of x, `first` with its bias and `act` ('none' | 'lrelu' | 'relu') writing its output packed in `act_fmt` (`out_fmt=` of
    `ops.mx_conv2d` / `mx_conv_transpose2d`), and `second` on that operand with its bias and the fp32 output, a channels-last view
    [B, N, Ho, Wo].  Bit for bit second's `native_conv` / `native_tconv` on act(first's): no fp32 tensor lies between the two convs.
    ValueError naming the modules and the reason for a pair `native_chain_refusal` gives a reason for."""
    why = native_chain_refusal(first, second)
    if why is not None:
        raise ValueError(f"native_chain: modules {_describe(first)} -> {_describe(second)}: {why}")
    C = _chain_channels(first)[0]
    if x.dim() != 4 or x.shape[1] != C:
        raise ValueError(f"native_chain: the input must be [B, {C}, H, W], got {tuple(x.shape)}")
    B, _, H, W = (int(v) for v in x.shape)
    a = ops.mx_quant_pack(x.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), act_fmt)
    mid, shape = _chain_step(first, a, (B, H, W), out_fmt=act_fmt, act=act)
    return _chain_step(second, mid, shape)[0].permute(0, 3, 1, 2)


# ---- GDN / IGDN with the norm pool on the same instruction (include/rdo_ptq_mxgdn.h) -----------------------------------------------------------
def native_gdn_refusal(module):
    """None for a QuantModule `native_gdn` serves, else the reason it does not, looked for in this order: it is no GDN / IGDN; its
    channels are no multiple of 32; they are above `hipops._lib.MXGDN_MAX_C`; its weight quantiser is no MX class"""
    q = getattr(module, "weight_quantizer", None)
    kind = getattr(module, "kind", None)
    if kind != "gdn":
        return f"a {kind} module is not a GDN: the native GDN path serves GDN and IGDN modules"
    C = int(module.weight.shape[0])
    if C % L.MX_BLOCK:
        return f"its {C} channels are no multiple of the MX block size {L.MX_BLOCK}"
    if C > L.MXGDN_MAX_C:
        return f"its {C} channels are above {L.MXGDN_MAX_C}, the most the kernel's LDS serves"
    if not is_mx_any(q):
        return f"its weight quantiser is a {type(q).__name__}, not an MXQuantizer or MXAdaRoundQuantizer"
    return None


def _gdn_operands(module):
    """(packed operand, decoded `ops.WeightPack`) of a GDN module's effective gamma' on the MX grid, memoised in
    `_pack_memo['mx_native_gdn']` for as long as `weight_pack()` returns the same pack"""
    why = native_gdn_refusal(module)
    if why is not None:
        raise ValueError(f"native_gdn_operand: module {_describe(module)}: {why}")
    pack, fmt = module.weight_pack(), module.weight_quantizer.fmt
    memos = module.__dict__.get("_pack_memo")
    if not isinstance(memos, dict):
        memos = module.__dict__["_pack_memo"] = {}
    memo = memos.get("mx_native_gdn")
    if memo is not None and memo[0] is pack and memo[1] == fmt:
        return memo[2]
    C = int(pack.w.shape[0])
    out = ops.mx_fakequant(pack.w.reshape(C, C), fmt, want=("wq", "codes", "scales"))
    both = (ops.mx_pack_codes(out["codes"], out["scales"], fmt), ops.WeightPack(out["wq"].reshape(C, 1, 1, C), pack.bias))
    memos["mx_native_gdn"] = (pack, fmt, both)
    return both


def native_gdn_operand(module):
    """The `ops.MXOperand` [C, C] of a GDN QuantModule's effective gamma' in its present quant state: `module.weight_pack().w` --
    reparam(weight_quantizer(gamma)) = max(., bound)^2 - pedestal of the quantised gamma -- put on the MX grid of the quantiser's format
    by `ops.mx_fakequant` (round to nearest), blocks along the input channel, and packed.  This is a SECOND rounding: the
    re-parametrisation takes the quantised gamma off its grid, and the instruction needs codes.  Rounding keeps signs and zeros, so
    gamma' >= 0 stays so, and beta' > 0 is not rounded: norm > 0.  Memoised in `_pack_memo` under a slot of its own and dropped by
    `drop_weight_pack()`.  ValueError naming the module and the reason for a module `native_gdn_refusal` gives a reason for."""
    return _gdn_operands(module)[0]


def _gdn_rows(what, module, x):
    C = int(module.weight.shape[0])
    if x.dim() != 4 or x.shape[1] != C:
        raise ValueError(f"{what}: the input must be [B, {C}, H, W], got {tuple(x.shape)}")
    B, _, H, W = (int(v) for v in x.shape)
    return x.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), (B, H, W)


def native_gdn(module, x, act_fmt, out_fmt=None):
    """The output of an eligible GDN / IGDN QuantModule (`native_gdn_operand`) in one `ops.mx_gdn` launch: `x` is the module's NCHW
    input; the squares of its NHWC pixels are quantised to `act_fmt` in blocks of 32 channels, the norm pool beta' + gamma' x^2 runs on
    the block-scaled matrix instruction with `module.weight_pack().bias` as beta', and y = x * norm^-1/2 (IGDN: x * norm^1/2) comes
    back as a channels-last view [B, C, H, W] -- or, with out_fmt, as the `ops.MXOperand` [B * H * W, C] of the NHWC pixels, the
    operand of a following conv.  Nothing else of the module's forward is applied."""
    g = native_gdn_operand(module)
    rows, (B, H, W) = _gdn_rows("native_gdn", module, x)
    y = ops.mx_gdn(rows, g, module.weight_pack().bias, act_fmt, inverse=bool(module.fwd_kwargs["inverse"]), out_fmt=out_fmt)
    return y if out_fmt is not None else y.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def native_gdn_chain_refusal(gdn, second):
    """None for a (GDN, conv or transposed conv) pair `native_gdn_chain` serves, else the reason it does not, looked for in this order:
    `gdn` is no module `native_gdn_refusal` accepts; `second` none `native_conv_refusal` / `native_tconv_refusal` accepts; `gdn` has an
    `se_module`, an activation function that is not the identity, or an active output quantiser; its channels are not `second`'s input
    channels"""
    from .quantizer import StraightThrough
    why = native_gdn_refusal(gdn)
    if why is not None:
        return f"gdn: {why}"
    why = (native_tconv_refusal if getattr(second, "kind", None) == "tconv" else native_conv_refusal)(second)
    if why is not None:
        return f"second: {why}"
    if gdn.se_module is not None:
        return "gdn has an se_module between its output and second"
    if not isinstance(gdn.activation_function, (StraightThrough, nn.Identity)):
        return f"gdn has an activation function of its own ({type(gdn.activation_function).__name__}), not the identity"
    if not gdn.disable_act_quant and gdn.use_act_quant and gdn.trained:
        return "gdn has an active output quantiser"
    n, c = int(gdn.weight.shape[0]), _chain_channels(second)[0]
    if n != c:
        return f"gdn's {n} channels are not second's {c} input channels"
    return None


def native_gdn_chain(gdn, second, x, act_fmt):
    """The pre-activation output of `second` from the NCHW input `x` of `gdn` in two launches: `ops.mx_gdn` writing the GDN's output
    packed in `act_fmt`, and `second` (`_chain_step`) on that operand.  Bit for bit second's `native_conv` / `native_tconv` on
    `native_gdn(gdn, x, act_fmt)`: no fp32 tensor lies between the two.  ValueError naming the modules and the reason for a pair
    `native_gdn_chain_refusal` gives a reason for."""
    why = native_gdn_chain_refusal(gdn, second)
    if why is not None:
        raise ValueError(f"native_gdn_chain: modules {_describe(gdn)} -> {_describe(second)}: {why}")
    _, shape = _gdn_rows("native_gdn_chain", gdn, x)
    return _chain_step(second, native_gdn(gdn, x, act_fmt, out_fmt=act_fmt), shape)[0].permute(0, 3, 1, 2)


# ---- Swin blocks: LayerNorm producer and the MLP half (include/rdo_ptq_mxswin.h) ---------------------------------------------------------------
def _act_quant_on(m):
    """whether the output quantiser of a QuantModule, or the `_aq` of a block, rounds in the present state"""
    return not getattr(m, "disable_act_quant", False) and m.use_act_quant and m.trained


def swin_quantisers_idle(block):
    """no activation quantiser rounds between the launches `native_ln_linear` and `native_swin_mlp` fuse"""
    return not any(_act_quant_on(m) for m in (block.norm1, block.norm2, block.mlp.fc2, block.mlp))


def native_swin_refusal(block):
    """None for a `QuantSwinTransformerBlock` whose forward `native_ln_linear` and `native_swin_mlp` serve, else the reason it keeps its
    forward, looked for in this order: a LayerNorm not over the last dimension only; C or the hidden width no multiple of 32 or above
    `hipops._lib.MXSWIN_MAX_C` / `MXSWIN_MAX_HIDDEN`; qkv, fc1 or fc2 not native-eligible (`native_refusal`), or fc1 and fc2 in different
    weight formats; an activation that is not the exact-erf `nn.GELU`; an `se_module` or an activation function on one of the five
    modules; an active activation quantiser on norm1, norm2, fc2 or the MLP's `_aq`."""
    from .quantizer import StraightThrough
    fc1, fc2, qkv = block.mlp.fc1, block.mlp.fc2, block.attn.qkv
    Hd, C = (int(v) for v in fc1.weight.shape)
    for name, n in (("norm1", block.norm1), ("norm2", block.norm2)):
        ns = tuple(n.fwd_kwargs["normalized_shape"])
        if n.kind != "layernorm" or ns != (C,):
            return f"{name} normalises over {ns}, not over the last dimension of {C} channels alone"
    if C % L.MX_BLOCK or Hd % L.MX_BLOCK:
        return f"its {C} channels or its hidden width {Hd} are no multiple of the MX block size {L.MX_BLOCK}"
    if C > L.MXSWIN_MAX_C or Hd > L.MXSWIN_MAX_HIDDEN:
        return f"its {C} channels are above {L.MXSWIN_MAX_C} or its hidden width {Hd} above {L.MXSWIN_MAX_HIDDEN}, the most the kernel's LDS serves"
    for name, m in (("attn.qkv", qkv), ("mlp.fc1", fc1), ("mlp.fc2", fc2)):
        why = native_refusal(m)
        if why is not None:
            return f"{name}: {why}"
    if fc1.weight_quantizer.fmt != fc2.weight_quantizer.fmt:
        return f"fc1's weights are in {fc1.weight_quantizer.fmt} and fc2's in {fc2.weight_quantizer.fmt}: the kernel takes one weight format"
    act = block.mlp.act
    if not isinstance(act, nn.GELU) or getattr(act, "approximate", "none") != "none":
        return f"the MLP's activation is {act!r}, not the exact-erf nn.GELU"
    for name, m in (("norm1", block.norm1), ("norm2", block.norm2), ("attn.qkv", qkv), ("mlp.fc1", fc1), ("mlp.fc2", fc2)):
        if m.se_module is not None or not isinstance(m.activation_function, (StraightThrough, nn.Identity)):
            return f"{name} has an se_module or an activation function of its own"
    if not swin_quantisers_idle(block):
        return "an activation quantiser is active on norm1, norm2, fc2 or between GELU and fc2"
    return None


def _ln_params(norm):
    """(weight, bias, eps) of a LayerNorm QuantModule in its present quant state, as the module's forward takes them"""
    w, b = norm._weights()
    return (None if w is None else w.detach().contiguous(), None if b is None else b.detach().contiguous(),
            float(norm.fwd_kwargs.get("eps", 1e-5)))


def native_ln_linear(norm, linear, x, act_fmt):
    """The pre-activation output of the eligible Linear `linear` on LayerNorm(x) of the QuantModule `norm` in two launches:
    `ops.mx_layer_norm_pack` writes the LayerNorm packed in `act_fmt`, `ops.mx_gemm` reads it.  Bit for bit `native_linear(linear,
    ops.add_layer_norm(x, None, weight, bias), act_fmt)`: no fp32 LayerNorm reaches memory.  Neither module's tail is applied."""
    w = native_operand(linear)
    rows, shape = native_rows(linear, x)
    lw, lb, eps = _ln_params(norm)
    return shape(ops.mx_gemm(ops.mx_layer_norm_pack(rows, None, lw, lb, act_fmt, eps=eps), w, native_bias(linear)))


def native_swin_mlp(block, x, a, act_fmt):
    """The second half of a `QuantSwinTransformerBlock` `native_swin_refusal` accepts, before the block's `_aq`, in one
    `ops.mx_swin_mlp` launch: x [B, L, C] is the block's input, a the attention branch; -> t + fc2(gelu(fc1(norm2(t)))) with t = x + a,
    both activations quantised to `act_fmt`, the weights the memoised `native_operand`s of fc1 and fc2.  a = None: x is t itself, the
    output of `native_swin_attn`."""
    why = native_swin_refusal(block)
    if why is not None:
        raise ValueError(f"native_swin_mlp: {why}")
    fc1, fc2 = block.mlp.fc1, block.mlp.fc2
    C = int(fc1.weight.shape[1])
    if x.shape[-1] != C or (a is not None and a.shape != x.shape):
        raise ValueError(f"native_swin_mlp: x must be [..., {C}] and a like x, got {tuple(x.shape)} and {tuple(a.shape)}")
    lw, lb, eps = _ln_params(block.norm2)
    out = ops.mx_swin_mlp(x.reshape(-1, C).contiguous(), None if a is None else a.reshape(-1, C).contiguous(), lw, lb, native_operand(fc1), native_bias(fc1),
                          native_operand(fc2), native_bias(fc2), act_fmt, eps=eps)
    return out.reshape(x.shape)


# ---- window attention with both products on the instruction (include/rdo_ptq_mxattn.h) ----------------------------------------------------------
def native_attention_refusal(attn):
    """None for a module whose attention core `native_attention` serves, else the reason it keeps its fp32 core, looked for in this order:
    it is no `QuantWindowAttention`; its head dim is no multiple of 4 (the kernel has no scalar path); its activation quantiser would
    round the probabilities and attn @ v (`use_act_quant` and `trained`: that path has its own two-launch split)."""
    from .quant_block import QuantWindowAttention
    if not isinstance(attn, QuantWindowAttention):
        return f"a {type(attn).__name__} is no QuantWindowAttention"
    hd = attn.dim // attn.num_heads
    if hd % 4:
        return f"its head dim {hd} ({attn.dim} channels, {attn.num_heads} heads) is no multiple of 4"
    if attn.use_act_quant and attn.trained:
        return "its activation quantiser rounds the probabilities and attn @ v between the two products"
    return None


def native_attention(attn, qkv, B, H, W, window, shift, fmt, p_fmt=None):
    """The attention core of a `QuantWindowAttention` `native_attention_refusal` accepts in one `ops.mx_window_attention` launch: qkv [B,
    H * W, 3C] the qkv linear's output in natural token order -> [B, H * W, C], the input of `proj`.  Q and K are quantised to `fmt` in
    blocks of 32 along the head dim, the probabilities to `p_fmt` (None: fmt) along the keys and V to `fmt` along the window's tokens; both
    products run on the block-scaled matrix instruction.  This is not the fp32 attention on rounded inputs of a Linear: four tensors are
    rounded, V along another axis than any Linear would round it."""
    why = native_attention_refusal(attn)
    if why is not None:
        raise ValueError(f"native_attention: {why}")
    C = attn.dim
    if qkv.dim() != 3 or tuple(qkv.shape) != (B, H * W, 3 * C):
        raise ValueError(f"native_attention: qkv must be [{B}, {H * W}, {3 * C}], got {tuple(qkv.shape)}")
    d = ops.attn_desc(B, H, W, C, attn.num_heads, window, shift, attn.scale)
    return ops.mx_window_attention(d, qkv.contiguous().view(B, H, W, 3 * C), attn.position_bias(), fmt, p_fmt).view(B, H * W, C)


# ---- the attention half of a Swin block in one launch (include/rdo_ptq_mxswinattn.h) ------------------------------------------------------------
def native_swin_attn_refusal(block):
    """None for a `QuantSwinTransformerBlock` whose attention half `native_swin_attn` serves, else the reason it keeps its five launches,
    looked for in this order: `native_swin_refusal`'s reason; `native_attention_refusal`'s for its attention; proj not native-eligible
    (`native_refusal`), or qkv and proj in different weight formats; C above `hipops._lib.MXSWINATTN_MAX_C`; an `se_module` or an
    activation function on proj; an active activation quantiser on qkv or proj."""
    from .quantizer import StraightThrough
    why = native_swin_refusal(block)
    if why is None:
        why = native_attention_refusal(block.attn)
    if why is not None:
        return why
    qkv, proj = block.attn.qkv, block.attn.proj
    why = native_refusal(proj)
    if why is not None:
        return f"attn.proj: {why}"
    if qkv.weight_quantizer.fmt != proj.weight_quantizer.fmt:
        return f"qkv's weights are in {qkv.weight_quantizer.fmt} and proj's in {proj.weight_quantizer.fmt}: the kernel takes one weight format"
    C = int(proj.weight.shape[1])
    if C > L.MXSWINATTN_MAX_C:
        return f"its {C} channels are above {L.MXSWINATTN_MAX_C}, the most the kernel's LDS serves"
    if proj.se_module is not None or not isinstance(proj.activation_function, (StraightThrough, nn.Identity)):
        return "attn.proj has an se_module or an activation function of its own"
    if _act_quant_on(qkv) or _act_quant_on(proj):
        return "an activation quantiser is active on qkv or proj"
    return None


def native_swin_attn(block, x, H, W, act_fmt):
    """The first half of a `QuantSwinTransformerBlock` `native_swin_attn_refusal` accepts in one `ops.mx_swin_attn` launch: x [B, L, C]
    is the block's input, L = H * W -> x + proj(attention(qkv(norm1(x)))) as [B, L, C], every activation -- the LayerNorm, Q, K, V, the
    probabilities, the attention output -- quantised to `act_fmt`, the weights the memoised `native_operand`s of qkv and proj.  The bits of
    `native_ln_linear`, `native_attention` (p_fmt = act_fmt), proj's `native_linear` and `ops.add`, without their round trips through
    memory."""
    why = native_swin_attn_refusal(block)
    if why is not None:
        raise ValueError(f"native_swin_attn: {why}")
    attn = block.attn
    C = attn.dim
    if x.dim() != 3 or x.shape[1] != H * W or x.shape[2] != C:
        raise ValueError(f"native_swin_attn: x must be [B, {H * W}, {C}], got {tuple(x.shape)}")
    B = int(x.shape[0])
    lw, lb, eps = _ln_params(block.norm1)
    d = ops.attn_desc(B, H, W, C, attn.num_heads, block.window_size, block.shift_size, attn.scale)
    return ops.mx_swin_attn(d, x.contiguous(), lw, lb, native_operand(attn.qkv), native_bias(attn.qkv), native_operand(attn.proj),
                            native_bias(attn.proj), attn.position_bias(), act_fmt, eps=eps)


# ---- the residual unit of the Cheng2020 attention block in one launch (include/rdo_ptq_mxresunit.h) ---------------------------------------------
def _residual_unit_convs(unit):
    """the three conv QuantModules of a `lic.layers._ResidualUnit` after the surgery: `unit.conv` is (conv, StraightThrough, conv,
    StraightThrough, conv) -- `quant_module_refactor` folds each ReLU into the QuantModule before it --; None for anything else"""
    seq = getattr(unit, "conv", None)
    if not isinstance(seq, nn.Sequential) or len(seq) != 5:
        return None
    convs = (seq[0], seq[2], seq[4])
    return convs if all(getattr(m, "kind", None) == "conv" for m in convs) else None


def native_residual_unit_refusal(unit):
    """None for a `_ResidualUnit` whose forward `native_residual_unit` serves, else the reason it keeps its forward, looked for in this
    order: its three convs are not 1x1 / 3x3 stride 1 padding 1 / 1x1 (dilation 1, groups 1) with N -> N/2 -> N/2 -> N channels; a weight
    is on no MX grid, or the three weight formats differ; N is no multiple of 64 or above `hipops._lib.MXRESUNIT_MAX_N`; a conv has an
    `se_module`, or the activation functions are not exactly ReLU, ReLU, none; an activation quantiser is active on one of the three."""
    from .quantizer import StraightThrough
    convs = _residual_unit_convs(unit)
    if convs is None:
        return f"a {type(unit).__name__} does not hold the three convs of a residual unit"
    c1, c2, c3 = convs
    N = int(c1.weight.shape[1])
    if N % 2:
        return f"its {N} channels are odd"
    want = (((N // 2, N, 1, 1), 0), ((N // 2, N // 2, 3, 3), 1), ((N, N // 2, 1, 1), 0))
    for name, m, (shape, pad) in zip(("conv.0", "conv.2", "conv.4"), convs, want):
        kw = m.fwd_kwargs
        if (tuple(m.weight.shape) != shape or isinstance(kw["padding"], str) or _pair(kw["stride"]) != (1, 1) or _pair(kw["padding"]) != (pad, pad)
                or _pair(kw["dilation"]) != (1, 1) or kw["groups"] != 1):
            return (f"{name} has weight {tuple(m.weight.shape)}, stride {kw['stride']}, padding {kw['padding']}, dilation {kw['dilation']}, groups "
                    f"{kw['groups']}, not weight {shape}, stride 1, padding {pad}")
    for name, m in zip(("conv.0", "conv.2", "conv.4"), convs):
        if not is_mx_any(m.weight_quantizer):
            return f"{name}: its weight quantiser is a {type(m.weight_quantizer).__name__}, not an MXQuantizer or MXAdaRoundQuantizer"
    fmts = [m.weight_quantizer.fmt for m in convs]
    if len(set(fmts)) != 1:
        return f"its weights are in {fmts[0]}, {fmts[1]} and {fmts[2]}: the kernel takes one weight format"
    if N % (2 * L.MX_BLOCK):
        return f"its {N} channels are no multiple of {2 * L.MX_BLOCK}: N / 2 must be whole MX blocks"
    if N > L.MXRESUNIT_MAX_N:
        return f"its {N} channels are above {L.MXRESUNIT_MAX_N}, the most the kernel's LDS serves"
    if any(m.se_module is not None for m in convs):
        return "one of its convs has an se_module"
    if (type(c1.activation_function) is not nn.ReLU or type(c2.activation_function) is not nn.ReLU
            or not isinstance(c3.activation_function, (StraightThrough, nn.Identity))):
        return (f"its activation functions are {type(c1.activation_function).__name__}, {type(c2.activation_function).__name__} and "
                f"{type(c3.activation_function).__name__}, not ReLU, ReLU and none")
    if any(_act_quant_on(m) for m in convs):
        return "an activation quantiser is active on one of its three convs"
    return None


def residual_unit_format(unit, x):
    """the activation format where `mx_resunit` is set on a `_ResidualUnit` (`QuantModel.set_mx_activations(..., residual_units=True)`),
    its three convs carry the same (act_fmt, 'native') with their quantised weights, no activation quantiser rounds between them and the
    input is not tracked; else None: the unit keeps its module-by-module forward"""
    convs = _residual_unit_convs(unit) if getattr(unit, "mx_resunit", False) else None
    if convs is None or (torch.is_grad_enabled() and x.requires_grad):
        return None
    on = getattr(convs[0], "mx_activations", None)
    if on is None or on[1] != "native" or any(getattr(m, "mx_activations", None) != on or not m.use_weight_quant or _act_quant_on(m) for m in convs):
        return None
    return on[0]


def _residual_unit_forward(unit, x):
    """`_ResidualUnit.fused_forward`: the one launch where `residual_unit_format` gives a format, else None -- the unit's own forward"""
    fmt = residual_unit_format(unit, x)
    return None if fmt is None else native_residual_unit(unit, x, fmt)


def native_residual_unit(unit, x, act_fmt):
    """The output of a `_ResidualUnit` `native_residual_unit_refusal` accepts in one `ops.mx_residual_unit` launch: x is the unit's NCHW
    input -> relu(x + conv1x1(relu(conv3x3(relu(conv1x1(x)))))) as a channels-last view [B, N, H, W], with x and the two intermediate
    tensors quantised to `act_fmt` in LDS, the weights the memoised `native_conv_operand`s and the biases those of the modules' present
    quant state.  The bits of the three modules' `native_conv` forwards with their un-fused ReLUs, the add and the last ReLU."""
    why = native_residual_unit_refusal(unit)
    if why is not None:
        raise ValueError(f"native_residual_unit: {why}")
    c1, c2, c3 = _residual_unit_convs(unit)
    N = int(c1.weight.shape[1])
    if x.dim() != 4 or x.shape[1] != N:
        raise ValueError(f"native_residual_unit: the input must be [B, {N}, H, W], got {tuple(x.shape)}")
    B, _, H, W = (int(v) for v in x.shape)
    out = ops.mx_residual_unit(x.permute(0, 2, 3, 1).reshape(-1, N).contiguous(), (B, H, W), native_conv_operand(c1), native_bias(c1),
                               native_conv_operand(c2), native_bias(c2), native_conv_operand(c3), native_bias(c3), act_fmt)
    return out.reshape(B, H, W, N).permute(0, 3, 1, 2)


# the model package does not know this one: the unit's class gets the hook here, `set_mx_activations` sets `mx_resunit` per unit
from lic.layers import _ResidualUnit  # noqa: E402

_ResidualUnit.fused_forward = _residual_unit_forward


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
    with its quantised weight pack and EPI_NONE.
    A GDN / IGDN (`set_mx_activations(..., gdn=True)`): 'native' is `native_gdn`; 'emulated' the fp32 GDN kernel on the decoded operands --
    xq of `ops.mx_quant_pack(x o x, act_fmt, want_xq=True)` as the pool's input (square_input=False), the decoded gamma' of
    `native_gdn_operand` with beta' as its weight pack, EPI_GDN / EPI_IGDN with aux = x."""
    act_fmt, mode = module.mx_activations
    kind = module.kind
    if kind == "gdn":
        if mode == "native":
            return native_gdn(module, x, act_fmt)
        rows, (B, H, W) = _gdn_rows("mx_forward", module, x)
        _, xq = ops.mx_quant_pack(rows * rows, act_fmt, want_xq=True)
        y = ops.conv2d_fwd_pack(xq.reshape(B, H, W, -1), _gdn_operands(module)[1], 1, 0,
                                epilogue=L.EPI_IGDN if module.fwd_kwargs["inverse"] else L.EPI_GDN, aux=rows.reshape(B, H, W, -1),
                                square_input=False)
        return y.permute(0, 3, 1, 2)
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
