"""Weight quantisers on the OCP microscaling (MX) block formats (include/rdo_ptq_mx.h): blocks of 32 elements along the GEMM's K
dimension, one shared power-of-two scale per block, FP4 / FP6 / FP8 elements.  `MXQuantizer` rounds to nearest (`ops.mx_fakequant`);
`MXAdaRoundQuantizer` carries learned rounding on the same grids (include/rdo_ptq_mxround.h; `QuantModel.set_weight_format(...,
rounding='learned')`, then `reconstruct`).  MX activations and a packed MX container are not built."""
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
            raise NotImplementedError(f"{type(self).__name__}({self.fmt}): MX activations are not built; this quantiser serves weights only")

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

    Weights only: a call with act=True raises NotImplementedError (MX activations are not built)."""

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

    Weights only: a call with act=True raises NotImplementedError (MX activations are not built)."""

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
