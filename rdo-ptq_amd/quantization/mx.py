"""`MXQuantizer`: a weight quantiser on the OCP microscaling (MX) block formats (include/rdo_ptq_mx.h; `ops.mx_fakequant`): blocks of 32
elements along the GEMM's K dimension, one shared power-of-two scale per block, FP4 / FP6 / FP8 elements.  Round to nearest only:
learned rounding on MX grids, MX activations and a packed MX container are not built."""
import torch
import torch.nn as nn

from hipops import _lib as L
from hipops import ops

from .quantizer import from_rows, to_rows

MX_FORMATS = tuple(L.MX_FORMATS)


def is_mx(q):
    return isinstance(q, MXQuantizer)


def refuse_mx(what, named_modules, error, why):
    """raise `error` naming the first module of (name, module) pairs whose weight quantiser is an `MXQuantizer`"""
    for name, m in named_modules:
        q = getattr(m, "weight_quantizer", None)
        if is_mx(q):
            raise error(f"{what}: module {name!r} holds an MXQuantizer ({q.fmt}): {why}")


class MXQuantizer(nn.Module):
    """Fake-quantises a weight to the MX format `fmt` (a name of `hipops._lib.MX_FORMATS`).  Called on a weight it returns the quantised
    weight in the weight's own shape.  The blocks run along the rows of `to_rows(weight, tconv)` -- conv: one row per output channel in
    (kh, kw, in) order; transposed conv: tconv=True; Linear: as stored; a 1-D weight is one row -- whatever `channel_wise` was on the
    quantiser it replaces: the block structure follows K.  There is no state to initialise: every call derives the scales from the weight.

    It carries what `QuantModule._weight_state` reads of a weight quantiser (inited = True, n_bits = the element bits, n_levels = 2 **
    n_bits, delta = zero_point = None), `fmt`, and `size_bits(weight)` = element bits x elements + 8 x blocks.  `QuantModel.weight_bits()`
    reads n_bits and so counts the element bits only, not the scales.

    Weights only: a call with act=True raises NotImplementedError (MX activations are not built)."""

    def __init__(self, fmt: str, tconv: bool = False):
        super().__init__()
        _, bits = ops.mx_format("MXQuantizer", fmt)
        self.fmt, self.tconv = fmt, bool(tconv)
        self.n_bits, self.n_levels = bits, 2 ** bits
        self.delta = self.zero_point = None
        self.inited = True

    def _rows(self, x):
        wr = to_rows(x, self.tconv)
        return wr.reshape(wr.shape[0], -1)

    def forward(self, x: torch.Tensor, act: bool = False, **kw):
        if act:
            raise NotImplementedError(f"MXQuantizer({self.fmt}): MX activations are not built; this quantiser serves weights only")
        wr = to_rows(x.detach(), self.tconv)
        wq = ops.mx_fakequant(wr.reshape(wr.shape[0], -1), self.fmt)["wq"].reshape(wr.shape)
        return from_rows(wq, x, self.tconv)

    def weight_cost(self, x):
        """(err, energy) float64 [rows] of `x` in this format, on the device: sum (w - wq)^2 and sum w^2 per row of `to_rows`"""
        out = ops.mx_fakequant(self._rows(x.detach()), self.fmt, want=("err", "energy"))
        return out["err"], out["energy"]

    def size_bits(self, weight):
        """element bits x elements + 8 x blocks, the blocks counted along the rows of `to_rows(weight)`"""
        rows = 1 if weight.dim() == 1 else int(weight.shape[1] if (self.tconv and weight.dim() == 4) else weight.shape[0])
        inner = int(weight.numel()) // rows
        return self.n_bits * rows * inner + 8 * rows * -(-inner // L.MX_BLOCK)

    def extra_repr(self):
        return f"fmt={self.fmt}, bit={self.n_bits}, tconv={self.tconv}"
