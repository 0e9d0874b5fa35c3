"""True-integer export of a calibrated QuantModel (in the spirit of light-uniform-PTQ/quant_int/quant_layer.py:116-122,
which overwrites weights with uint8 levels): for every trained QuantModule the unsigned integer levels, the per-channel
scale `delta` and the zero point, such that  w_q = (levels - zero_point) * delta  is exactly the hard-rounded weight the
module uses at inference (`AdaRoundQuantizer.forward` with soft_targets=False, quantizer.py:441-449); and the frozen activation ranges.

The reports (`reports.py`) and the width allocators (`widths.py`) are documented under this module's name (`export.rd_report`,
`export.allocate_bits`, ...): the two import lines at the end keep that path."""
from collections import OrderedDict

import torch

from .quant_layer import QuantModule
from .quantizer import AdaRoundQuantizer


def integer_state(qnn) -> "OrderedDict[str, dict]":
    """name -> {levels (uint8, or int32 above 8 bits; logical weight shape), delta, zero_point, n_bits, bias, kind}.  `bias` is the one
    the quantised forward uses (`m.bias`): `org_bias` unless a bias correction moved it (`unit_passes.correct_unit_bias`).  ValueError
    for a model that holds an `MXQuantizer` (`QuantModel.set_weight_format`): an MX grid has no levels, delta and zero point."""
    from .mx import refuse_mx
    refuse_mx("integer_state", qnn.named_modules(), ValueError, "an MX grid has no integer levels, delta and zero point to export")
    out = OrderedDict()
    for name, m in qnn.named_modules():
        if not isinstance(m, QuantModule) or m.org_weight is None:
            continue
        q = m.weight_quantizer
        if not q.inited if hasattr(q, "inited") else False:
            continue
        w = m.org_weight
        d, z = q.delta.to(w.device), q.zero_point.to(w.device)
        if isinstance(q, AdaRoundQuantizer):
            up = (q.alpha.detach() >= 0).to(w.dtype)
            x_int = torch.floor(w / d) + up
        else:
            x_int = torch.round(w / d)
        levels = torch.clamp(x_int + z, 0, q.n_levels - 1)
        out[name] = {"levels": levels.to(torch.uint8 if q.n_bits <= 8 else torch.int32).cpu(), "delta": d.detach().cpu(), "zero_point": z.detach().cpu(),
                     "n_bits": q.n_bits, "bias": None if m.bias is None else m.bias.detach().cpu(), "kind": m.kind}
    return out


def activation_state(qnn) -> "OrderedDict[str, dict]":
    """name -> {lo, hi (fp32 [channels], CPU), n_bits, channels} of every frozen static activation quantiser (`QuantModel.act_ranges`):
    x_q = round(clamp((x - lo) / r, 0, 1) * (2^n_bits - 1)) / (2^n_bits - 1) * r + lo with r = max(hi - lo, 1e-6), per channel.
    Empty for a model whose activation quantisers are dynamic: there is nothing fixed to write."""
    out = OrderedDict()
    for name, (lo, hi, n_bits) in qnn.act_ranges().items():
        out[name] = {"lo": lo.detach().cpu().clone(), "hi": hi.detach().cpu().clone(), "n_bits": int(n_bits), "channels": int(lo.numel())}
    return out


def dequantize(entry) -> torch.Tensor:
    return (entry["levels"].to(torch.float32) - entry["zero_point"]) * entry["delta"]


from .reports import act_bit_report, act_width_report, activation_report, bias_report, bit_report, format_report, rd_report, unit_report  # noqa: E402,F401
from .widths import act_applied, act_modules, allocate_act_bits, allocate_bits, allocate_formats, is_trained, weighted_modules  # noqa: E402,F401
