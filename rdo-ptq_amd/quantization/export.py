"""True-integer export of a calibrated QuantModel (in the spirit of light-uniform-PTQ/quant_int/quant_layer.py:116-122,
which overwrites weights with uint8 levels): for every trained QuantModule the unsigned integer levels, the per-channel
scale `delta` and the zero point, such that  w_q = (levels - zero_point) * delta  is exactly the hard-rounded weight the
module uses at inference (`AdaRoundQuantizer.forward` with soft_targets=False, quantizer.py:441-449)."""
from collections import OrderedDict

import torch

from .quant_layer import QuantModule
from .quantizer import AdaRoundQuantizer


def integer_state(qnn) -> "OrderedDict[str, dict]":
    """name -> {levels (uint8, or int32 above 8 bits; logical weight shape), delta, zero_point, n_bits, bias, kind}."""
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
                     "n_bits": q.n_bits, "bias": None if m.org_bias is None else m.org_bias.detach().cpu(), "kind": m.kind}
    return out


def activation_state(qnn) -> "OrderedDict[str, dict]":
    """name -> {lo, hi (fp32 [channels], CPU), n_bits, channels} of every frozen static activation quantiser (`QuantModel.act_ranges`):
    x_q = round(clamp((x - lo) / r, 0, 1) * (2^n_bits - 1)) / (2^n_bits - 1) * r + lo with r = max(hi - lo, 1e-6), per channel.
    Empty for a model whose activation quantisers are dynamic: there is nothing fixed to write."""
    out = OrderedDict()
    for name, (lo, hi, n_bits) in qnn.act_ranges().items():
        out[name] = {"lo": lo.detach().cpu().clone(), "hi": hi.detach().cpu().clone(), "n_bits": int(n_bits), "channels": int(lo.numel())}
    return out


def activation_report(qnn) -> "OrderedDict[str, dict]":
    """name -> {err, energy (fp32 [channels]), clip_lo, clip_hi (int32 [channels]), n, sqnr_db, clipped_share (float64 [channels]), n_bits,
    channels} of every frozen static activation range whose statistics were recorded (args.act_report; the names of
    `QuantModel.act_ranges`), on the CPU: the squared error of the frozen grid measured on the calibration inputs, their energy sum x^2,
    the counts of the values below and above the range, the values seen per channel; sqnr_db = 10 log10(energy / err) in float64 (inf
    where err == 0), clipped_share = (clip_lo + clip_hi) / n.  Empty for a model without recorded statistics."""
    out = OrderedDict()
    for name, q in qnn.act_quantizers():
        stats = getattr(q, "act_stats", None) or {}
        if not q.act_frozen():
            continue
        for site in sorted(q.act_range):
            st = stats.get(site)
            if st is None:
                continue
            err, energy = st["err"].detach().cpu().clone(), st["energy"].detach().cpu().clone()
            lo, hi, n = st["clip_lo"].detach().cpu().clone(), st["clip_hi"].detach().cpu().clone(), int(st["n"])
            e64, s64 = err.double(), energy.double()
            sqnr = torch.where(e64 == 0, torch.full_like(e64, float("inf")), 10.0 * torch.log10(s64 / e64))
            out[name if site == 0 else f"{name}#{site}"] = {
                "err": err, "energy": energy, "clip_lo": lo, "clip_hi": hi, "n": n, "sqnr_db": sqnr,
                "clipped_share": (lo.double() + hi.double()) / max(n, 1), "n_bits": int(getattr(q, "dynamic_bits", 8)),
                "channels": int(err.numel())}
    return out


UNIT_REPORT_STATES = ("nearest", "learned")


def unit_report(qnn) -> "OrderedDict[str, dict]":
    """unit name -> the measured output error of every calibrated unit whose statistics were recorded (args.unit_report;
    `recon.report_unit`), in module order, on the CPU.  With d = full-precision output - quantised output of the unit on its cached
    calibration inputs, per output channel and for both states 'nearest' (every trained weight rounded to nearest) and 'learned' (the
    unit as calibrated):
      channels, n                    channel count; pixels per channel (all ranks)
      err, shift, energy [state]     float64 [C]: sum d^2, sum d, sum of the squared full-precision output
      sqnr_db [state]                float64 [C]: 10 log10(energy / err), inf where err == 0
      gain_db                        float64 [C]: sqnr_db['learned'] - sqnr_db['nearest'] (what the learned rounding gained)
      shift_share [state]            float64 [C]: shift^2 / (n err), 0 where err == 0: the part of the squared error that a per-channel
                                     bias would remove (in [0, 1] by Cauchy-Schwarz)
      total                          {err, shift, energy, sqnr_db [state], gain_db}: the same over the summed channels (Python floats)
    Empty for a model without recorded statistics."""
    def sqnr(energy, err):
        return torch.where(err == 0, torch.full_like(err, float("inf")), 10.0 * torch.log10(energy / err))
    out = OrderedDict()
    for _, m in qnn.named_modules():
        st = getattr(m, "unit_stats", None)
        if not st:
            continue
        n = int(st["n"])
        row = {"n": n, "total": {}}
        for f in ("err", "shift", "energy", "sqnr_db", "shift_share"):
            row[f] = {}
            if f in ("err", "shift", "energy", "sqnr_db"):
                row["total"][f] = {}
        for state in UNIT_REPORT_STATES:
            shift, err, energy = (st[state][f].detach().to("cpu", torch.float64).clone() for f in ("shift", "err", "energy"))
            row["err"][state], row["shift"][state], row["energy"][state] = err, shift, energy
            row["sqnr_db"][state] = sqnr(energy, err)
            row["shift_share"][state] = torch.where(err == 0, torch.zeros_like(err), shift * shift / (max(n, 1) * err))
            row["total"]["err"][state], row["total"]["shift"][state] = float(err.sum()), float(shift.sum())
            row["total"]["energy"][state] = float(energy.sum())
            row["total"]["sqnr_db"][state] = float(sqnr(energy.sum(), err.sum()))
        row["channels"] = int(row["err"]["learned"].numel())
        row["gain_db"] = row["sqnr_db"]["learned"] - row["sqnr_db"]["nearest"]
        row["total"]["gain_db"] = row["total"]["sqnr_db"]["learned"] - row["total"]["sqnr_db"]["nearest"]
        out[str(st["name"])] = row
    return out


def dequantize(entry) -> torch.Tensor:
    return (entry["levels"].to(torch.float32) - entry["zero_point"]) * entry["delta"]
