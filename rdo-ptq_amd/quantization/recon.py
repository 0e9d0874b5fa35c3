"""Shared body of `layer_reconstruction` / `block_reconstruction` (reference: layer_opt.py:175-320, block_opt.py:176-324).

The choreography around the hot loop is the reference's; the loop itself runs on `engine.UnitEngine`."""
import logging
import time
import zlib
from collections import OrderedDict

import torch

from . import dp
from hipops import ops
from .engine import UnitEngine
from .quant_block import BaseQuantBlock, QuantRSTB
from .swin_engine import TapeEngine
from .quant_layer import QuantModule, _nhwc, _sq
from .quantizer import AdaRoundQuantizer, to_rows
from .utils import LinearTempDecay, save_inp_oup_data, set_mode

_COOPS = ("g_a", "h_a", "h_s", "g_s")
BIAS_CORRECT_MODES = ("weight", "output")


def find_unquantized_module(model, _name_="g_a", module_list=None, name_list=None):
    """Switch every untrained unit to full precision and collect those of the current sub-coder (layer_opt.py:15-43).
    For Sequential-indexed models the names never contain g_a/h_a/h_s/g_s, so the lists stay empty."""
    module_list = [] if module_list is None else module_list
    name_list = [] if name_list is None else name_list
    for name, module in model.named_children():
        if isinstance(module, (QuantModule, BaseQuantBlock)):
            if not module.trained:
                module.set_quant_state(False, False)
                for tag in _COOPS:
                    if tag in _name_ and tag in name:
                        name_list.append(name)
                        module_list.append(module)
        else:
            find_unquantized_module(module, _name_, module_list, name_list)
    return module_list[1:], name_list[1:]


def fp_out(module_list, x, round_after, batch=8):
    """`fp_out` of the reference (layer_opt.py:45-75) over a whole cache: the remaining stages of the sub-coder in full
    precision (their quant state was switched off by find_unquantized_module), then round for analysis-transform units."""
    outs = []
    with torch.no_grad():
        for i in range(0, x.shape[0], batch):
            h = x[i:i + batch]
            for m in module_list:
                h = m(h) if isinstance(m, QuantModule) else m(h, (h.shape[2], h.shape[3]))
            if round_after:
                h = ops.round_(_nhwc(h)).permute(0, 3, 1, 2)
            outs.append(h)
    return torch.cat(outs)


class LossFunction:
    """The objective of one reconstruction unit with the reference's call signature (layer_opt.py:87-173; the block variant,
    block_opt.py:87-173, sums the rounding term over the block's QuantModules).  The calibration engine evaluates the same three
    terms on the device inside the recorded iteration; this class is the inspection / logging form of it on torch tensors
    (used by the parity tests to evaluate the loss of a calibrated unit), not part of the hot loop."""

    def __init__(self, unit, round_loss="relaxation", weight=1., rec_loss="mse", max_count=2000, b_range=(10, 2),
                 decay_start=0.0, warmup=0.0, p=2., lmbda=None, metric=None):
        self.unit, self.round_loss, self.weight, self.rec_loss = unit, round_loss, weight, rec_loss
        self.layer = self.block = unit                 # attribute names of the two reference classes
        self.loss_start = max_count * warmup
        self.p, self.lmbda, self.metric = p, lmbda, metric
        self.temp_decay = LinearTempDecay(max_count, rel_start_decay=warmup + (1 - warmup) * decay_start,
                                          start_b=b_range[0], end_b=b_range[1])
        self.count = 0

    def _round_modules(self):
        if isinstance(self.unit, QuantModule):
            return [self.unit]
        return [m for m in self.unit.modules() if isinstance(m, QuantModule) and m.org_weight is not None]

    def __call__(self, pred, tgt, quant_net_out=None, cali_data=None, grad=None):
        from .quantizer import lp_loss
        self.count += 1
        if self.rec_loss != "mse":
            raise NotImplementedError("only rec_loss='mse' (the mode main2.py uses) is built")
        rec_loss = lp_loss(pred, tgt, p=self.p)
        task_loss = 0.
        if quant_net_out is not None:
            task_loss = lp_loss(quant_net_out, cali_data, p=self.metric)
        b = self.temp_decay(self.count)
        if self.count < self.loss_start or self.round_loss == "none":
            b = round_loss = 0
        elif self.round_loss == "relaxation":
            round_loss = 0
            for m in self._round_modules():
                round_vals = m.weight_quantizer.get_soft_targets()
                round_loss += self.weight * (1 - ((round_vals - .5).abs() * 2).pow(b)).sum()
        else:
            raise NotImplementedError
        total_loss = round_loss + rec_loss + task_loss
        if self.count % 500 == 0:
            logging.info("Total loss:\t{:.3f} ( task:{:.3f}, rec:{:.3f}, round:{:.3f})\tb={:.2f}\tcount={}".format(
                float(total_loss), float(task_loss), float(rec_loss), float(round_loss), b, self.count))
        return total_loss


def unit_seed(unit_name: str) -> int:
    """Seed of the QDrop stream of one unit: the process seed (main2.py seed_all -> torch.manual_seed) mixed with a CRC of the
    unit's name -- reproducible from run to run (Python's str hash is salted per process) and distinct per unit."""
    return (torch.initial_seed() ^ zlib.crc32(unit_name.encode())) & 0xFFFFFFFF


def _unit_modules(unit):
    """kind + the engine's module dict for a QuantModule or a Cheng2020 block."""
    if isinstance(unit, QuantModule):
        return "layer", {"layer": unit}
    kind = getattr(unit, "unit_kind", None)
    if kind == "rb":
        return kind, {"conv1": unit.conv1, "conv2": unit.conv2, "skip": unit.skip}
    if kind == "rbws":
        return kind, {"conv1": unit.conv1, "conv2": unit.conv2, "gdn": unit.gdn, "skip": unit.skip}
    if kind == "rbu":
        return kind, {"subpel_conv": unit.subpel_conv[0], "conv": unit.conv, "igdn": unit.igdn,
                      "upsample": unit.upsample[0], "upscale": unit.subpel_conv[1].upscale_factor}
    if kind == "rstb":
        return kind, {"rstb": unit}
    raise NotImplementedError(f"reconstruction of {type(unit).__name__} is not built yet")


def _rd_metric(args, cali_data):
    """args.rd_metric: the distortion of the loss_mode='rd' task term, 'mse' (default) or 'ms-ssim' (the objective of CompressAI's
    MS-SSIM checkpoints).  Not `args.metric`: LossFunction.metric is the --task_loss exponent.  Checked before any work is done:
    the five MS-SSIM scales of an 11-tap window need crops with both sides above 160 pixels."""
    metric = getattr(args, "rd_metric", "mse") if args is not None else "mse"
    if metric not in ("mse", "ms-ssim"):
        raise ValueError(f"unknown rd_metric {metric!r} ('mse' or 'ms-ssim')")
    if metric == "ms-ssim" and getattr(args, "loss_mode", "lp") == "rd" and min(cali_data.shape[-2:]) <= 160:
        raise ValueError(f"rd_metric='ms-ssim' needs calibration crops with both sides above 160 pixels (five scales of an 11-tap "
                         f"window); got {tuple(cali_data.shape[-2:])}")
    return metric


def _act_args(args):
    """args.act_mode: 'dynamic' (default; the reference's ActQuant) or 'static' (per-channel ranges frozen from the calibration set);
    args.act_range: how a static range is fixed, 'max' (default: min / max over the calibration set), 'l2' (each channel then shrinks
    to the best of ten candidates by squared error) or 'learned' (the 'l2' ranges are then trained on the unit's reconstruction error:
    `learn_act_ranges`, with args.act_iters steps, default 500, of size args.act_lr, default 1e-3, relative to a channel's observed
    width) or 'percentile' (a second pass takes a 1024-bin histogram of every channel on its observed range; each end then gives up whole
    bins while they hold no more than a share 1 - args.act_percentile / 100, default 99.99, of the channel's values) or 'hist_mse' (the
    same histogram pass; each channel then takes the clip pair, out of all 524 800, that minimises the modelled squared error on its
    grid width: `ops.act_hist_mse_select`) or 'auto' (one pass takes the 'l2' error sums and the histograms, the ranges that 'max', 'l2',
    'percentile' and 'hist_mse' would freeze are then SCORED on the same inputs, `ops.actquant_score`, and each channel takes the one of
    least measured squared error); args.act_report (default False; a bool): after freezing, one more pass records every site's measured
    error, energy and clipped counts (`export.activation_report`); args.unit_report (default False; a bool): a trained unit then measures
    its own output error on its cached inputs, learned rounding against round-to-nearest (`report_unit`, `export.unit_report`);
    args.bias_correct (default off; 'weight' or 'output'): a trained unit then corrects the biases of its conv, transposed-conv and
    Linear layers by the mean error of their pre-activations on the calibration set (`correct_unit_bias`, `export.bias_report`).
    Checked before any work is done."""
    mode = getattr(args, "act_mode", "dynamic") if args is not None else "dynamic"
    how = getattr(args, "act_range", "max") if args is not None else "max"
    if mode not in ("dynamic", "static"):
        raise ValueError(f"unknown act_mode {mode!r} ('dynamic' or 'static')")
    if how not in ("max", "l2", "learned", "percentile", "hist_mse", "auto"):
        raise ValueError(f"unknown act_range {how!r} ('max', 'l2', 'learned', 'percentile', 'hist_mse' or 'auto')")
    _act_learn_args(args)
    _act_percentile_args(args)
    _act_report_args(args)
    _unit_report_args(args)
    _bias_correct_args(args)
    return mode, how


def _act_report_args(args):
    """args.act_report, validated: a bool (default False)."""
    report = getattr(args, "act_report", False) if args is not None else False
    if not isinstance(report, bool):
        raise ValueError(f"act_report must be True or False, got {report!r}")
    return report


def _unit_report_args(args):
    """args.unit_report, validated: a bool (default False)."""
    report = getattr(args, "unit_report", False) if args is not None else False
    if not isinstance(report, bool):
        raise ValueError(f"unit_report must be True or False, got {report!r}")
    return report


def _bias_correct_args(args):
    """args.bias_correct, validated -> None (off: absent, None or False, the default), 'weight' or 'output'.  True is refused like every
    other value: the mode must be named."""
    mode = getattr(args, "bias_correct", None) if args is not None else None
    if mode is None or mode is False:
        return None
    if not isinstance(mode, str) or mode not in BIAS_CORRECT_MODES:
        raise ValueError(f"bias_correct must be 'weight', 'output' or off (None / False), got {mode!r}")
    return mode


def _act_learn_args(args):
    """(args.act_iters, args.act_lr) of act_range='learned', validated: a positive whole number of steps, a positive finite step size."""
    iters = getattr(args, "act_iters", 500) if args is not None else 500
    lr = getattr(args, "act_lr", 1e-3) if args is not None else 1e-3
    return _check_learn(iters, lr)


def _check_learn(iters, lr):
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"act_iters must be a positive integer, got {iters!r}")
    if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not (0.0 < float(lr) < float("inf")):
        raise ValueError(f"act_lr must be a positive finite number, got {lr!r}")
    return iters, float(lr)


def _act_percentile_args(args):
    """args.act_percentile of act_range='percentile', validated: a real number p with 50 < p <= 100 (100 = the max range)."""
    return _check_percentile(getattr(args, "act_percentile", 99.99) if args is not None else 99.99)


def _check_percentile(p):
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not (50.0 < float(p) <= 100.0):
        raise ValueError(f"act_percentile must be a number p with 50 < p <= 100, got {p!r}")
    return float(p)


def _is_rstb(unit):
    return isinstance(unit, QuantRSTB) or getattr(unit, "unit_kind", None) == "rstb"


def calibrate_act_ranges(unit, inp_q, act_range="max", batch=32, keep_obs=False, percentile=99.99):
    """Fix the static activation ranges of a calibrated unit: run it once over its cached quantised inputs in the state the W8A8
    evaluation uses (the unit, its QuantModules and nested block wrappers with weight and activation quantisation on) with its quantisers
    observing, then freeze them; with act_range='l2' a second pass over the same inputs accumulates the candidates' squared errors
    first; with act_range='percentile' the second pass takes every channel's histogram on its observed range, and freezing clips a
    share 1 - percentile / 100 of its values at each end; with act_range='hist_mse' the same pass is followed by the exhaustive search
    for the clip pair of least modelled squared error on the quantiser's grid width.  Under data parallelism the observed ranges and
    the error sums or histograms are reduced over the ranks before they are used, so every rank freezes the same grid (integer counts:
    the very grid of one process on all inputs).  Every quant state flag is left as it was found.  `keep_obs`: the quantisers keep the
    observed max ranges next to the frozen ones (`act_obs`) for `learn_act_ranges`.
    With act_range='auto' the second pass takes the 'l2' error sums AND the histograms (both read the same max-range inputs); from them
    every site forms the four ranges that 'max', 'l2', 'percentile' and 'hist_mse' would freeze (`act_candidates`), a third pass measures
    their squared error on the same inputs (`act_score`: still behind max-range upstream quantisers), and each channel freezes the one of
    least measured error.  The measured sums and counts are reduced over the ranks like the others, so every rank picks from the same
    numbers."""
    if act_range in ("percentile", "auto"):
        percentile = _check_percentile(percentile)
    mods = [m for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    quants = [m.act_quantizer for m in mods]
    states = [(m, m.use_weight_quant, m.use_act_quant) for m in mods]

    def run():
        with torch.no_grad():
            for i in range(0, inp_q.shape[0], batch):
                h = inp_q[i:i + batch]
                unit(h, (h.shape[2], h.shape[3])) if isinstance(unit, QuantRSTB) else unit(h)

    def applied(name):                   # in a fixed order: the collectives of all ranks must line up
        return [getattr(q, name)[k] for q in quants for k in sorted(getattr(q, name))]
    try:
        for m in mods:
            m.use_weight_quant = m.use_act_quant = True
        for q in quants:
            q.act_observe()
        run()
        dp.reduce_act_stats(ranges=applied("act_range"))
        if act_range == "l2":
            for q in quants:
                if q.act_range:
                    q.act_search()
            run()
            dp.reduce_act_stats(sums=applied("act_err"))
        elif act_range in ("percentile", "hist_mse"):
            for q in quants:
                if q.act_range:
                    q.act_histogram(percentile, rule="mse" if act_range == "hist_mse" else "percentile")
            run()
            dp.reduce_act_stats(sums=applied("act_hist"))
        elif act_range == "auto":
            seen = [q for q in {id(q): q for q in quants}.values() if q.act_range]
            for q in seen:
                q.act_histogram(percentile, rule="mse", search=True)
            run()
            dp.reduce_act_stats(sums=applied("act_err") + applied("act_hist"))
            for q in seen:
                q.act_score(q.act_candidates())
            run()
            _reduce_scores(seen)
        for q in quants:
            q.act_freeze(keep_obs=keep_obs)
    finally:
        for m, w, a_ in states:
            m.use_weight_quant, m.use_act_quant = w, a_


def _reduce_scores(quants):
    """the sums, counts and pixel counts of a scoring pass over the ranks, in the fixed site order"""
    def applied(name):
        return [getattr(q, name)[k] for q in quants for k in sorted(getattr(q, name))]
    if dp.world()[1] <= 1:
        return
    dp.reduce_act_stats(sums=applied("act_err") + applied("act_energy") + applied("act_clip"))
    sites = [(q, k) for q in quants for k in sorted(q.act_score_n)]
    if sites:
        n = torch.tensor([q.act_score_n[k] for q, k in sites], dtype=torch.int32, device=sites[0][0].act_err[sites[0][1]].device)
        dp.reduce_act_stats(sums=[n])                    # (the guard of the pass keeps the sum inside 32 bits)
        for (q, k), v in zip(sites, n.tolist()):
            q.act_score_n[k] = int(v)


def report_act_ranges(unit, inp_q, batch=32):
    """Measure the frozen static activation ranges of a calibrated unit: one pass over its cached quantised inputs in the W8A8 state, every
    frozen quantiser scoring its own range (K = 1) and passing its frozen output on; the measured squared error, the energy, the counts of
    the values clipped at each end and the pixel count stay on the quantiser as `act_stats[site]` (summed over the ranks under data
    parallelism).  The ranges do not change; every quant state flag is left as it was found."""
    mods = [m for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    quants = list({id(m.act_quantizer): m.act_quantizer for m in mods if m.act_quantizer.act_frozen()}.values())
    states = [(m, m.use_weight_quant, m.use_act_quant) for m in mods]
    try:
        for m in mods:
            m.use_weight_quant = m.use_act_quant = True
        for q in quants:
            q.act_score()
        with torch.no_grad():
            for i in range(0, inp_q.shape[0], batch):
                h = inp_q[i:i + batch]
                unit(h, (h.shape[2], h.shape[3])) if isinstance(unit, QuantRSTB) else unit(h)
        _reduce_scores(quants)
    finally:
        for q in quants:
            if getattr(q, "act_phase", "idle") == "score":
                q.act_freeze()
        for m, w, a_ in states:
            m.use_weight_quant, m.use_act_quant = w, a_


def _nearest_alpha(q, w):
    """A stand-in for the alpha of the AdaRoundQuantizer `q` of weight `w` whose sign makes the hard forward, floor(w / delta) + (alpha >=
    0), round to nearest: +1 where frac = w / delta - floor(w / delta) >= 0.5 (fp32, the quantiser's own rows and scales), -1 below."""
    wr = q._rows(w.detach())
    d, _ = q._row_scales(wr)
    r = wr / d.reshape(-1, *([1] * (wr.dim() - 1)))
    up = (r - torch.floor(r)) >= 0.5
    return q._unrows(torch.where(up, 1.0, -1.0).to(wr.dtype).contiguous(), w)


def report_unit(unit, unit_name, inp_q, out_fp, batch=32):
    """Measure what calibration gained on a trained unit: two passes over its cached quantised inputs `inp_q`, in the quant state the unit
    is found in (frozen static activation ranges included), each compared with the cached full-precision outputs `out_fp` per output
    channel by `ops.pair_moments(out_fp batch, output batch)` on channels-last storage:
      'nearest'   every trained weight (every AdaRoundQuantizer of the unit) rounded to nearest on the delta | zero point the quantiser
                  holds, clamp(floor(w / delta) + (frac >= 0.5) + z, 0, n_levels - 1) with frac = w / delta - floor(w / delta) in fp32: A
                  TIE ROUNDS UP (towards +inf), not to even as torch.round does.  Alpha is swapped for a tensor whose sign encodes frac >=
                  0.5 for the duration of the pass, then put back (the same Parameter objects) and the weight packs are dropped;
      'learned'   the unit as calibrated.
    The fp32 sums of the batches are added in float64 on the device; under data parallelism the two float64 [3, C] tensors are summed
    over the ranks ('nearest', then 'learned'), then the pixel count.  The result stays on the unit as `unit.unit_stats` = {"name", "n",
    "nearest": {"shift", "err", "energy"}, "learned": {...}} with float64 [C] CPU tensors (`export.unit_report` reads it).  Nothing else
    changes: alpha, delta, zero points, ranges, `act_stats` and every flag are left as they were found."""
    rstb = isinstance(unit, QuantRSTB)
    adas = [(m, m.weight_quantizer) for m in unit.modules()
            if isinstance(m, QuantModule) and isinstance(m.weight_quantizer, AdaRoundQuantizer)]

    def run():
        # (zero sums, not None: a rank with no rows still takes part in the collectives below)
        acc, n = torch.zeros(3, out_fp.shape[1], dtype=torch.float64, device=out_fp.device), 0
        with torch.no_grad():
            for i in range(0, inp_q.shape[0], batch):
                h = inp_q[i:i + batch]
                out = _nhwc(unit(h, (h.shape[2], h.shape[3])) if rstb else unit(h))
                ref = _nhwc(out_fp[i:i + batch])
                mom = ops.pair_moments(ref, out).double()
                acc = acc + mom
                n += ref.numel() // ref.shape[-1]
        return acc, n

    held = [(q, q.alpha) for _, q in adas]
    try:
        for m, q in adas:
            q.alpha = torch.nn.Parameter(_nearest_alpha(q, m.weight), requires_grad=q.alpha.requires_grad)
            m.drop_weight_pack()
        nearest, n = run()
    finally:
        for (m, _), (q, alpha) in zip(adas, held):
            q.alpha = alpha
            m.drop_weight_pack()
    learned, _ = run()
    if dp.world()[1] > 1:
        count = torch.tensor([n], dtype=torch.int64, device=nearest.device)
        dp.reduce_act_stats(sums=[nearest, learned, count])
        n = int(count.item())
    names = ("shift", "err", "energy")
    unit.unit_stats = {"name": unit_name, "n": int(n),
                       "nearest": {f: v for f, v in zip(names, nearest.cpu())},
                       "learned": {f: v for f, v in zip(names, learned.cpu())}}
    return unit.unit_stats


def _tap_layer(m):
    """-> (k, stride, pad, output_padding, transposed) of the conv, transposed-conv or Linear QuantModule `m`; what the forward refuses
    (dilated / grouped convolutions) is refused here, and a kernel that is not square"""
    if m.kind == "linear":
        return 1, 1, 0, 0, False
    kw = m.fwd_kwargs
    if m.kind == "conv":
        stride, pad = m.conv_geometry()
        op = 0
    else:
        if _sq(kw["dilation"]) != 1 or kw["groups"] != 1:
            raise NotImplementedError("dilated / grouped transposed convolutions are not on the supported path")
        stride, pad, op = _sq(kw["stride"]), _sq(kw["padding"]), _sq(kw["output_padding"])
    kh, kwid = int(m.org_weight.shape[2]), int(m.org_weight.shape[3])
    if kh != kwid:
        raise NotImplementedError(f"bias correction: a {kh} x {kwid} kernel is not square")
    return kh, stride, pad, op, m.kind == "tconv"


def _tap_call(m, x):
    """-> (channels-last input, k, stride, pad, (Ho, Wo) or None, transposed, output pixels) of one call of `m` on the input `x`"""
    k, stride, pad, op, tr = _tap_layer(m)
    if m.kind == "linear":
        t = x.contiguous()
        return t, 1, 1, 0, None, False, t.numel() // t.shape[-1]
    t = _nhwc(x)
    hw = (ops.tap_out_size(t.shape[1], k, stride, pad, tr, op), ops.tap_out_size(t.shape[2], k, stride, pad, tr, op))
    return t, k, stride, pad, hw, tr, t.shape[0] * hw[0] * hw[1]


class _TapCollector:
    """Forward pre-hooks on QuantModules that add up the tap sums of what each is fed: per module a float64 [k * k * Cin] device tensor
    (the fp32 sums of a call, `ops.tap_sums`, are added into it in float64 on the device), the output pixels seen, and the order of
    the first calls."""

    def __init__(self, mods, device, order_only=False):
        """order_only: the hooks note the order of the first calls and take no sums"""
        self.sums, self.n, self.order, self.device, self.order_only = {}, {}, [], device, order_only
        self.handles = [m.register_forward_pre_hook(self._hook) for m in mods]

    def _hook(self, m, args):
        if self.order_only:
            if m not in self.order:
                self.order.append(m)
            return
        t, k, stride, pad, hw, tr, n = _tap_call(m, args[0].detach())
        s32 = ops.tap_sums(t, k, stride, pad, hw, transposed=tr)
        if m not in self.sums:
            self.order.append(m)
            self.sums[m] = torch.zeros(s32.numel(), dtype=torch.float64, device=s32.device)
            self.n[m] = 0
        self.sums[m] += s32.reshape(-1).double()
        self.n[m] += int(n)

    def get(self, m):
        """(float64 sums, pixels) of `m`; zeros for a module no call reached (a rank without rows still joins the collectives)"""
        if m not in self.sums:
            k = 1 if m.kind == "linear" else int(m.org_weight.shape[2])
            cin = m.org_weight.shape[1] if m.kind != "tconv" else m.org_weight.shape[0]
            return torch.zeros(k * k * int(cin), dtype=torch.float64, device=self.device), 0
        return self.sums[m], self.n[m]

    def close(self):
        for h in self.handles:
            h.remove()
        self.handles = []


def _bias_rows(m, quantised):
    """the effective weight of `m` in one quant state as contiguous fp32 rows [O, k * k * Cin] in the `to_rows` order"""
    held = m.use_weight_quant
    try:
        m.use_weight_quant = bool(quantised)
        w = m._weights()[0].detach()
    finally:
        m.use_weight_quant = held
    rows = w if m.kind == "linear" else to_rows(w, tconv=m.kind == "tconv")
    return rows.reshape(rows.shape[0], -1).contiguous().float()


def correct_unit_bias(unit, unit_name, inp_q, inp_fp, out_fp, mode="weight", batch=32):
    """Empirical bias correction of a trained unit (Nagel et al. 2019): every conv, transposed-conv and Linear QuantModule of the unit
    that has a bias and weight quantisation on gets
        bias = float32(org_bias + (W_fp . S_ref - W_q . S_q) / n)
    with S = the tap sums of the layer's INPUT over the calibration set (`ops.tap_sums`: the sum over all n output pixels of the
    pre-activation of a weight W on that input is n b + W . S, exactly, so the pre-activation itself, which the fused kernels never
    write, is not needed), W_fp / W_q the full-precision / the hard-rounded weight in the `to_rows` order, and both products and their
    difference in float64 (`ops.bias_shift`).  S_q is taken on what the layer is fed in the quantised unit on `inp_q`; S_ref is
      mode 'weight':  S_q -- the mean error of the layer's own rounding is removed;
      mode 'output':  what the layer is fed in the full-precision unit on `inp_fp` -- the mean pre-activation becomes that of the target
                      the calibration reconstructed against.
    The bias is absolute from `org_bias`: correcting twice gives the same bits.  The layers are corrected one after the other in the
    order of their first call in the forward, each from a pass of its own over `inp_q`, so that a layer sees its corrected
    predecessors.  All passes run without a tape, batch for batch, the quantised ones with weight quantisation on and the unit's own
    activation quantisers OFF (in both activation modes: a static quantiser that is not frozen yet cannot run), the full-precision one
    in the (False, False) state; every flag is put back.  Before the first and after the last layer pass the unit output is compared
    with `out_fp` (`ops.pair_moments`).  GDN, LayerNorm and bias-less layers are left alone and listed with the reason.  Under data
    parallelism the tap sums, the pixel counts and the moments are summed over the ranks in the fixed layer order, so every rank
    writes the same biases.  Left behind: `m.bias_shift` (float64 [O], CPU) on every corrected layer and `unit.bias_stats`
    (`export.bias_report` reads it); `org_bias`, alpha, delta, zero points and ranges are not written."""
    if mode not in BIAS_CORRECT_MODES:
        raise ValueError(f"bias_correct must be 'weight' or 'output', got {mode!r}")
    rstb = isinstance(unit, QuantRSTB)
    names = {m: (n or "layer") for n, m in unit.named_modules() if isinstance(m, QuantModule)}
    mods = [m for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    states = [(m, m.use_weight_quant, m.use_act_quant) for m in mods]
    skipped, layers = OrderedDict(), []
    for m, name in names.items():
        if m.org_weight is None:
            continue                                     # (a PixelShuffle wrapper: nothing to correct, nothing to report)
        if m.kind in ("gdn", "layernorm"):
            skipped[name] = f"{m.kind}: its output mean is not linear in the mean of its input"
        elif m.bias is None or m.org_bias is None:
            skipped[name] = "no bias"
        elif not m.use_weight_quant:
            skipped[name] = "weight quantisation off"
        else:
            _tap_layer(m)                     # (raises for a geometry off the supported path, before any pass)
            layers.append(m)
    device = out_fp.device
    world_size = dp.world()[1]

    def run(x, moments=False):
        # (zero sums, not None: a rank with no rows still takes part in the collectives below)
        acc, n = torch.zeros(3, out_fp.shape[1], dtype=torch.float64, device=device), 0
        with torch.no_grad():
            for i in range(0, x.shape[0], batch):
                h = x[i:i + batch]
                out = unit(h, (h.shape[2], h.shape[3])) if rstb else unit(h)
                if moments:
                    ref = _nhwc(out_fp[i:i + batch])
                    acc = acc + ops.pair_moments(ref, _nhwc(out)).double()
                    n += ref.numel() // ref.shape[-1]
        return acc, n

    def set_state(w, a_):
        for m in mods:
            m.use_weight_quant, m.use_act_quant = w, a_

    ref_sums = {}
    try:
        # the full-precision pass ('output'), or a first quantised pass ('weight'), also fixes the order of the layers' first calls
        col = _TapCollector(layers, device, order_only=mode != "output")
        try:
            set_state(mode != "output", False)
            if mode == "output":
                run(inp_fp)                   # every S_ref in one pass
                col.close()
                set_state(True, False)
            before, n_out = run(inp_q, moments=True)
        finally:
            col.close()
        order = list(col.order) + [m for m in layers if m not in col.order]         # (no rows here: module order)
        if world_size > 1:
            # ranks with rows all saw the same order; a rank without rows takes theirs (MAX over the ranks of each layer's position)
            pos = torch.full((max(1, len(layers)),), -1, dtype=torch.int32, device=device)
            for i, m in enumerate(col.order):
                pos[layers.index(m)] = i
            dp.reduce_max(pos)
            got = pos[:len(layers)].tolist()
            if all(v >= 0 for v in got):
                order = [m for _, m in sorted(zip(got, layers), key=lambda t: t[0])]
        if mode == "output":
            for m in order:
                ref_sums[m] = col.get(m)[0]
            if world_size > 1 and order:
                dp.reduce_act_stats(sums=[ref_sums[m] for m in order])
        shifts = OrderedDict()
        for m in order:
            one = _TapCollector([m], device)
            try:
                run(inp_q)
            finally:
                one.close()
            s_q, n = one.get(m)
            if world_size > 1:
                count = torch.tensor([n], dtype=torch.int64, device=device)
                dp.reduce_act_stats(sums=[s_q, count])
                n = int(count.item())
            if n < 1:
                raise ValueError(f"correct_unit_bias: {unit_name}: no calibration rows reached {names[m]}")
            w_q = _bias_rows(m, True)
            w_ref = _bias_rows(m, False)
            shift, bias = ops.bias_shift(w_ref, w_q, ref_sums[m] if mode == "output" else s_q, s_q, n, m.org_bias.detach().float().contiguous())
            m.bias.data.copy_(bias)
            m.drop_weight_pack()              # (the memo keys on _version, which a .data write does not bump)
            m.bias_shift = shift.cpu()
            shifts[names[m]] = {"shift": m.bias_shift.clone(), "n": int(n), "kind": m.kind}
        after, _ = run(inp_q, moments=True)
        if world_size > 1:
            count = torch.tensor([n_out], dtype=torch.int64, device=device)
            dp.reduce_act_stats(sums=[before, after, count])
            n_out = int(count.item())
    finally:
        for m, w, a_ in states:
            m.use_weight_quant, m.use_act_quant = w, a_
    fields = ("shift", "err", "energy")
    unit.bias_stats = {"name": unit_name, "mode": mode, "n": int(n_out), "layers": shifts, "skipped": skipped,
                       "before": {f: v for f, v in zip(fields, before.cpu())}, "after": {f: v for f, v in zip(fields, after.cpu())}}
    return unit.bias_stats


def learn_act_ranges(unit, inp_q, out_fp, iters=500, lr=1e-3, batch=32, seed=0, idx_table=None):
    """Train the frozen static activation ranges of a calibrated unit on its reconstruction error (the activation-grid step of BRECQ /
    QDrop, after the rounding has been learned).  The unit runs in the W8A8 state with its hard-rounded weights under torch's tape (the
    modules' tape forwards; every frozen quantiser as `ActQuantStaticFn`, straight-through round) on mini-batches inp_q[idx] of `batch`
    rows (never a ragged one; idx from a generator seeded with `seed`, or the rows of `idx_table` [iters, batch]); the loss is
    lp_loss(out, out_fp[idx], p=2); every site range the forward reached takes one projected Adam step per iteration
    (`ops.act_range_step`: step size relative to the observed width, the range stays inside the observed max range).  Under data
    parallelism the range gradients of all sites, concatenated in the fixed site order of `calibrate_act_ranges`, are summed over the
    ranks and divided by the world size before the step, so every rank holds the same grids.  The quantisers end frozen; every quant
    state flag is left as it was found."""
    from hipops.autograd import SqDiffSumFn
    if _is_rstb(unit):
        raise NotImplementedError("learn_act_ranges: a Swin (RSTB) unit's activation-quantised window attention cannot sit on torch's tape "
                                  "(quant_block.QuantWindowAttention); use act_range='max' or 'l2' for it")
    iters, lr = _check_learn(iters, lr)
    mods = [m for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    quants = list({id(m.act_quantizer): m.act_quantizer for m in mods if m.act_quantizer.act_frozen()}.values())
    states = [(m, m.use_weight_quant, m.use_act_quant) for m in mods]
    n = inp_q.shape[0]
    B = max(1, min(int(batch), n))
    if idx_table is None:
        g = torch.Generator().manual_seed(int(seed))
        idx_table = torch.stack([torch.randperm(n, generator=g)[:B] for _ in range(iters)])
    if idx_table.dim() != 2 or idx_table.shape[0] < iters:
        raise ValueError(f"learn_act_ranges: idx_table must be [iters >= {iters}, batch], got {tuple(idx_table.shape)}")
    idx_table = idx_table.to(device=inp_q.device, dtype=torch.long)
    world_size = dp.world()[1]
    try:
        for m in mods:
            m.use_weight_quant = m.use_act_quant = True
        for q in quants:
            q.act_learn()
        sites = [(q, k) for q in quants for k in sorted(q.act_range)]          # in a fixed order: the collectives of all ranks must line up
        moments = [(torch.zeros_like(q.act_obs[k]), torch.zeros_like(q.act_obs[k])) for q, k in sites]
        steps = [0] * len(sites)
        for it in range(iters):
            idx = idx_table[it]
            x = inp_q.index_select(0, idx).detach().requires_grad_(True)
            tgt = out_fp.index_select(0, idx)
            with torch.enable_grad():
                out = unit(x)
                loss = SqDiffSumFn.apply(out, tgt, float(out.shape[1]) / out.numel())      # = lp_loss(out, tgt, p=2)
                grads = torch.autograd.grad(loss, [q.act_range[k] for q, k in sites], allow_unused=True)
            if world_size > 1:
                flat = torch.cat([torch.zeros_like(q.act_obs[k]) if g_ is None else g_ for (q, k), g_ in zip(sites, grads)])
                dp.reduce_act_grads(flat)
                grads = [None if g_ is None else f for g_, f in zip(grads, flat.split([q.act_obs[k].numel() for q, k in sites]))]
            for i, ((q, k), g_) in enumerate(zip(sites, grads)):
                if g_ is None:                        # a site this forward did not reach
                    continue
                steps[i] += 1
                ops.act_range_step(q.act_range[k], g_.contiguous(), q.act_obs[k], moments[i][0], moments[i][1], steps[i], lr)
    finally:
        for q in quants:
            if getattr(q, "act_phase", "idle") == "learn":
                q.act_freeze()
            else:
                q.act_obs = {}
        for m, w, a_ in states:
            m.use_weight_quant, m.use_act_quant = w, a_


def reconstruct(model, unit, unit_name, cali_data, *a, **kw):
    """`_reconstruct` with the cross-unit state tidied up: the full-precision cache memo of the schedule
    (quantization/utils.py::_FpMemo) is dropped when a unit raises, so a schedule that dies half-way pins no device memory; and the
    quantisers that `_reconstruct` put on torch's tape for the unit (`act_ste`: loss_mode='rd' behind frozen activation quantisers) are
    taken off it again, whatever happened."""
    ste = []
    try:
        return _reconstruct(model, unit, unit_name, cali_data, *a, _ste=ste, **kw)
    except BaseException:
        from .utils import _FpMemo
        _FpMemo.clear()
        raise
    finally:
        for q in ste:
            q.act_ste = False


def _reconstruct(model, unit, unit_name, cali_data, batch_size=32, iters=20000, weight=0.01, opt_mode="mse", asym=False,
                 include_act_func=True, b_range=(20, 2), warmup=0.0, input_prob=1.0, act_quant=False, lr=4e-5, p=2.0,
                 config=None, args=None, is_block=False, _ste=None):
    if opt_mode != "mse":
        # The reference cannot run these modes on a compression model either: its LossFunction returns None for them whenever a coder
        # tail output is passed (layer_opt.py:146-151, always the case in its loops, so `err.backward()` fails), and GetLayerGrad feeds
        # the model's output DICT to log_softmax / kl_div (utils.py:316-321: BRECQ's classification code).
        raise NotImplementedError(f"opt_mode={opt_mode!r}: only 'mse' (the mode main2.py uses) is built -- the Fisher-weighted modes of the "
                                  "reference are classification left-overs that do not run on its compression models")
    task_p = getattr(args, "task_loss", 2.0) if args is not None else 2.0
    if float(p) != 2.0:
        raise NotImplementedError("rec_loss is built for p = 2 (the value main2.py passes); --task_loss may be any exponent >= 1")
    if float(task_p) < 1.0:
        raise ValueError("--task_loss < 1 has no finite gradient at zero error")
    rd_metric = _rd_metric(args, cali_data)
    act_mode, act_range = _act_args(args)
    act_iters, act_lr = _act_learn_args(args)
    act_percentile = _act_percentile_args(args)
    act_report = _act_report_args(args)
    unit_report = _unit_report_args(args)
    bias_correct = _bias_correct_args(args)
    if act_quant and act_mode == "static" and act_range == "learned" and _is_rstb(unit):
        raise NotImplementedError("act_range='learned': a Swin (RSTB) unit's activation-quantised window attention cannot sit on torch's "
                                  "tape (quant_block.QuantWindowAttention); calibrate it with act_range='max' or 'l2'")
    rank, world_size = dp.world()
    if world_size > 1:                      # data parallel: this rank calibrates on its shard with its share of the batch
        if batch_size % world_size != 0:
            raise ValueError(f"data-parallel calibration: batch_size {batch_size} is not a multiple of the world size "
                             f"{world_size} (the global mini-batch is split evenly; pass a multiple, e.g. {world_size * max(1, batch_size // world_size)})")
        if cali_data.size(0) % world_size != 0:
            raise ValueError(f"data-parallel calibration: {cali_data.size(0)} calibration images do not split evenly over "
                             f"{world_size} ranks (uneven shards would weight samples unequally)")
        cali_data = dp.shard(cali_data)
        batch_size = batch_size // world_size
    # args.timing (optional list): the caller wants this unit's wall split -- cache building / plan recording / loop -- which costs
    # three device synchronisations (tools/full_schedule.py, bench.py's recon_model_wall_s)
    timing = getattr(args, "timing", None) if args is not None else None

    def _mark():
        if timing is not None:
            torch.cuda.synchronize()
        return time.time()
    t0 = _mark()
    # dynamic activation quantisation makes cached values depend on the caching batch: keep the reference's batch of 1 then (a static
    # grid is the same whatever shares the batch)
    static_act = bool(act_quant) and act_mode == "static"
    if act_quant:
        # args decide, in both directions: a model calibrated static earlier and reconstructed again with act_mode='dynamic' (or without
        # it) runs dynamic grids; frozen ranges stay on the quantisers and come back with QuantModel.set_act_mode('static')
        for m in model.modules():
            if isinstance(m, (QuantModule, BaseQuantBlock)) and getattr(m.act_quantizer, "act_mode", "dynamic") != act_mode:
                m.act_quantizer.set_act_mode(act_mode)
    if static_act and getattr(args, "loss_mode", "lp") == "rd" and _ste is not None:
        # the R + lambda*D task loss differentiates through the trained modules behind the unit: their frozen quantisers go on torch's tape
        # (straight-through round) for the duration of this unit; `reconstruct` clears the flag.  The cache passes run without a tape.
        for m in model.modules():
            if isinstance(m, (QuantModule, BaseQuantBlock)) and m.act_quantizer.act_frozen() and not getattr(m.act_quantizer, "act_ste", False):
                m.act_quantizer.act_ste = True
                _ste.append(m.act_quantizer)
    cache_bs = 1 if (act_quant and not static_act) else max(1, min(32, cali_data.size(0)))
    (inp_q, inp_fp), out_fp = save_inp_oup_data(model, unit, cali_data, asym, act_quant, batch_size=cache_bs, input_prob=True)
    t1 = _mark()
    logging.info("Cached init time: {}".format(t1 - t0))
    module_list, name_list = find_unquantized_module(model, unit_name, [], [])
    logging.info(name_list)
    # Lu2022 naming (g_a0 ... g_s7): the task term runs through the untrained rest of the sub-coder, and through round_ste for
    # analysis-transform units (layer_opt.py:45-75); its target is the same function of the cached FP outputs (:262-263)
    tail_round = "g_a" in unit_name
    task_cache = None
    model.set_quant_state(False, False)
    rd_mode = getattr(args, "loss_mode", "lp") == "rd"
    if (module_list or tail_round) and not rd_mode:          # (the R + lambda*D task term does not use the lp target)
        task_cache = _nhwc(fp_out(module_list, out_fp, tail_round))
    set_mode(model, act_quant)
    if not is_block and ("g_s7" in unit_name or "7" in unit_name):
        logging.info("=======last layer, close activation quantization=======")
        unit.set_quant_state(True, False)
    else:
        unit.set_quant_state(True, act_quant)
    if not is_block and unit.org_weight is None:
        return None                                   # PixelShuffle units carry nothing to train (layer_opt.py:245-246)
    kind, mods = _unit_modules(unit)
    # opt-in task loss: the R + lambda*D loss of the whole model that the reference sketches and comments out
    # (layer_opt.py:146-148).  args.loss_mode = 'rd' (default 'lp' = the reference's lp_loss pair)
    rd = None
    if getattr(args, "loss_mode", "lp") == "rd":
        rd = dict(model=model, unit=unit, cali=cali_data.to(next(model.parameters()).device), lmbda=float(getattr(args, "lmbda", 0.01)),
                  metric=rd_metric)
    elif getattr(args, "loss_mode", "lp") != "lp":
        raise ValueError(f"unknown loss_mode {args.loss_mode!r} ('lp' or 'rd')")
    # the CLI --lr is ignored by the reference (Adam default 1e-3, layer_opt.py:253-254); kept that way.
    common = dict(batch_size=batch_size, iters=iters, weight=weight, b_range=b_range, warmup=warmup, input_prob=input_prob,
                  lr=1e-3, seed=unit_seed(unit_name), include_act_func=include_act_func, batch_offset=rank * batch_size,
                  task_p=float(task_p))
    if rd is not None:
        # The rate-distortion task term replaces the lp term through the rest of the sub-coder: the whole wrapped model behind the unit
        # runs under torch's tape (hipops.autograd; Swin blocks included), so the Lu2022 units need no recorded FP tail here
        common["rd"] = rd
        if kind == "rstb":
            eng = TapeEngine(kind, mods, _nhwc(inp_q), _nhwc(inp_fp), _nhwc(out_fp), **common)
        else:
            eng = UnitEngine(kind, mods, _nhwc(inp_q), _nhwc(inp_fp), _nhwc(out_fp), **common)
    elif kind == "rstb" or task_cache is not None:
        eng = TapeEngine(kind, mods, _nhwc(inp_q), _nhwc(inp_fp), _nhwc(out_fp), tail=module_list, tail_round=tail_round,
                         task_cache=task_cache, **common)
    else:
        eng = UnitEngine(kind, mods, _nhwc(inp_q), _nhwc(inp_fp), _nhwc(out_fp), **common)
    eng.prepare()                # graph capture belongs to the set-up ("recording + graph capture" of the timing split), not to the loop
    t2 = _mark()
    # the next unit's index table is drawn while this unit's loop runs on the GPU (engine.IdxStream: adopted only if the next request
    # matches and nobody touched the CPU generator in between)
    from .engine import IdxStream
    IdxStream.begin(eng.cq.shape[0], eng.B, eng.iters)
    per_turn = max(256, eng.iters // 12)
    eng.run(idle=lambda: IdxStream.step(per_turn))
    t3 = _mark()
    if timing is not None:
        timing.append(dict(unit=unit_name, kind=kind, cache_s=t1 - t0, record_s=t2 - t1, loop_s=t3 - t2))
    # rank-invariant from here on: the overflow verdict of the unit (a MAX all-reduce under data parallelism) is formed ONCE, here, on
    # every rank; `logs_terms` is a collective as well when world > 1 (mean of the ranks' data terms), so with several ranks every rank
    # computes the log rows whether or not its own logger prints them -- the log level may differ from rank to rank, the sequence of
    # collectives must not
    eng.sync_overflow()
    want_log = logging.getLogger().isEnabledFor(logging.INFO)
    if iters >= 500 and (want_log or world_size > 1):
        rec, task, rd, b = eng.logs_terms()
        for c in (range(500, iters + 1, 500) if want_log else ()):
            logging.info("Total loss:\t{:.3f} ( task:{:.3f}, rec:{:.3f}, round:{:.3f})\tb={:.2f}\tcount={}".format(
                float(rec[c - 1] + task[c - 1] + rd[c - 1]), float(task[c - 1]), float(rec[c - 1]), float(rd[c - 1]),
                float(b[c - 1]), c))
    eng.finish()
    for m in ([unit] if not is_block else unit.modules()):
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.trained = True
    if bias_correct is not None:
        # before the static ranges are fixed: they are then observed on the corrected outputs
        t6 = _mark()
        correct_unit_bias(unit, unit_name, inp_q, inp_fp, out_fp, bias_correct, batch=cache_bs)
        if timing is not None:
            timing[-1]["bias_s"] = _mark() - t6
    if static_act:
        # only now does the unit apply its own activation quantisers (`trained`): fix their grids on what the unit will be fed.  Also for
        # a unit the reference's "last layer" rule above trained without activation quantisation: that rule matches every layer unit whose
        # name holds a '7' (g_a[7] of Cheng2020-attn, convs inside its attention blocks), and the cache passes of later units and the
        # W8A8 evaluation apply those quantisers all the same (utils.set_mode).  What decides is whether a later forward applies the
        # quantiser: one behind `disable_act_quant` is never called, observes nothing and stays without a range.
        t4 = _mark()
        if act_range == "learned":
            calibrate_act_ranges(unit, inp_q, "l2", batch=cache_bs, keep_obs=True)         # the starting ranges
            learn_act_ranges(unit, inp_q, out_fp, act_iters, act_lr, batch_size, seed=unit_seed(unit_name))
        else:
            calibrate_act_ranges(unit, inp_q, act_range, batch=cache_bs, percentile=act_percentile)
        if act_report:
            report_act_ranges(unit, inp_q, batch=cache_bs)
        if timing is not None:
            timing[-1]["act_s"] = _mark() - t4
    if unit_report:
        t5 = _mark()
        report_unit(unit, unit_name, inp_q, out_fp, batch=cache_bs)
        if timing is not None:
            timing[-1]["report_s"] = _mark() - t5
    return eng
