"""Shared body of `layer_reconstruction` / `block_reconstruction` (reference: layer_opt.py:175-320, block_opt.py:176-324).

The choreography around the hot loop is the reference's; the loop itself runs on `engine.UnitEngine`.  What runs on a unit after its
loop, which the reference does not have (activation ranges, reports, bias correction), is in `unit_passes`; its argument checks are here."""
import logging
import time
import types
import zlib

import torch

from . import dp
from hipops import ops
from .engine import UnitEngine
from .quant_block import BaseQuantBlock
from .swin_engine import TapeEngine
from .quant_layer import QuantModule, _nhwc
from .unit_passes import (BIAS_CORRECT_MODES, SWIN_LEARN_REFUSAL, _check_learn, _check_percentile, _is_rstb, calibrate_act_ranges,
                          correct_unit_bias, learn_act_ranges, report_act_ranges, report_unit)
from .unit_passes import _TapCollector, _bias_rows, _nearest_alpha, _reduce_scores, _tap_call, _tap_layer  # noqa: F401  (importable from here as before)
from .utils import LinearTempDecay, save_inp_oup_data, set_mode

_COOPS = ("g_a", "h_a", "h_s", "g_s")


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


def _arg(args, name, default):
    """args.name; `default` where `args` is None or does not carry it"""
    return getattr(args, name, default) if args is not None else default


def _rd_metric(args, cali_data):
    """args.rd_metric: the distortion of the loss_mode='rd' task term, 'mse' (default) or 'ms-ssim' (the objective of CompressAI's
    MS-SSIM checkpoints).  Not `args.metric`: LossFunction.metric is the --task_loss exponent.  Checked before any work is done:
    the five MS-SSIM scales of an 11-tap window need crops with both sides above 160 pixels."""
    metric = _arg(args, "rd_metric", "mse")
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
    width; a Swin (RSTB) unit only with args.act_learn_swin=True, default False, a bool) or 'percentile' (a second pass takes a
    1024-bin histogram of every channel on its observed range; each end then gives up whole
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
    opt = _pass_options(args)
    return opt.act_mode, opt.act_range


def _pass_options(args):
    """Every option `_act_args` describes, read and validated once, a bad one reported in this order -> a namespace of act_mode,
    act_range, act_iters, act_lr, act_learn_swin, act_percentile, act_report, unit_report and bias_correct."""
    mode, how = _arg(args, "act_mode", "dynamic"), _arg(args, "act_range", "max")
    if mode not in ("dynamic", "static"):
        raise ValueError(f"unknown act_mode {mode!r} ('dynamic' or 'static')")
    if how not in ("max", "l2", "learned", "percentile", "hist_mse", "auto"):
        raise ValueError(f"unknown act_range {how!r} ('max', 'l2', 'learned', 'percentile', 'hist_mse' or 'auto')")
    iters, lr = _act_learn_args(args)
    return types.SimpleNamespace(act_mode=mode, act_range=how, act_iters=iters, act_lr=lr, act_percentile=_act_percentile_args(args),
                                 act_report=_act_report_args(args), act_learn_swin=_bool_arg(args, "act_learn_swin"),
                                 unit_report=_unit_report_args(args), bias_correct=_bias_correct_args(args))


def _bool_arg(args, name):
    flag = _arg(args, name, False)
    if not isinstance(flag, bool):
        raise ValueError(f"{name} must be True or False, got {flag!r}")
    return flag


def _act_report_args(args):
    """args.act_report, validated: a bool (default False)."""
    return _bool_arg(args, "act_report")


def _unit_report_args(args):
    """args.unit_report, validated: a bool (default False)."""
    return _bool_arg(args, "unit_report")


def _bias_correct_args(args):
    """args.bias_correct, validated -> None (off: absent, None or False, the default), 'weight' or 'output'.  True is refused like every
    other value: the mode must be named."""
    mode = _arg(args, "bias_correct", None)
    if mode is None or mode is False:
        return None
    if not isinstance(mode, str) or mode not in BIAS_CORRECT_MODES:
        raise ValueError(f"bias_correct must be 'weight', 'output' or off (None / False), got {mode!r}")
    return mode


def _act_learn_args(args):
    """(args.act_iters, args.act_lr) of act_range='learned', validated: a positive whole number of steps, a positive finite step size."""
    return _check_learn(_arg(args, "act_iters", 500), _arg(args, "act_lr", 1e-3))


def _act_percentile_args(args):
    """args.act_percentile of act_range='percentile', validated: a real number p with 50 < p <= 100 (100 = the max range)."""
    return _check_percentile(_arg(args, "act_percentile", 99.99))


def _check_mx_learned(unit, named, args):
    """A unit whose weighted modules hold `mx.MXAdaRoundQuantizer`s runs on the per-op MX step of the engine: all of them must hold one,
    and what that first version does not serve is refused (NotImplementedError naming the option) before any cache is built."""
    from .mx import is_mx_learned
    weighted = [(n, m) for n, m in named if isinstance(m, QuantModule) and m.org_weight is not None]
    learned = [n for n, m in weighted if is_mx_learned(m.weight_quantizer)]
    if not learned:
        return
    what = "reconstruct: learned rounding on MX grids"
    other = [n for n, m in weighted if not is_mx_learned(m.weight_quantizer)]
    if other:
        raise NotImplementedError(f"{what}: module {other[0]!r} holds an integer-grid quantiser next to the MXAdaRoundQuantizer of module "
                                  f"{learned[0]!r}: a unit is calibrated on one kind of grid (set_weight_format names whole units)")
    if _is_rstb(unit):
        raise NotImplementedError(f"{what} is not built for RSTB / Swin units (unit of module {learned[0]!r})")
    if dp.world()[1] > 1:
        raise NotImplementedError(f"{what} is not built for data-parallel calibration (world_size > 1)")
    if _arg(args, "loss_mode", "lp") == "rd":
        raise NotImplementedError(f"{what} is not built for loss_mode='rd'")
    if _arg(args, "bias_correct", None) not in (None, False):
        raise NotImplementedError(f"{what}: args.bias_correct is not built for it (the correction reads an integer grid)")
    if _arg(args, "unit_report", False):
        raise NotImplementedError(f"{what}: args.unit_report is not built for it (the report re-rounds an integer grid to nearest)")


def reconstruct(model, unit, unit_name, cali_data, *a, **kw):
    """`_reconstruct` with the cross-unit state tidied up: the full-precision cache memo of the schedule
    (quantization/utils.py::_FpMemo) is dropped when a unit raises, so a schedule that dies half-way pins no device memory; and the
    quantisers that `_reconstruct` put on torch's tape for the unit (`act_ste`: loss_mode='rd' behind frozen activation quantisers) are
    taken off it again, whatever happened.  A unit that holds an `MXQuantizer` is refused (NotImplementedError) before any cache is
    built; one whose weighted modules all hold an `MXAdaRoundQuantizer` is calibrated on its MX grid (`_check_mx_learned` has what that
    path refuses).  A model in which any module runs on MX activations (`QuantModel.set_mx_activations`) is refused the same way."""
    from .mx import refuse_mx, refuse_mx_activations
    refuse_mx_activations("reconstruct", model.named_modules() if isinstance(model, torch.nn.Module) else (),
                          "calibration under MX activations is not built (QuantModel.set_mx_activations(None) switches them off)")
    inside = unit.named_modules() if isinstance(unit, torch.nn.Module) else ()
    named = [(f"{unit_name}.{n}" if n else unit_name, m) for n, m in inside]
    refuse_mx("reconstruct", named, NotImplementedError,
              "learned rounding on MX grids is not built (QuantModel.set_weight_format('int') puts the integer grid back; "
              "set_weight_format(..., rounding='learned') installs the quantiser that this loop calibrates)", learned=False)
    _check_mx_learned(unit, named, kw.get("args", a[13] if len(a) > 13 else None))
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
    task_p = _arg(args, "task_loss", 2.0)
    if float(p) != 2.0:
        raise NotImplementedError("rec_loss is built for p = 2 (the value main2.py passes); --task_loss may be any exponent >= 1")
    if float(task_p) < 1.0:
        raise ValueError("--task_loss < 1 has no finite gradient at zero error")
    rd_metric = _rd_metric(args, cali_data)
    opt = _pass_options(args)
    if act_quant and opt.act_mode == "static" and opt.act_range == "learned" and _is_rstb(unit) and not opt.act_learn_swin:
        raise NotImplementedError(f"act_range='learned': {SWIN_LEARN_REFUSAL}")
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
    timing = _arg(args, "timing", None)

    def _mark():
        if timing is not None:
            torch.cuda.synchronize()
        return time.time()
    t0 = _mark()
    # dynamic activation quantisation makes cached values depend on the caching batch: keep the reference's batch of 1 then (a static
    # grid is the same whatever shares the batch)
    static_act = bool(act_quant) and opt.act_mode == "static"
    if act_quant:
        # args decide, in both directions: a model calibrated static earlier and reconstructed again with act_mode='dynamic' (or without
        # it) runs dynamic grids; frozen ranges stay on the quantisers and come back with QuantModel.set_act_mode('static')
        for m in model.modules():
            if isinstance(m, (QuantModule, BaseQuantBlock)) and getattr(m.act_quantizer, "act_mode", "dynamic") != opt.act_mode:
                m.act_quantizer.set_act_mode(opt.act_mode)
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
    if opt.bias_correct is not None:
        # before the static ranges are fixed: they are then observed on the corrected outputs
        t6 = _mark()
        correct_unit_bias(unit, unit_name, inp_q, inp_fp, out_fp, opt.bias_correct, batch=cache_bs)
        if timing is not None:
            timing[-1]["bias_s"] = _mark() - t6
    if static_act:
        # only now does the unit apply its own activation quantisers (`trained`): fix their grids on what the unit will be fed.  Also for
        # a unit the reference's "last layer" rule above trained without activation quantisation: that rule matches every layer unit whose
        # name holds a '7' (g_a[7] of Cheng2020-attn, convs inside its attention blocks), and the cache passes of later units and the
        # W8A8 evaluation apply those quantisers all the same (utils.set_mode).  What decides is whether a later forward applies the
        # quantiser: one behind `disable_act_quant` is never called, observes nothing and stays without a range.
        t4 = _mark()
        if opt.act_range == "learned":
            calibrate_act_ranges(unit, inp_q, "l2", batch=cache_bs, keep_obs=True)         # the starting ranges
            learn_act_ranges(unit, inp_q, out_fp, opt.act_iters, opt.act_lr, batch_size, seed=unit_seed(unit_name), swin=opt.act_learn_swin)
        else:
            calibrate_act_ranges(unit, inp_q, opt.act_range, batch=cache_bs, percentile=opt.act_percentile)
        if opt.act_report:
            report_act_ranges(unit, inp_q, batch=cache_bs)
        if timing is not None:
            timing[-1]["act_s"] = _mark() - t4
    if opt.unit_report:
        t5 = _mark()
        report_unit(unit, unit_name, inp_q, out_fp, batch=cache_bs)
        if timing is not None:
            timing[-1]["report_s"] = _mark() - t5
    return eng
