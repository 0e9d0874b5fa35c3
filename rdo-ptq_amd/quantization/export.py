"""True-integer export of a calibrated QuantModel (in the spirit of light-uniform-PTQ/quant_int/quant_layer.py:116-122,
which overwrites weights with uint8 levels): for every trained QuantModule the unsigned integer levels, the per-channel
scale `delta` and the zero point, such that  w_q = (levels - zero_point) * delta  is exactly the hard-rounded weight the
module uses at inference (`AdaRoundQuantizer.forward` with soft_targets=False, quantizer.py:441-449)."""
import math
from collections import OrderedDict

import torch

from .quant_block import BaseQuantBlock
from .quant_layer import QuantModule
from .quantizer import AdaRoundQuantizer
from .utils import quant_state


def integer_state(qnn) -> "OrderedDict[str, dict]":
    """name -> {levels (uint8, or int32 above 8 bits; logical weight shape), delta, zero_point, n_bits, bias, kind}.  `bias` is the one
    the quantised forward uses (`m.bias`): `org_bias` unless a bias correction moved it (`unit_passes.correct_unit_bias`)."""
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


def _moment_columns(row, st, states):
    """What `unit_report` and `bias_report` both derive from recorded pair moments `st[state]` with row["n"] pixels per channel, into the
    dicts the row already holds: row[f][state] for f = err | shift | energy | shift_share (float64 [C], CPU) and row["total"][f][state]
    for err | shift | energy (Python floats)."""
    for state in states:
        shift, err, energy = (st[state][f].detach().to("cpu", torch.float64).clone() for f in ("shift", "err", "energy"))
        row["err"][state], row["shift"][state], row["energy"][state] = err, shift, energy
        row["shift_share"][state] = torch.where(err == 0, torch.zeros_like(err), shift * shift / (max(row["n"], 1) * err))
        row["total"]["err"][state], row["total"]["shift"][state] = float(err.sum()), float(shift.sum())
        row["total"]["energy"][state] = float(energy.sum())


UNIT_REPORT_STATES = ("nearest", "learned")


def unit_report(qnn) -> "OrderedDict[str, dict]":
    """unit name -> the measured output error of every calibrated unit whose statistics were recorded (args.unit_report;
    `unit_passes.report_unit`), in module order, on the CPU.  With d = full-precision output - quantised output of the unit on its cached
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
        row = {"n": int(st["n"]), "total": {}}
        for f in ("err", "shift", "energy", "sqnr_db", "shift_share"):
            row[f] = {}
            if f in ("err", "shift", "energy", "sqnr_db"):
                row["total"][f] = {}
        _moment_columns(row, st, UNIT_REPORT_STATES)
        for state in UNIT_REPORT_STATES:
            err, energy = row["err"][state], row["energy"][state]
            row["sqnr_db"][state] = sqnr(energy, err)
            row["total"]["sqnr_db"][state] = float(sqnr(energy.sum(), err.sum()))
        row["channels"] = int(row["err"]["learned"].numel())
        row["gain_db"] = row["sqnr_db"]["learned"] - row["sqnr_db"]["nearest"]
        row["total"]["gain_db"] = row["total"]["sqnr_db"]["learned"] - row["total"]["sqnr_db"]["nearest"]
        out[str(st["name"])] = row
    return out


BIAS_REPORT_STATES = ("before", "after")


def bias_report(qnn) -> "OrderedDict[str, dict]":
    """unit name -> what the bias correction of every unit that ran it did (args.bias_correct; `unit_passes.correct_unit_bias`), in module
    order, on the CPU.  With d = full-precision output - quantised output of the unit on its cached calibration inputs (the unit's own
    activation quantisers off), per output channel, 'before' the first and 'after' the last layer was corrected:
      mode, channels, n              'weight' | 'output'; channel count; output pixels per channel (all ranks)
      err, shift, energy [state]     float64 [C]: sum d^2, sum d, sum of the squared full-precision output
      shift_share [state]            float64 [C]: shift^2 / (n err), 0 where err == 0 (as in `unit_report`)
      removed                        float64 [C]: err['before'] - err['after'], the squared error the correction took out
      layers                         layer name -> {shift (float64 [O]: bias - org_bias before the fp32 rounding), n (the layer's output
                                     pixels), kind, max_abs}, in the order the layers were corrected
      skipped                        layer name -> why it was left alone (GDN, LayerNorm, no bias, weight quantisation off)
      total                          {err, shift, energy, shift_share [state], removed}: the same over the summed channels (Python floats)
    Empty for a model without recorded statistics."""
    out = OrderedDict()
    for _, m in qnn.named_modules():
        st = getattr(m, "bias_stats", None)
        if not st:
            continue
        row = {"mode": str(st["mode"]), "n": int(st["n"]), "total": {}}
        for f in ("err", "shift", "energy", "shift_share"):
            row[f], row["total"][f] = {}, {}
        _moment_columns(row, st, BIAS_REPORT_STATES)
        for state in BIAS_REPORT_STATES:
            shift, e = row["shift"][state], row["total"]["err"][state]
            row["total"]["shift_share"][state] = 0.0 if e == 0 else float((shift * shift).sum()) / (max(row["n"], 1) * e)
        row["channels"] = int(row["err"]["after"].numel())
        row["removed"] = row["err"]["before"] - row["err"]["after"]
        row["total"]["removed"] = row["total"]["err"]["before"] - row["total"]["err"]["after"]
        row["layers"] = OrderedDict()
        for name, e in st["layers"].items():
            shift = e["shift"].detach().to("cpu", torch.float64).clone()
            row["layers"][str(name)] = {"shift": shift, "n": int(e["n"]), "kind": str(e["kind"]),
                                        "max_abs": float(shift.abs().max()) if shift.numel() else 0.0}
        row["skipped"] = OrderedDict((str(k), str(v)) for k, v in st["skipped"].items())
        out[str(st["name"])] = row
    return out


def _rd_report_args(qnn, images, lmbda, act_quant, batch, units, what="rd_report"):
    """every argument check of `rd_report` (and, under its own name, of `bit_report`), before any GPU work -> the selected (name, unit)
    pairs in `units()` order"""
    if not torch.is_tensor(images) or images.dtype != torch.float32:
        raise ValueError(f"{what}: images must be an fp32 tensor [n, 3, H, W], got "
                         f"{images.dtype if torch.is_tensor(images) else type(images).__name__}")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"{what}: images must be [n, 3, H, W], got {tuple(images.shape)}")
    if images.numel() == 0:
        raise ValueError(f"{what}: images is empty: {tuple(images.shape)}")
    if images.shape[2] % 64 or images.shape[3] % 64:
        raise ValueError(f"{what}: the image sides must be multiples of 64 (the calibration crops; nothing is padded), got "
                         f"{tuple(images.shape[2:])}")
    if isinstance(lmbda, bool) or not isinstance(lmbda, (int, float)) or not math.isfinite(lmbda) or lmbda <= 0:
        raise ValueError(f"{what}: lmbda must be a positive finite number, got {lmbda!r}")
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise ValueError(f"{what}: batch must be an integer >= 1, got {batch!r}")
    if not isinstance(act_quant, bool):
        raise ValueError(f"{what}: act_quant must be True or False, got {act_quant!r}")
    known = qnn.units()
    if units is None:
        return list(known.items())
    if isinstance(units, str) or not all(isinstance(u, str) for u in units):
        raise ValueError(f"{what}: units must be None or a list of unit names, got {units!r}")
    unknown = [u for u in units if u not in known]
    if unknown:
        raise ValueError(f"{what}: unknown unit name(s) {unknown}; QuantModel.units() has {list(known)}")
    return [(n, u) for n, u in known.items() if n in set(units)]


def _dynamic_grids(qnn):
    """does an activation quantiser that a forward with act_quant=True applies (its module trained, not disabled) follow its own
    tensor's min | max?"""
    for _, m in qnn.named_modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)) and m.trained and not getattr(m, "disable_act_quant", False) \
                and getattr(m.act_quantizer, "act_mode", "dynamic") != "static":
            return True
    return False


class _StateRunner:
    """The state runner of `rd_report` and `bit_report`: passes over this rank's share of `images` in whatever state the model is in, the
    data-parallel reduction of the passes' float64 sums, and the rows made of them (the columns `rd_report` documents)."""

    def __init__(self, qnn, images, lmbda, bs, what):
        from . import dp
        self.qnn, self.lmbda, self.bs = qnn, lmbda, bs
        self.n, _, H, W = (int(v) for v in images.shape)
        self.pixels = self.n * H * W
        self.device = next(qnn.parameters()).device
        rank, self.world = dp.world()
        if self.n < self.world:
            raise ValueError(f"{what}: {self.n} image(s) for {self.world} ranks: every rank needs at least one")
        self.mine = images[rank::self.world]

    def measure(self):
        """one pass over this rank's images in the state the model is in -> (keys, float64 device sums [bits of every key | sse])"""
        from hipops import ops
        device, mine, bs = self.device, self.mine, self.bs
        keys, acc, sse = None, None, torch.zeros(1, dtype=torch.float64, device=device)
        with torch.no_grad():
            for i in range(0, mine.shape[0], bs):
                x = mine[i:i + bs].to(device).contiguous()
                out = self.qnn(x)
                liks = out["likelihoods"]
                if keys is None:
                    keys = list(liks)
                    acc = [torch.zeros(liks[k].shape[1], dtype=torch.float64, device=device) for k in keys]
                for a, k in zip(acc, keys):
                    a += ops.neg_log2_channel_sums(liks[k]).double()
                sse += ops.sq_diff_sum_ordered(out["x_hat"].contiguous(), x, 1.0, clamp01=True).double()
        return keys, acc, sse

    def reduce(self, states):
        """all-reduce (SUM) the sums of every measured state in place; nothing to do for one rank"""
        from . import dp
        if self.world <= 1:
            return
        flat = torch.cat([t for _, acc, sse in states for t in acc + [sse]])
        dp.reduce_act_stats(sums=[flat])
        off = 0
        for _, acc, sse in states:
            for t in acc + [sse]:
                t.copy_(flat[off:off + t.numel()])
                off += t.numel()

    def row(self, state):
        keys, acc, sse = state
        bits = OrderedDict((k, a.cpu()) for k, a in zip(keys, acc))
        total = float(sum(b.sum() for b in bits.values()))
        mse = float(sse) / (3 * self.pixels)
        r = OrderedDict(bits=bits, bits_total=total, sse=float(sse), bpp=total / self.pixels, mse=mse,
                        psnr_db=float("inf") if mse == 0 else -10.0 * math.log10(mse))
        r["loss"] = r["bpp"] + self.lmbda * 255.0 ** 2 * mse
        return r

    @staticmethod
    def against(r, fp):
        r["d_bits"] = OrderedDict((k, r["bits"][k] - fp["bits"][k]) for k in r["bits"])
        for f in ("bpp", "mse", "psnr_db", "loss"):
            r["d_" + f] = r[f] - fp[f]
        return r


def rd_report(qnn, images, lmbda=0.01, act_quant=False, batch=8, units=None) -> "OrderedDict":
    """What each reconstruction unit costs in rate and distortion, measured on `images` (fp32 [n, 3, H, W] in [0, 1] on any device,
    H and W multiples of 64: the calibration crops, nothing is padded) under torch.no_grad().  Every state runs over the same images:
      'fp'          qnn.set_quant_state(False, False)
      'all'         qnn.set_quant_state(True, act_quant): what the W8 / W8A8 evaluation runs (disable_act_quant, `trained` and the
                    bit-widths as they stand on the model)
      one per unit  qnn.set_quant_state(False, False); unit.set_quant_state(True, act_quant): only that unit quantised
    `units`: None for all of `qnn.units()`, or a list of its names (reported in `units()` order).  With P = n H W, per state:
      bits[k]       float64 [C_k] on the CPU for every key k of out["likelihoods"] in the model's order: each batch's likelihood tensor
                    goes once through `ops.neg_log2_channel_sums`, the fp32 results are added in float64 on the device
      bits_total    the float64 sum over the keys of the channel sums
      sse           sum of ops.sq_diff_sum_ordered(x_hat, x, 1.0, clamp01=True) of the batches, added in float64
      bpp, mse      bits_total / P, sse / (3 P)
      psnr_db       -10 log10(mse), inf where mse == 0: the PSNR of the POOLED error, not `evaluate_images`' mean of per-image PSNRs
      loss          bpp + lmbda 255^2 mse
    and on every row but 'fp' the differences against 'fp': d_bits[k], d_bpp, d_mse, d_psnr_db, d_loss.
    -> OrderedDict: 'fp', 'all', 'units' (name -> row), 'n', 'pixels' (= P), 'lmbda', 'act_quant', 'additivity' {'sum_units_d_loss',
    'all_d_loss'} (unit costs are NOT additive: the pair shows by how much), 'batch' (the batch used).

    Batch: with act_quant=True and an applied activation quantiser on a dynamic grid, a tensor's grid depends on what shares its batch;
    the batch is then 1 whatever `batch` says (the rule of the calibration's cache batch).
    State: every module's use_weight_quant | use_act_quant pair is recorded first and restored in a `finally`; alpha, delta, zero points,
    activation ranges, act_stats, unit_stats and `trained` are not written.  A weight quantiser that has never run initialises its scale
    on its first use here, as in any forward.
    Data parallel: with an initialised process group rank r takes the images r, r + world, ..., the float64 sums are all-reduced (SUM)
    and every rank returns the same report; 'n' and 'pixels' are global (the rule of `evaluate_images`); fewer images than ranks is refused.
    Cost: len(units) + 2 passes over `images` -- meant for the calibration crops, not for Kodak at full size.
    Raises ValueError before any GPU work for: images not fp32 4-D with 3 channels, empty, or sides not multiples of 64; lmbda not a
    positive finite number; batch not an integer >= 1; act_quant not a bool; an unknown unit name."""
    chosen = _rd_report_args(qnn, images, lmbda, act_quant, batch, units)
    bs = 1 if (act_quant and _dynamic_grids(qnn)) else batch
    run = _StateRunner(qnn, images, lmbda, bs, "rd_report")
    states = []
    with quant_state(qnn):
        qnn.set_quant_state(False, False)
        states.append(run.measure())
        qnn.set_quant_state(True, act_quant)
        states.append(run.measure())
        for _, u in chosen:
            qnn.set_quant_state(False, False)
            u.set_quant_state(True, act_quant)
            states.append(run.measure())
    run.reduce(states)
    fp = run.row(states[0])
    full = run.against(run.row(states[1]), fp)
    rows = OrderedDict((name, run.against(run.row(st), fp)) for (name, _), st in zip(chosen, states[2:]))
    rep = OrderedDict()
    rep["fp"], rep["all"], rep["units"] = fp, full, rows
    rep["n"], rep["pixels"], rep["lmbda"], rep["act_quant"] = run.n, run.pixels, float(lmbda), act_quant
    rep["additivity"] = {"sum_units_d_loss": float(sum(r["d_loss"] for r in rows.values())), "all_d_loss": full["d_loss"]}
    rep["batch"] = bs
    return rep


def weighted_modules(unit):
    """the QuantModules of a unit that hold a weight (pixel shuffles do not), in module order"""
    return [m for m in unit.modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def is_trained(m):
    """has this QuantModule been calibrated?  Its AdaRoundQuantizer's alpha belongs to the delta it was trained on: no other width fits it"""
    return bool(m.trained) or isinstance(m.weight_quantizer, AdaRoundQuantizer)


_QUANTIZER_FIELDS = ("n_bits", "n_levels", "delta", "zero_point", "inited")


def _width_grids(m, widths):
    """the grids of one weighted module at every width, scored by `ops.uaq_width_scan` -> (delta, zp fp32 [K, rows], err float64 [K, rows],
    energy float64 [rows]).  Plain asymmetric 'max': one min-max scan.  Any other scale_method: the quantiser's own
    `init_quantization_scale` after `bitwidth_refactor(b)` (the caller restores the width), scored by a scan in given mode."""
    from hipops import ops
    q = m.weight_quantizer
    w = m.weight.detach()
    wr = q._rows(w)
    flat = wr.reshape(wr.shape[0], -1)
    if "max" in q.scale_method and "scale" not in q.scale_method and not q.sym:
        return ops.uaq_width_scan(flat, widths)
    ds, zs = [], []
    for b in widths:
        q.bitwidth_refactor(b)
        d, z = q.init_quantization_scale(w, q.channel_wise)
        ds.append(d.reshape(-1).expand(flat.shape[0]))
        zs.append(z.reshape(-1).expand(flat.shape[0]))
    return ops.uaq_width_scan(flat, widths, torch.stack(ds).float().contiguous(), torch.stack(zs).float().contiguous())


def bit_report(qnn, images, widths=(4, 6, 8), lmbda=0.01, batch=8, units=None) -> "OrderedDict":
    """What each reconstruction unit costs in rate and distortion at each of several weight widths, measured on `images` like `rd_report`
    (its rules for `images`, `lmbda`, `batch` and `units`) under torch.no_grad(), BEFORE calibration: weights only (activation
    quantisation is off in every state), round to nearest.  The states, all over the same images:
      'fp'                    qnn.set_quant_state(False, False): the 'fp' state of `rd_report`
      one per (unit, width)   qnn.set_quant_state(False, False); unit.set_quant_state(True, False), with every weighted QuantModule of
                              the unit temporarily at width b: in `units()` order, the widths in the order given
    Grids: a weight quantiser with the plain asymmetric 'max' scale takes delta and zero point of all widths from ONE
    `ops.uaq_width_scan` of its weight (the bits of `uaq_init_minmax` at 2^b levels: what its own first forward at that width would
    set); any other scale_method takes them from its own `init_quantization_scale` after `bitwidth_refactor(b)`, and the scan scores them
    in given mode, so the weight columns always come from the kernel.
    -> OrderedDict:
      'fp'       the row of `rd_report`'s 'fp'
      'units'    name -> width -> row: the keys of an `rd_report` unit row (bits, bits_total, sse, bpp, mse, psnr_db, loss, d_bits, d_bpp,
                 d_mse, d_psnr_db, d_loss), and size_bits = b x the unit's weight elements, weight_err = the sum over the unit's modules
                 and rows of sum (w - wq)^2 in float64, weight_sqnr_db = 10 log10(sum energy / sum err) in float64 (inf at zero error)
      'weights'  name -> weight elements of the unit (its weighted QuantModules; biases are not counted)
      'widths' (list), 'n', 'pixels', 'lmbda', 'batch'
    State: the fields n_bits, n_levels, delta, zero_point and inited of every weight quantiser of the chosen units and every module's
    use_weight_quant | use_act_quant pair are recorded first and put back in a `finally` (the same objects, so the same bits);
    `drop_weight_pack()` runs at every switch and at the end; a quantiser that had not been initialised is left uninitialised.
    Data parallel: as `rd_report` (images sharded by rank, float64 sums all-reduced, every rank returns the same table); every rank
    scans the weights itself, which gives the same bits.
    Cost: len(units) * len(widths) + 1 passes over `images`.
    Raises ValueError before any GPU work for what `rd_report` refuses, for widths that are not a non-empty sequence of at most 8
    distinct whole numbers in 2 .. MAX_BITS, and for a chosen unit that holds a trained module (the table is taken before calibration)."""
    from hipops import ops
    from .quantizer import MAX_BITS, _scale_shape
    what = "bit_report"
    chosen = _rd_report_args(qnn, images, lmbda, False, batch, units, what=what)
    widths = ops.width_list(what, widths, MAX_BITS)
    mods = OrderedDict((name, weighted_modules(u)) for name, u in chosen)
    for name, ms in mods.items():
        if any(is_trained(m) for m in ms):
            raise ValueError(f"{what}: unit {name!r} holds a trained module: the table is taken before calibration")
    run = _StateRunner(qnn, images, lmbda, batch, what)
    held = [(m, {f: getattr(m.weight_quantizer, f) for f in _QUANTIZER_FIELDS}) for ms in mods.values() for m in ms]
    states, weight_cols = [], OrderedDict()
    try:
        with quant_state(qnn):
            grids = {}
            for name, ms in mods.items():
                grids[name] = [_width_grids(m, widths) for m in ms]
                err = torch.stack([g[2].sum(1) for g in grids[name]]).sum(0).cpu()            # float64 [K]
                energy = float(torch.stack([g[3].sum() for g in grids[name]]).sum())
                weight_cols[name] = (err, energy)
            qnn.set_quant_state(False, False)
            states.append(run.measure())
            for name, u in chosen:
                for k, b in enumerate(widths):
                    qnn.set_quant_state(False, False)
                    u.set_quant_state(True, False)
                    for m, (d, z, _, _) in zip(mods[name], grids[name]):
                        q = m.weight_quantizer
                        shape = _scale_shape(m.weight, q.tconv) if q.channel_wise else ()
                        q.bitwidth_refactor(b)
                        q.delta, q.zero_point, q.inited = d[k].reshape(shape), z[k].reshape(shape), True
                        m.drop_weight_pack()
                    states.append(run.measure())
    finally:
        for m, fields in held:
            for f, v in fields.items():
                setattr(m.weight_quantizer, f, v)
            m.drop_weight_pack()
    run.reduce(states)
    fp = run.row(states[0])
    rep = OrderedDict()
    rep["fp"], rep["units"], rep["weights"] = fp, OrderedDict(), OrderedDict()
    it = iter(states[1:])
    for name, _ in chosen:
        count = sum(int(m.weight.numel()) for m in mods[name])
        err, energy = weight_cols[name]
        rep["weights"][name] = count
        rep["units"][name] = OrderedDict()
        for k, b in enumerate(widths):
            r = run.against(run.row(next(it)), fp)
            e = float(err[k])
            r["size_bits"], r["weight_err"] = b * count, e
            r["weight_sqnr_db"] = float("inf") if e == 0 else 10.0 * math.log10(energy / e)
            rep["units"][name][b] = r
    rep["widths"], rep["n"], rep["pixels"], rep["lmbda"], rep["batch"] = list(widths), run.n, run.pixels, float(lmbda), batch
    return rep


def _hull(options):
    """options: [(width, size, cost)] of one unit -> its hull points in ascending size: the lower convex hull from the smallest size up to
    the least-cost point (among equal costs the smallest).  Going down the list from the end, the cost per bit saved rises from step to
    step; points on a chord are kept."""
    pts = sorted(options, key=lambda p: p[1])
    best = min(range(len(pts)), key=lambda i: (pts[i][2], pts[i][1]))
    hull = []
    for p in pts[:best + 1]:
        # q = hull[-1] lies above the chord hull[-2] -> p when stepping p -> q costs more per bit than q -> hull[-2]
        while len(hull) >= 2 and (hull[-1][2] - p[2]) / (p[1] - hull[-1][1]) > (hull[-2][2] - hull[-1][2]) / (hull[-1][1] - hull[-2][1]):
            hull.pop()
        hull.append(p)
    return hull


def allocate_bits(report, budget_bits=None, avg_bits=None, fixed=None) -> dict:
    """Choose one weight width per unit from a `bit_report` table under a size budget.  Pure host code.
    `budget_bits`: a whole number of weight bits, or `avg_bits`: a real number of bits per weight, the budget then being
    floor(avg_bits * sum of report['weights']); exactly one of the two.  `fixed`: name -> width, a unit that has that one option.
    The rule.  Each unit's options are the points (size_bits, d_loss) of its row.  Kept is the lower convex hull of the options from the
    smallest size up to the unit's least-cost point (among equal costs the smallest); larger widths that cost more are dropped.  Every
    unit starts at its least-cost hull point.  While the total size exceeds the budget, the hull step with the smallest slope is taken,
    slope = cost added / size saved in float64, ties to the earlier unit in `units()` order; the first total <= budget stops it.
    ValueError, naming the smallest reachable size, when even that exceeds the budget.
    -> {'bits': OrderedDict name -> width, 'size_bits', 'avg_bits' (size_bits / sum of weights), 'cost' (sum of the chosen d_loss, added
    in unit order), 'budget_bits', 'steps': [(unit, from width, to width, slope)] in the order taken}.
    Guaranteed: no assignment of total size <= the returned size_bits has a lower total cost.  (Hull steps taken in slope order visit
    the minimisers of cost + s * size for the rising step slope s >= 0 -- the Lagrangian property; an assignment A' with size' <= size
    has cost' >= cost + s (size - size') >= cost.  Before the first step s = 0: every unit sits at its least cost.)
    Not guaranteed: that no assignment BETWEEN the returned size and the budget costs less (the rule does not search the gap), and
    anything about the calibrated model: the table is round-to-nearest and its costs are not additive (`rd_report`'s 'additivity'); on
    random-init models the costs are noise of either sign."""
    what = "allocate_bits"
    try:
        table, weights = report["units"], report["weights"]
        names = list(table)
        opts = OrderedDict((n, [(b, table[n][b]["size_bits"], float(table[n][b]["d_loss"])) for b in table[n]]) for n in names)
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f"{what}: report must be a `bit_report` table ('units': name -> width -> row with size_bits and d_loss; "
                         f"'weights'): {e!r}")
    if not names or any(not o for o in opts.values()):
        raise ValueError(f"{what}: the table holds no unit, or a unit without a width")
    if list(weights) != names or any(isinstance(w, bool) or not isinstance(w, int) or w < 1 for w in weights.values()):
        raise ValueError(f"{what}: report['weights'] must give a positive element count for every unit of the table, in its order")
    for n, o in opts.items():
        for b, size, cost in o:
            if isinstance(size, bool) or not isinstance(size, int) or size < 1 or not math.isfinite(cost):
                raise ValueError(f"{what}: unit {n!r} at width {b}: size_bits {size!r} must be a positive whole number and d_loss {cost!r} finite")
        if len({size for _, size, _ in o}) != len(o):
            raise ValueError(f"{what}: unit {n!r} has two widths of the same size")
    total_w = sum(weights.values())
    if (budget_bits is None) == (avg_bits is None):
        raise ValueError(f"{what}: exactly one of budget_bits and avg_bits must be given")
    if budget_bits is not None:
        if isinstance(budget_bits, bool) or not isinstance(budget_bits, int) or budget_bits < 1:
            raise ValueError(f"{what}: budget_bits must be a whole number >= 1, got {budget_bits!r}")
        budget = int(budget_bits)
    else:
        if isinstance(avg_bits, bool) or not isinstance(avg_bits, (int, float)) or not math.isfinite(avg_bits) or avg_bits <= 0:
            raise ValueError(f"{what}: avg_bits must be a positive finite number, got {avg_bits!r}")
        budget = math.floor(avg_bits * total_w)
    fixed = {} if fixed is None else fixed
    if not isinstance(fixed, dict):
        raise ValueError(f"{what}: fixed must be None or a dict name -> width, got {fixed!r}")
    for n, b in fixed.items():
        if n not in opts:
            raise ValueError(f"{what}: fixed names the unknown unit {n!r}; the table has {names}")
        if isinstance(b, bool) or b not in table[n]:
            raise ValueError(f"{what}: fixed gives unit {n!r} the width {b!r}; the table has {list(table[n])}")
    hulls = [_hull([p for p in opts[n] if n not in fixed or p[0] == fixed[n]]) for n in names]
    least = sum(h[0][1] for h in hulls)
    if least > budget:
        raise ValueError(f"{what}: the smallest reachable size is {least} bits; the budget is {budget}")
    at = [len(h) - 1 for h in hulls]
    size = sum(h[i][1] for h, i in zip(hulls, at))
    steps = []
    while size > budget:
        pick, slope = None, None
        for u, (h, i) in enumerate(zip(hulls, at)):
            if i == 0:
                continue
            s = (h[i - 1][2] - h[i][2]) / (h[i][1] - h[i - 1][1])
            if pick is None or s < slope:
                pick, slope = u, s
        h, i = hulls[pick], at[pick]
        steps.append((names[pick], h[i][0], h[i - 1][0], slope))
        size -= h[i][1] - h[i - 1][1]
        at[pick] = i - 1
    cost = 0.0
    for h, i in zip(hulls, at):
        cost += h[i][2]
    return {"bits": OrderedDict((n, h[i][0]) for n, h, i in zip(names, hulls, at)), "size_bits": size, "avg_bits": size / total_w,
            "cost": cost, "budget_bits": budget, "steps": steps}


def act_modules(unit):
    """(name inside the unit, module) of every QuantModule / BaseQuantBlock of a unit, the unit itself included ('' is its name): the
    holders of the unit's activation quantisers, in module order"""
    return [(mn, m) for mn, m in unit.named_modules() if isinstance(m, (QuantModule, BaseQuantBlock))]


def act_applied(m):
    """does a forward with act_quant=True apply this module's activation quantiser?"""
    return bool(m.trained) and not getattr(m, "disable_act_quant", False)


def _distinct(quantisers):
    """de-duplicated by identity, in order"""
    seen, out = set(), []
    for q in quantisers:
        if id(q) not in seen:
            seen.add(id(q))
            out.append(q)
    return out


def _sqnr_db(energy, err):
    return torch.where(err == 0, torch.full_like(err, float("inf")), 10.0 * torch.log10(energy / err))


def _reduce_scans(scans):
    """all-reduce (SUM) the closed scan sums in place, in the fixed order of the list: scans = [[(site name, {err, energy, n})]] of every
    state; the counts travel as float64 (whole numbers far below 2^53).  Nothing to do for one rank."""
    from . import dp
    if dp.world()[1] <= 1:
        return
    rows = [st for state in scans for _, st in state]
    if not rows:
        return
    dev = rows[0]["err"].device
    flat = torch.cat([t for st in rows for t in (st["err"].reshape(-1), st["energy"], torch.tensor([st["n"]], dtype=torch.float64, device=dev))])
    dp.reduce_act_stats(sums=[flat])
    off = 0
    for st in rows:
        for f in ("err", "energy"):
            k = st[f].numel()
            st[f].copy_(flat[off:off + k].reshape(st[f].shape))
            off += k
        st["n"] = int(flat[off])
        off += 1


def _close_scans(named):
    """close the scan of every (name, quantiser) -> [(site name, sums)] in order; site names follow `QuantModel.act_ranges`"""
    out = []
    for name, q in named:
        sums = q.act_scan_close()
        for site in sorted(sums):
            out.append((name if site == 0 else f"{name}#{site}", sums[site]))
    return out


def act_width_report(qnn, images, widths=(4, 6, 8), batch=8) -> "OrderedDict":
    """The one-pass screening table of activation widths: what the grid of every applied activation quantiser costs the values it sees, at
    each of `widths`, measured on `images` (the rules of `rd_report` for `images` and `batch`) under torch.no_grad().  The model runs ONCE
    over the images in qnn.set_quant_state(True, True) -- `rd_report`'s 'all' state with act_quant=True: `trained`, `disable_act_quant`
    and the widths as they stand -- with a width scan open on every applied quantiser (`UniformAffineQuantizer.act_scan`,
    `ops.actquant_width_scan`: one read of each tensor for all K widths, where K passes of the scoring kernel would read it K times).
    What flows downstream is the model's own quantised activation at its own width; the scanned grid is the site's frozen range (static)
    or the tensor's own min | max (dynamic).
    -> OrderedDict:
      'sites'   site name (those of `QuantModel.act_ranges`: 'name', 'name#1') -> {unit (None outside `units()`), mode, n_bits (current),
                channels, n (values seen per channel), err float64 [K, C] = sum (x - Q_k(x))^2, energy float64 [C] = sum x^2, sqnr_db
                float64 [K, C] = 10 log10(energy / err) (inf at zero error), total {err float64 [K], energy, sqnr_db float64 [K]}: the same
                over the summed channels}, on the CPU
      'widths' (list), 'n' (images), 'batch' (the batch used: 1 when an applied quantiser is on a dynamic grid)
    Frozen ranges are used as they stand at every width: a 'hist_mse' / 'auto' range was chosen for the width it was calibrated at.
    State: the quant-state flags are recorded first and restored in a `finally`, where the scans are closed too; nothing else is written.
    Data parallel: as `rd_report`, the scan sums joining a float64 all-reduce in a fixed order.
    Raises ValueError before any GPU work for what `rd_report` refuses of images and batch and `ops.width_list` of widths."""
    from hipops import ops
    from .quantizer import MAX_BITS
    what = "act_width_report"
    _rd_report_args(qnn, images, 0.01, True, batch, None, what=what)
    widths = ops.width_list(what, widths, MAX_BITS)
    unit_of = {id(m): name for name, u in qnn.units().items() for _, m in act_modules(u)}
    named, meta, seen = [], {}, set()
    for name, m in qnn.named_modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)) and act_applied(m) and id(m.act_quantizer) not in seen:
            seen.add(id(m.act_quantizer))
            named.append((f"{name}.act_quantizer", m.act_quantizer))
            meta[f"{name}.act_quantizer"] = (unit_of.get(id(m)), m.act_quantizer)
    bs = 1 if _dynamic_grids(qnn) else batch
    run = _StateRunner(qnn, images, 0.01, bs, what)
    try:
        with quant_state(qnn):
            qnn.set_quant_state(True, True)
            for _, q in named:
                q.act_scan(widths)
            with torch.no_grad():
                for i in range(0, run.mine.shape[0], bs):
                    qnn(run.mine[i:i + bs].to(run.device).contiguous())
    finally:
        scans = _close_scans(named)
    _reduce_scans([scans])
    rep = OrderedDict()
    rep["sites"] = OrderedDict()
    for site, st in scans:
        unit, q = meta[site.split("#")[0]]
        err, energy = st["err"].cpu(), st["energy"].cpu()
        rep["sites"][site] = {"unit": unit, "mode": getattr(q, "act_mode", "dynamic"), "n_bits": int(getattr(q, "dynamic_bits", 8)),
                              "channels": int(energy.numel()), "n": int(st["n"]), "err": err, "energy": energy,
                              "sqnr_db": _sqnr_db(energy.unsqueeze(0), err),
                              "total": {"err": err.sum(1), "energy": float(energy.sum()), "sqnr_db": _sqnr_db(energy.sum(), err.sum(1))}}
    rep["widths"], rep["n"], rep["batch"] = list(widths), run.n, bs
    return rep


_MISSING = object()


def act_bit_report(qnn, images, widths=(4, 6, 8), lmbda=0.01, weight_quant=False, batch=8, units=None) -> "OrderedDict":
    """What each reconstruction unit costs in rate and distortion at each of several ACTIVATION widths, measured on `images` like
    `rd_report` (its rules for `images`, `lmbda`, `batch` and `units`) under torch.no_grad(), on a calibrated model: the sibling of
    `bit_report`.  The states, all over the same images:
      'fp'                    qnn.set_quant_state(False, False): the 'fp' state of `rd_report`
      one per (unit, width)   qnn.set_quant_state(False, False); set_quant_state(weight_quant, True) on the unit and on every
                              QuantModule / BaseQuantBlock in it (what `QuantModel.set_quant_state` does on the whole model: the
                              block wrappers nested in a Swin unit, its window attentions, switch with it, so both of their sites
                              are measured), with every activation quantiser of the unit (the `act_quantizer` of each of these
                              modules, de-duplicated by identity) temporarily at dynamic_bits = b and the applied ones scanning at
                              [b]: in `units()` order, the widths in the order given
    -> OrderedDict:
      'fp'        the row of `rd_report`'s 'fp'
      'units'     name -> width -> row: the keys of an `rd_report` unit row (bits, bits_total, sse, bpp, mse, psnr_db, loss, d_bits, d_bpp,
                  d_mse, d_psnr_db, d_loss), and size_bits = b x the unit's elements, act_err = the sum over the unit's sites and
                  channels of sum (x - Q_b(x))^2 in float64, act_sqnr_db = 10 log10(sum energy / sum err) in float64 (inf at zero error)
      'elements'  name -> the activation values the unit quantises per image, counted from the calls (a whole number)
      'skipped'   name -> why a unit has no row: none of its quantisers is applied (nothing trained, or all disabled).  Only with
                  units=None; such a unit is refused when it is named
      'widths' (list), 'n', 'pixels', 'lmbda', 'weight_quant', 'batch' (the batch used)
    Frozen ranges are used as they stand at every width: a 'hist_mse' / 'auto' range was chosen for the width it was calibrated at, and is
    not selected again (re-selection per width is out of scope).  A dynamic grid follows its tensor at every width.
    Batch: 1 whatever `batch` says when an applied quantiser of a chosen unit is on a dynamic grid (the batch-1 rule of `rd_report`).
    State: dynamic_bits and act_stats of every activation quantiser of the chosen units and every module's use_weight_quant |
    use_act_quant pair are recorded first and put back in a `finally`, where open scans are closed; ranges, alpha, delta and zero points
    are not written.
    Data parallel: as `rd_report`, the scan sums joining the float64 all-reduce in a fixed order (state by state, site by site).
    Cost: len(units) * len(widths) + 1 passes over `images`.
    Raises ValueError before any GPU work for what `rd_report` refuses, for weight_quant not a bool, for widths that are not a non-empty
    sequence of at most 8 distinct whole numbers in 2 .. MAX_BITS, and for a named unit in which no quantiser is applied."""
    from hipops import ops
    from .quantizer import MAX_BITS
    what = "act_bit_report"
    chosen = _rd_report_args(qnn, images, lmbda, True, batch, units, what=what)
    if not isinstance(weight_quant, bool):
        raise ValueError(f"{what}: weight_quant must be True or False, got {weight_quant!r}")
    widths = ops.width_list(what, widths, MAX_BITS)
    every, applied, skipped = OrderedDict(), OrderedDict(), OrderedDict()
    for name, u in chosen:
        ms = act_modules(u)
        on, seen = [], set()
        for mn, m in ms:
            if act_applied(m) and id(m.act_quantizer) not in seen:
                seen.add(id(m.act_quantizer))
                on.append((f"{mn}.act_quantizer" if mn else "act_quantizer", m.act_quantizer))
        if not on:
            why = "no activation quantiser of the unit is applied (nothing trained, or all disabled)"
            if units is not None:
                raise ValueError(f"{what}: unit {name!r}: {why}")
            skipped[name] = why
            continue
        every[name], applied[name] = _distinct(m.act_quantizer for _, m in ms), on
    chosen = [(name, u) for name, u in chosen if name in every]
    dynamic = any(getattr(q, "act_mode", "dynamic") != "static" for qs in applied.values() for _, q in qs)
    bs = 1 if dynamic else batch
    run = _StateRunner(qnn, images, lmbda, bs, what)
    held = [(q, q.__dict__.get("dynamic_bits", _MISSING), q.__dict__.get("act_stats", _MISSING))
            for q in _distinct(q for qs in every.values() for q in qs)]
    states, scans = [], []
    try:
        with quant_state(qnn):
            qnn.set_quant_state(False, False)
            states.append(run.measure())
            for name, u in chosen:
                for b in widths:
                    qnn.set_quant_state(False, False)
                    for _, m in act_modules(u):
                        m.set_quant_state(weight_quant, True)
                    for q in every[name]:
                        q.dynamic_bits = b
                    for _, q in applied[name]:
                        q.act_scan([b])
                    states.append(run.measure())
                    scans.append(_close_scans(applied[name]))
    finally:
        for q, bits, stats in held:
            q.act_scan_close()
            for f, v in (("dynamic_bits", bits), ("act_stats", stats)):
                if v is _MISSING:
                    q.__dict__.pop(f, None)
                else:
                    setattr(q, f, v)
    run.reduce(states)
    _reduce_scans(scans)
    fp = run.row(states[0])
    rep = OrderedDict()
    rep["fp"], rep["units"], rep["elements"], rep["skipped"] = fp, OrderedDict(), OrderedDict(), skipped
    it, sc = iter(states[1:]), iter(scans)
    for name, _ in chosen:
        rep["units"][name] = OrderedDict()
        for b in widths:
            r = run.against(run.row(next(it)), fp)
            sites = next(sc)
            values = sum(int(st["n"]) * int(st["energy"].numel()) for _, st in sites)
            if values % run.n or rep["elements"].setdefault(name, values // run.n) != values // run.n:
                raise RuntimeError(f"{what}: unit {name!r} quantised {values} values over {run.n} images at width {b}: not the same whole "
                                   "number per image")
            e = float(sum(float(st["err"].sum()) for _, st in sites))
            energy = float(sum(float(st["energy"].sum()) for _, st in sites))
            r["size_bits"], r["act_err"] = b * rep["elements"][name], e
            r["act_sqnr_db"] = float("inf") if e == 0 else 10.0 * math.log10(energy / e)
            rep["units"][name][b] = r
    rep["widths"], rep["n"], rep["pixels"], rep["lmbda"] = list(widths), run.n, run.pixels, float(lmbda)
    rep["weight_quant"], rep["batch"] = weight_quant, bs
    return rep


def allocate_act_bits(report, budget_bits=None, avg_bits=None, fixed=None) -> dict:
    """Choose one activation width per unit from an `act_bit_report` table under a size budget: `allocate_bits` on the table with the
    units' elements (activation values per image) in the place of the weight counts -- its rule, its guarantees and its result, with
    sizes in activation bits per image and `avg_bits` in bits per quantised activation value.  What it returns under 'bits' is what
    `QuantModel.set_act_bits` takes."""
    try:
        table = {"units": report["units"], "weights": report["elements"]}
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f"allocate_act_bits: report must be an `act_bit_report` table ('units', 'elements'): {e!r}")
    return allocate_bits(table, budget_bits=budget_bits, avg_bits=avg_bits, fixed=fixed)


def dequantize(entry) -> torch.Tensor:
    return (entry["levels"].to(torch.float32) - entry["zero_point"]) * entry["delta"]
