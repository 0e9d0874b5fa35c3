"""Reports on a QuantModel.  Three read what the calibration left on the model: `activation_report` (the frozen activation ranges),
`unit_report` (each unit's output error, learned rounding against round-to-nearest) and `bias_report` (what the bias correction did).
Five measure on images: `rd_report` (rate and distortion cost of each unit), `bit_report` / `act_bit_report` (the same at several weight /
activation widths: the tables `widths.allocate_bits` / `allocate_act_bits` choose from), `format_report` (the same in several MX block
formats) and `act_width_report` (one-pass screening of activation widths); `mx_native_report` measures, layer by layer, the MX codes on the matrix cores against their emulation.  The measuring ones are lists of states handed to one sweep driver, `_Sweep`, which owns the argument checks, the
rank sharding, the passes, the restore, the rank reduction and the rows."""
import math
from collections import OrderedDict

import torch

from .quant_block import BaseQuantBlock
from .quant_layer import QuantModule
from .utils import distinct, held_attrs, quant_state
from .widths import act_applied, act_modules, is_trained, weighted_modules


def _sqnr_db(energy, err):
    """10 log10(energy / err) of tensors, inf where err == 0"""
    return torch.where(err == 0, torch.full_like(err, float("inf")), 10.0 * torch.log10(energy / err))


def _sqnr_db_float(energy, err):
    """the same of Python floats (`math.log10`: it may differ from the tensor form in the last bit)"""
    return float("inf") if err == 0 else 10.0 * math.log10(energy / err)


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
            out[name if site == 0 else f"{name}#{site}"] = {
                "err": err, "energy": energy, "clip_lo": lo, "clip_hi": hi, "n": n, "sqnr_db": _sqnr_db(energy.double(), err.double()),
                "clipped_share": (lo.double() + hi.double()) / max(n, 1), "n_bits": int(getattr(q, "dynamic_bits", 8)),
                "channels": int(err.numel())}
    return out


def _moment_rows(qnn, attr, states, fields, totals, head=()):
    """What `unit_report` and `bias_report` both derive from the pair moments a pass recorded under `attr`: (the recorded dict st, its
    row) of every module that holds one, in module order.  The row has the entries `head` of st (strings), n (pixels per channel), an
    empty dict per name of `fields` and in row["total"] per name of `totals`, and for every state of `states`, filled from st[state]:
    row[f][state] for f = err | shift | energy | shift_share (float64 [C], CPU), row["total"][f][state] for err | shift | energy (Python
    floats); then channels."""
    for _, m in qnn.named_modules():
        st = getattr(m, attr, None)
        if not st:
            continue
        row = {h: str(st[h]) for h in head}
        row["n"], row["total"] = int(st["n"]), {}
        for f in fields:
            row[f] = {}
            if f in totals:
                row["total"][f] = {}
        for state in states:
            shift, err, energy = (st[state][f].detach().to("cpu", torch.float64).clone() for f in ("shift", "err", "energy"))
            row["err"][state], row["shift"][state], row["energy"][state] = err, shift, energy
            row["shift_share"][state] = torch.where(err == 0, torch.zeros_like(err), shift * shift / (max(row["n"], 1) * err))
            row["total"]["err"][state], row["total"]["shift"][state] = float(err.sum()), float(shift.sum())
            row["total"]["energy"][state] = float(energy.sum())
        row["channels"] = int(row["err"][states[-1]].numel())
        yield st, row


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
    out = OrderedDict()
    fields = ("err", "shift", "energy", "sqnr_db", "shift_share")
    for st, row in _moment_rows(qnn, "unit_stats", UNIT_REPORT_STATES, fields, fields[:4]):
        for state in UNIT_REPORT_STATES:
            err, energy = row["err"][state], row["energy"][state]
            row["sqnr_db"][state] = _sqnr_db(energy, err)
            row["total"]["sqnr_db"][state] = float(_sqnr_db(energy.sum(), err.sum()))
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
    fields = ("err", "shift", "energy", "shift_share")
    for st, row in _moment_rows(qnn, "bias_stats", BIAS_REPORT_STATES, fields, fields, head=("mode",)):
        for state in BIAS_REPORT_STATES:
            shift, e = row["shift"][state], row["total"]["err"][state]
            row["total"]["shift_share"][state] = 0.0 if e == 0 else float((shift * shift).sum()) / (max(row["n"], 1) * e)
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


def _dynamic_grids(qnn):
    """does an activation quantiser that a forward with act_quant=True applies (its module trained, not disabled) follow its own
    tensor's min | max?"""
    for _, m in qnn.named_modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)) and m.trained and not getattr(m, "disable_act_quant", False) \
                and getattr(m.act_quantizer, "act_mode", "dynamic") != "static":
            return True
    return False


def _close_scans(named):
    """close the scan of every (name, quantiser) -> [(site name, sums)] in order; site names follow `QuantModel.act_ranges`"""
    out = []
    for name, q in named:
        sums = q.act_scan_close()
        for site in sorted(sums):
            out.append((name if site == 0 else f"{name}#{site}", sums[site]))
    return out


class _Sweep:
    """The sweep driver of the measuring reports (`what` names the report in every message).  Making one checks the arguments before
    any GPU work; `shard` takes this rank's share of the images; `run` puts the model through a list of states with one pass over
    those images in each, restores what the states changed, reduces the sums over the ranks and makes the rows (the columns `rd_report`
    documents); `width_table` arranges them per (unit, width)."""

    def __init__(self, what, qnn, images, batch, rd=None, side=64):
        """Checks `images` and `batch` -- all `act_width_report` needs -- and with rd = (lmbda, act_quant, units) those three as well,
        reporting faults in the order images, lmbda, batch, act_quant, units; `chosen` is then the selected (name, unit) pairs in
        `units()` order.  `side`: what the image sides must be a multiple of (64 for the codecs' rate and distortion; a report that
        measures layers takes whatever the model runs)."""
        self.what, self.qnn, self.images = what, qnn, images
        if not torch.is_tensor(images) or images.dtype != torch.float32:
            raise ValueError(f"{what}: images must be an fp32 tensor [n, 3, H, W], got "
                             f"{images.dtype if torch.is_tensor(images) else type(images).__name__}")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"{what}: images must be [n, 3, H, W], got {tuple(images.shape)}")
        if images.numel() == 0:
            raise ValueError(f"{what}: images is empty: {tuple(images.shape)}")
        if images.shape[2] % side or images.shape[3] % side:
            raise ValueError(f"{what}: the image sides must be multiples of {side} (the calibration crops; nothing is padded), got "
                             f"{tuple(images.shape[2:])}")
        lmbda, act_quant, units = (None, None, None) if rd is None else rd
        if rd is not None and (isinstance(lmbda, bool) or not isinstance(lmbda, (int, float)) or not math.isfinite(lmbda) or lmbda <= 0):
            raise ValueError(f"{what}: lmbda must be a positive finite number, got {lmbda!r}")
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError(f"{what}: batch must be an integer >= 1, got {batch!r}")
        self.lmbda, self.chosen = lmbda, None if rd is None else self._units(act_quant, units)
        self.n, _, H, W = (int(v) for v in images.shape)
        self.pixels = self.n * H * W

    def _units(self, act_quant, units):
        what, known = self.what, self.qnn.units()
        if not isinstance(act_quant, bool):
            raise ValueError(f"{what}: act_quant must be True or False, got {act_quant!r}")
        if units is None:
            return list(known.items())
        if isinstance(units, str) or not all(isinstance(u, str) for u in units):
            raise ValueError(f"{what}: units must be None or a list of unit names, got {units!r}")
        unknown = [u for u in units if u not in known]
        if unknown:
            raise ValueError(f"{what}: unknown unit name(s) {unknown}; QuantModel.units() has {list(known)}")
        return [(n, u) for n, u in known.items() if n in set(units)]

    def shard(self, bs):
        """this rank's share of the images, to be run `bs` at a time (`images[rank::world]`); fewer images than ranks is refused"""
        from . import dp
        self.bs, self.device = bs, next(self.qnn.parameters()).device
        rank, self.world = dp.world()
        if self.n < self.world:
            raise ValueError(f"{self.what}: {self.n} image(s) for {self.world} ranks: every rank needs at least one")
        self.mine = self.images[rank::self.world]

    def _pass(self, measure):
        """one pass over this rank's images in the state the model is in -> (keys, float64 device sums [bits of every key | sse]);
        without `measure` the model only runs, for what its quantisers take from the pass -> ([], [])"""
        from hipops import ops
        device, mine, bs = self.device, self.mine, self.bs
        keys, acc, sse = None, None, torch.zeros(1, dtype=torch.float64, device=device) if measure else None
        with torch.no_grad():
            for i in range(0, mine.shape[0], bs):
                x = mine[i:i + bs].to(device).contiguous()
                out = self.qnn(x)
                if not measure:
                    continue
                liks = out["likelihoods"]
                if keys is None:
                    keys = list(liks)
                    acc = [torch.zeros(liks[k].shape[1], dtype=torch.float64, device=device) for k in keys]
                for a, k in zip(acc, keys):
                    a += ops.neg_log2_channel_sums(liks[k]).double()
                sse += ops.sq_diff_sum_ordered(out["x_hat"].contiguous(), x, 1.0, clamp01=True).double()
        return (keys, acc + [sse]) if measure else ([], [])

    def _reduce(self, tensors):
        """all-reduce (SUM) float64 device tensors in place, as ONE flat tensor in the order given; nothing to do for one rank"""
        from . import dp
        if self.world <= 1 or not tensors:
            return
        flat = torch.cat([t.reshape(-1) for t in tensors])
        dp.reduce_act_stats(sums=[flat])
        off = 0
        for t in tensors:
            t.copy_(flat[off:off + t.numel()].reshape(t.shape))
            off += t.numel()

    def _reduce_scans(self, scans):
        """the same for the closed scan sums [[(site name, {err, energy, n})]], state by state and site by site; the counts travel as
        float64 (whole numbers far below 2^53)"""
        if self.world <= 1:
            return
        rows = [st for state in scans for _, st in state]
        counts = [torch.tensor([st["n"]], dtype=torch.float64, device=st["err"].device) for st in rows]
        self._reduce([t for st, n in zip(rows, counts) for t in (st["err"], st["energy"], n)])
        for st, n in zip(rows, counts):
            st["n"] = int(n)

    def _row(self, keys, sums):
        bits = OrderedDict((k, a.cpu()) for k, a in zip(keys, sums))
        total, sse = float(sum(b.sum() for b in bits.values())), float(sums[-1])
        mse = sse / (3 * self.pixels)
        r = OrderedDict(bits=bits, bits_total=total, sse=sse, bpp=total / self.pixels, mse=mse,
                        psnr_db=float("inf") if mse == 0 else -10.0 * math.log10(mse))
        r["loss"] = r["bpp"] + self.lmbda * 255.0 ** 2 * mse
        return r

    def run(self, states, held=(), fields=(), scanned=(), measure=True):
        """states: [(key, enter)], the first being 'fp' when rows are wanted.  For each in order: qnn.set_quant_state(False, False),
        `enter()` (None: nothing more to set up), one pass; an `enter` may return a `leave()`, called after the pass, that yields the
        state's closed scans (`_close_scans`).  The quant-state flags and the attributes `fields` of the objects `held` are put back
        whatever happens (`quant_state`, `held_attrs`), and the scans of the quantisers `scanned` are closed.  Then one all-reduce of
        the passes' sums and one of the scans', in state order.
        -> (rows: key -> row, every one but the first with the differences against the first; scans: key -> what `leave()` gave)."""
        qnn, sums, scans = self.qnn, [], OrderedDict()
        with quant_state(qnn), held_attrs(held, fields):
            try:
                for key, enter in states:
                    qnn.set_quant_state(False, False)
                    leave = None if enter is None else enter()
                    sums.append(self._pass(measure))
                    if leave is not None:
                        scans[key] = leave()
            finally:
                for q in scanned:
                    q.act_scan_close()
        self._reduce([t for _, ts in sums for t in ts])
        self._reduce_scans(list(scans.values()))
        rows, fp = OrderedDict(), None
        for (key, _), (keys, ts) in zip(states, sums if measure else []):
            r = rows[key] = self._row(keys, ts)
            if fp is None:
                fp = r
                continue
            r["d_bits"] = OrderedDict((k, r["bits"][k] - fp["bits"][k]) for k in r["bits"])
            for f in ("bpp", "mse", "psnr_db", "loss"):
                r["d_" + f] = r[f] - fp[f]
        return rows, scans

    @staticmethod
    def width_table(rows, names, widths, elements, cost, column):
        """name -> width -> rows[name, width] with three more columns: size_bits = width x elements[name], `column`_err and
        `column`_sqnr_db from (err, energy) = cost(name, k) for the k-th width, as Python floats"""
        table = OrderedDict()
        for name in names:
            table[name] = OrderedDict()
            for k, b in enumerate(widths):
                r, (err, energy) = rows[name, b], cost(name, k)
                r["size_bits"], r[column + "_err"] = b * elements[name], err
                r[column + "_sqnr_db"] = _sqnr_db_float(energy, err)
                table[name][b] = r
        return table


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
    sweep = _Sweep("rd_report", qnn, images, batch, (lmbda, act_quant, units))
    sweep.shard(1 if (act_quant and _dynamic_grids(qnn)) else batch)
    states = [("fp", None), ("all", lambda: qnn.set_quant_state(True, act_quant))]
    states += [(("unit", name), lambda u=u: u.set_quant_state(True, act_quant)) for name, u in sweep.chosen]
    rows, _ = sweep.run(states)
    rep = OrderedDict()
    rep["fp"], rep["all"] = rows["fp"], rows["all"]
    rep["units"] = OrderedDict((name, rows["unit", name]) for name, _ in sweep.chosen)
    rep["n"], rep["pixels"], rep["lmbda"], rep["act_quant"] = sweep.n, sweep.pixels, float(lmbda), act_quant
    rep["additivity"] = {"sum_units_d_loss": float(sum(r["d_loss"] for r in rep["units"].values())), "all_d_loss": rep["all"]["d_loss"]}
    rep["batch"] = sweep.bs
    return rep


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
    sweep = _Sweep(what, qnn, images, batch, (lmbda, False, units))
    widths = ops.width_list(what, widths, MAX_BITS)
    mods = OrderedDict((name, weighted_modules(u)) for name, u in sweep.chosen)
    for name, ms in mods.items():
        if any(is_trained(m) for m in ms):
            raise ValueError(f"{what}: unit {name!r} holds a trained module: the table is taken before calibration")
    sweep.shard(batch)
    every = [m for ms in mods.values() for m in ms]
    grids, weight_cols = {}, {}

    def scan():
        """the weights of every chosen unit at every width, once, in front of the 'fp' pass: the first GPU work"""
        for name, ms in mods.items():
            grids[name] = [_width_grids(m, widths) for m in ms]
            err = torch.stack([g[2].sum(1) for g in grids[name]]).sum(0).cpu()            # float64 [K]
            weight_cols[name] = (err, float(torch.stack([g[3].sum() for g in grids[name]]).sum()))

    def at(name, u, k, b):
        def enter():
            u.set_quant_state(True, False)
            for m, (d, z, _, _) in zip(mods[name], grids[name]):
                q = m.weight_quantizer
                shape = _scale_shape(m.weight, q.tconv) if q.channel_wise else ()
                q.bitwidth_refactor(b)
                q.delta, q.zero_point, q.inited = d[k].reshape(shape), z[k].reshape(shape), True
                m.drop_weight_pack()
        return enter
    states = [("fp", scan)] + [((name, b), at(name, u, k, b)) for name, u in sweep.chosen for k, b in enumerate(widths)]
    try:
        rows, _ = sweep.run(states, held=[m.weight_quantizer for m in every], fields=_QUANTIZER_FIELDS)
    finally:
        for m in every:                                                                     # (the widths are back: no pack of another one stays)
            m.drop_weight_pack()
    counts = OrderedDict((name, sum(int(m.weight.numel()) for m in ms)) for name, ms in mods.items())
    rep = OrderedDict()
    rep["fp"] = rows["fp"]
    rep["units"] = sweep.width_table(rows, list(mods), widths, counts,
                                     lambda name, k: (float(weight_cols[name][0][k]), weight_cols[name][1]), "weight")
    rep["weights"] = counts
    rep["widths"], rep["n"], rep["pixels"], rep["lmbda"], rep["batch"] = list(widths), sweep.n, sweep.pixels, float(lmbda), batch
    return rep


def _format_list(what, formats):
    """`formats` as a list of names: a non-empty sequence of distinct names of `hipops._lib.MX_FORMATS`, else ValueError"""
    from hipops import ops
    if isinstance(formats, (str, bytes)) or not hasattr(formats, "__len__") or not hasattr(formats, "__iter__"):
        raise ValueError(f"{what}: formats must be a sequence of MX format names, got {formats!r}")
    formats = list(formats)
    if not formats:
        raise ValueError(f"{what}: formats must hold at least one name")
    for f in formats:
        ops.mx_format(what, f)
    if len(set(formats)) != len(formats):
        raise ValueError(f"{what}: formats must be distinct, got {formats}")
    return formats


def format_report(qnn, images, formats=("mxfp4", "mxfp6_e2m3", "mxfp8_e4m3"), lmbda=0.01, batch=8, units=None) -> "OrderedDict":
    """What each reconstruction unit costs in rate and distortion in each of several MX block formats (include/rdo_ptq_mx.h), measured on
    `images` like `rd_report` (its rules for `images`, `lmbda`, `batch` and `units`) under torch.no_grad(), BEFORE calibration: weights
    only (activation quantisation is off in every state), round to nearest.  `bit_report` with formats in place of widths.  The states,
    all over the same images:
      'fp'                     qnn.set_quant_state(False, False): the 'fp' state of `rd_report`
      one per (unit, format)   qnn.set_quant_state(False, False); unit.set_quant_state(True, False), with every weighted QuantModule of
                               the unit temporarily holding an `mx.MXQuantizer` of the format: in `units()` order, the formats in the
                               order given
    -> OrderedDict:
      'fp'       the row of `rd_report`'s 'fp'
      'units'    name -> format -> row: the keys of an `rd_report` unit row (bits, bits_total, sse, bpp, mse, psnr_db, loss, d_bits, d_bpp,
                 d_mse, d_psnr_db, d_loss), and size_bits = the sum over the unit's modules of element bits x elements + 8 x blocks,
                 weight_err = the sum over the unit's modules and rows of the kernel's sum (w - wq)^2 in float64, weight_sqnr_db = 10
                 log10(sum energy / sum err) in float64 (inf at zero error), bits_per_weight = size_bits / the unit's weight elements
      'weights'  name -> weight elements of the unit (its weighted QuantModules; biases are not counted)
      'formats' (list), 'n', 'pixels', 'lmbda', 'batch'
    State: the `weight_quantizer` of every weighted module of the chosen units and every module's use_weight_quant | use_act_quant
    pair are recorded first and put back in a `finally` (the same objects, so the same bits); `drop_weight_pack()` runs at every switch
    and at the end.
    Data parallel: as `rd_report`; every rank scores the weights itself, which gives the same bits.
    Cost: len(units) * len(formats) + 1 passes over `images`.
    Raises ValueError before any GPU work for what `rd_report` refuses, for formats that are not a non-empty sequence of distinct names
    of `MX_FORMATS`, and for a chosen unit that holds a trained module (the table is taken before calibration)."""
    from .mx import MXQuantizer
    what = "format_report"
    sweep = _Sweep(what, qnn, images, batch, (lmbda, False, units))
    formats = _format_list(what, formats)
    mods = OrderedDict((name, weighted_modules(u)) for name, u in sweep.chosen)
    for name, ms in mods.items():
        if any(is_trained(m) for m in ms):
            raise ValueError(f"{what}: unit {name!r} holds a trained module: the table is taken before calibration")
    sweep.shard(batch)
    every = [m for ms in mods.values() for m in ms]
    made = {(name, f): [MXQuantizer(f, tconv=m.if_tconv) for m in ms] for name, ms in mods.items() for f in formats}
    weight_cols = {}

    def scan():
        """the weights of every chosen unit in every format, once, in front of the 'fp' pass: the first GPU work"""
        for (name, f), qs in made.items():
            costs = [q.weight_cost(m.weight) for q, m in zip(qs, mods[name])]
            weight_cols[name, f] = (float(torch.stack([e.sum() for e, _ in costs]).sum()), float(torch.stack([en.sum() for _, en in costs]).sum()))

    def at(name, u, f):
        def enter():
            u.set_quant_state(True, False)
            for m, q in zip(mods[name], made[name, f]):
                m.weight_quantizer = q
                m.drop_weight_pack()
        return enter
    states = [("fp", scan)] + [((name, f), at(name, u, f)) for name, u in sweep.chosen for f in formats]
    try:
        rows, _ = sweep.run(states, held=every, fields=("weight_quantizer",))
    finally:
        for m in every:                                                                     # (the quantisers are back: no pack of a format stays)
            m.drop_weight_pack()
    counts = OrderedDict((name, sum(int(m.weight.numel()) for m in ms)) for name, ms in mods.items())
    rep = OrderedDict()
    rep["fp"], rep["units"] = rows["fp"], OrderedDict()
    for name, ms in mods.items():
        rep["units"][name] = OrderedDict()
        for f in formats:
            r, (err, energy) = rows[name, f], weight_cols[name, f]
            r["size_bits"] = sum(q.size_bits(m.weight) for q, m in zip(made[name, f], ms))
            r["weight_err"], r["weight_sqnr_db"] = err, _sqnr_db_float(energy, err)
            r["bits_per_weight"] = r["size_bits"] / counts[name]
            rep["units"][name][f] = r
    rep["weights"] = counts
    rep["formats"], rep["n"], rep["pixels"], rep["lmbda"], rep["batch"] = list(formats), sweep.n, sweep.pixels, float(lmbda), batch
    return rep


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
    sweep = _Sweep(what, qnn, images, batch)
    widths = ops.width_list(what, widths, MAX_BITS)
    unit_of = {id(m): name for name, u in qnn.units().items() for _, m in act_modules(u)}
    holders = [(name, m) for name, m in qnn.named_modules() if isinstance(m, (QuantModule, BaseQuantBlock)) and act_applied(m)]
    holders = distinct(holders, of=lambda p: p[1].act_quantizer)
    named = [(f"{name}.act_quantizer", m.act_quantizer) for name, m in holders]
    meta = {f"{name}.act_quantizer": (unit_of.get(id(m)), m.act_quantizer) for name, m in holders}
    sweep.shard(1 if _dynamic_grids(qnn) else batch)

    def enter():
        qnn.set_quant_state(True, True)
        for _, q in named:
            q.act_scan(widths)
        return lambda: _close_scans(named)
    _, scans = sweep.run([("all", enter)], scanned=[q for _, q in named], measure=False)
    rep = OrderedDict()
    rep["sites"] = OrderedDict()
    for site, st in scans["all"]:
        unit, q = meta[site.split("#")[0]]
        err, energy = st["err"].cpu(), st["energy"].cpu()
        rep["sites"][site] = {"unit": unit, "mode": getattr(q, "act_mode", "dynamic"), "n_bits": int(getattr(q, "dynamic_bits", 8)),
                              "channels": int(energy.numel()), "n": int(st["n"]), "err": err, "energy": energy,
                              "sqnr_db": _sqnr_db(energy.unsqueeze(0), err),
                              "total": {"err": err.sum(1), "energy": float(energy.sum()), "sqnr_db": _sqnr_db(energy.sum(), err.sum(1))}}
    rep["widths"], rep["n"], rep["batch"] = list(widths), sweep.n, sweep.bs
    return rep


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
    sweep = _Sweep(what, qnn, images, batch, (lmbda, True, units))
    if not isinstance(weight_quant, bool):
        raise ValueError(f"{what}: weight_quant must be True or False, got {weight_quant!r}")
    widths = ops.width_list(what, widths, MAX_BITS)
    every, applied, skipped = OrderedDict(), OrderedDict(), OrderedDict()
    for name, u in sweep.chosen:
        ms = act_modules(u)
        on = [(f"{mn}.act_quantizer" if mn else "act_quantizer", m.act_quantizer)
              for mn, m in distinct([p for p in ms if act_applied(p[1])], of=lambda p: p[1].act_quantizer)]
        if not on:
            why = "no activation quantiser of the unit is applied (nothing trained, or all disabled)"
            if units is not None:
                raise ValueError(f"{what}: unit {name!r}: {why}")
            skipped[name] = why
            continue
        every[name], applied[name] = distinct(m.act_quantizer for _, m in ms), on
    dynamic = any(getattr(q, "act_mode", "dynamic") != "static" for qs in applied.values() for _, q in qs)
    sweep.shard(1 if dynamic else batch)

    def at(name, u, b):
        def enter():
            for _, m in act_modules(u):
                m.set_quant_state(weight_quant, True)
            for q in every[name]:
                q.dynamic_bits = b
            for _, q in applied[name]:
                q.act_scan([b])
            return lambda: _close_scans(applied[name])
        return enter
    held = distinct(q for qs in every.values() for q in qs)
    states = [("fp", None)] + [((name, b), at(name, u, b)) for name, u in sweep.chosen if name in every for b in widths]
    rows, scans = sweep.run(states, held=held, fields=("dynamic_bits", "act_stats"), scanned=held)
    elements = OrderedDict()
    for (name, b), sites in scans.items():
        values = sum(int(st["n"]) * int(st["energy"].numel()) for _, st in sites)
        if values % sweep.n or elements.setdefault(name, values // sweep.n) != values // sweep.n:
            raise RuntimeError(f"{what}: unit {name!r} quantised {values} values over {sweep.n} images at width {b}: not the same whole "
                               "number per image")

    def cost(name, k):
        sites = scans[name, widths[k]]
        return (float(sum(float(st["err"].sum()) for _, st in sites)), float(sum(float(st["energy"].sum()) for _, st in sites)))
    rep = OrderedDict()
    rep["fp"], rep["units"] = rows["fp"], sweep.width_table(rows, list(every), widths, elements, cost, "act")
    rep["elements"], rep["skipped"] = elements, skipped
    rep["widths"], rep["n"], rep["pixels"], rep["lmbda"] = list(widths), sweep.n, sweep.pixels, float(lmbda)
    rep["weight_quant"], rep["batch"] = weight_quant, sweep.bs
    return rep


def mx_native_report(qnn, images, act_fmt="mxfp8_e4m3", batch=8, units=None, convs=False, tconvs=False) -> "OrderedDict":
    """How far the MX codes on the matrix cores are from the emulation a calibration runs under, layer by layer (include/rdo_ptq_mxgemm.h;
    `mx.native_linear`), measured on `images` (fp32 [n, 3, H, W] of any size the model runs) under torch.no_grad() in ONE pass over the
    images in the state the model is in: weights in their MX formats (`set_weight_format`), the quant-state flags as set.  Every
    eligible module of the chosen units (`mx.native_refusal`: a Linear or 1x1 stride-1 conv on an MX weight quantiser with input
    channels a multiple of 32) computes, under a forward pre-hook, from its actual input x:
      native     `ops.mx_quant_pack(rows of x, act_fmt)` x `mx.native_operand(module)` + bias by `ops.mx_gemm`
      emulated   xq of the same `mx_quant_pack` call and the decoded weight (`ops.mx_dequant` of the operand's own codes) through the
                 fp32-accurate forward kernel the module's forward uses, epilogue EPI_NONE, same bias
    The model's own forward goes on with x untouched.
    convs=True also measures every conv `mx.native_conv_refusal` accepts (include/rdo_ptq_mxconv.h: a square kernel, one stride, one
    zero padding, dilation 1, groups 1, input channels a multiple of 32; a 1x1 conv among them goes this way too):
      native     `ops.mx_quant_pack(NHWC pixels of x, act_fmt)`, then `ops.mx_conv2d` with `mx.native_conv_operand(module)` + bias
      emulated   xq of the same call as NHWC and the decoded weight as [N, k, k, Cin] through `ops.conv2d_fwd_pack` at the module's
                 stride and padding, epilogue EPI_NONE, same bias
    Their rows gain k, stride and pad; K is k * k * Cin, rows counts output pixels, act_sqnr_db is taken over the input pixels; a conv
    that is refused is skipped for the reason `native_conv_refusal` gives.  convs=False gives what it gave before convs existed.
    tconvs=True also measures every transposed conv `mx.native_tconv_refusal` accepts (include/rdo_ptq_mxtconv.h):
      native     `ops.mx_quant_pack(NHWC pixels of x, act_fmt)`, then `ops.mx_conv_transpose2d` with `mx.native_tconv_operand(module)` + bias
      emulated   xq of the same call as NHWC and the decoded weight as [N, k, k, Cin] through `ops.conv_transpose2d` at the module's
                 stride, padding and output padding, epilogue EPI_NONE, same bias
    Their rows gain k, stride, pad and output_padding; K is k * k * Cin, N the output channels (`weight.shape[1]`).  tconvs=False gives
    what it gave before tconvs existed, the 'skipped' reasons included.
    -> OrderedDict:
      'modules'  name -> {unit, rows (per pass, all images), K, N, w_fmt, act_fmt, max_abs_diff, rel_l2 = |native - emulated| /
                 |emulated| from float64 sums over the batches (0 when both are zero), act_sqnr_db = 10 log10(sum x^2 / sum (x - xq)^2)
                 in float64 (inf at zero error)}
      'skipped'  name -> why a weighted module of the chosen units has no row
      'act_fmt', 'n', 'batch'
    State: every module's use_weight_quant | use_act_quant pair is put back in a `finally` and the hooks are removed whatever a forward
    raises; quantisers, alpha and scales are not written; the operands made stay memoised next to the weight packs.
    Raises ValueError before any GPU work for what `rd_report` refuses of images (but for their size), batch and units, for an unknown
    act_fmt, for convs or tconvs not a bool, and for a named unit without an eligible module; NotImplementedError for world_size > 1."""
    from hipops import _lib as L
    from hipops import ops
    from . import dp, mx
    what = "mx_native_report"
    sweep = _Sweep(what, qnn, images, batch, side=1)
    chosen = sweep._units(False, units)
    ops.mx_format(what, act_fmt)
    if not isinstance(convs, bool):
        raise ValueError(f"{what}: convs must be True or False, got {convs!r}")
    if not isinstance(tconvs, bool):
        raise ValueError(f"{what}: tconvs must be True or False, got {tconvs!r}")
    if dp.world()[1] > 1:
        raise NotImplementedError(f"{what}: not built for data-parallel runs (world_size > 1)")
    eligible, skipped = OrderedDict(), OrderedDict()
    for uname, u in chosen:
        found = False
        for mn, m in u.named_modules():
            if not isinstance(m, QuantModule) or m.org_weight is None:
                continue
            name = f"{uname}.{mn}" if mn else uname
            as_conv = convs and m.kind == "conv"
            as_tconv = tconvs and m.kind == "tconv"
            why = mx.native_tconv_refusal(m) if as_tconv else mx.native_conv_refusal(m) if as_conv else mx.native_refusal(m)
            if why is None:
                eligible[name], found = (uname, m), True
            else:
                skipped[name] = why
        if units is not None and not found:
            raise ValueError(f"{what}: unit {uname!r} holds no eligible module: "
                             f"{ {n: w for n, w in skipped.items() if n == uname or n.startswith(uname + '.')} }")
    sweep.shard(batch)
    flags = quant_state(qnn)                                                            # the flags as found: `run` clears them before `enter`
    sums, packs, handles = {}, {}, []

    def decoded(name, b, bias, shape):
        pack = packs.get(name)
        if pack is None or pack[0] is not b:
            wdec = ops.mx_dequant(ops.mx_unpack_codes(b), b.scales, b.K, b.fmt)
            pack = packs[name] = (b, ops.WeightPack(wdec.reshape(shape), bias))
        return pack[1]

    def measure_conv(mod, name, x):
        """(pixel rows, xq, native, emulated) of a conv on `ops.mx_conv2d`; native and emulated [output pixels, N]"""
        C = int(mod.weight.shape[1])
        if x.dim() != 4 or x.shape[1] != C:
            raise ValueError(f"{what}: module {name!r}: the input must be [B, {C}, H, W], got {tuple(x.shape)}")
        B, _, H, W = (int(v) for v in x.shape)
        k, stride, pad = mx.conv_geometry(mod)
        rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
        b = mx.native_conv_operand(mod)
        a, xq = ops.mx_quant_pack(rows, act_fmt, want_xq=True)
        bias = mx.native_bias(mod)
        native = ops.mx_conv2d(a, b, (B, H, W), k, stride, pad, bias).reshape(-1, b.rows)
        emulated = ops.conv2d_fwd_pack(xq.reshape(B, H, W, C), decoded(name, b, bias, (b.rows, k, k, C)), stride, pad, epilogue=L.EPI_NONE)
        return rows, xq, native, emulated.reshape(native.shape)

    def measure_tconv(mod, name, x):
        """(pixel rows, xq, native, emulated) of a transposed conv on `ops.mx_conv_transpose2d`; native and emulated [output pixels, N]"""
        C = int(mod.weight.shape[0])
        if x.dim() != 4 or x.shape[1] != C:
            raise ValueError(f"{what}: module {name!r}: the input must be [B, {C}, H, W], got {tuple(x.shape)}")
        B, _, H, W = (int(v) for v in x.shape)
        k, stride, pad, opad = mx.tconv_geometry(mod)
        rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
        b = mx.native_tconv_operand(mod)
        a, xq = ops.mx_quant_pack(rows, act_fmt, want_xq=True)
        bias = mx.native_bias(mod)
        native = ops.mx_conv_transpose2d(a, b, (B, H, W), k, stride, pad, opad, bias).reshape(-1, b.rows)
        emulated = ops.conv_transpose2d(xq.reshape(B, H, W, C), None, None, stride, pad, opad, epilogue=L.EPI_NONE,
                                        pack=decoded(name, b, bias, (b.rows, k, k, C)))
        return rows, xq, native, emulated.reshape(native.shape)

    def measure(name, m):
        as_conv = convs and m.kind == "conv"
        as_tconv = tconvs and m.kind == "tconv"

        def hook(mod, args):
            x = args[0].detach()
            if as_tconv:
                rows, xq, native, emulated = measure_tconv(mod, name, x)
            elif as_conv:
                rows, xq, native, emulated = measure_conv(mod, name, x)
            else:
                rows, _ = mx.native_rows(mod, x)
                b = mx.native_operand(mod)
                a, xq = ops.mx_quant_pack(rows, act_fmt, want_xq=True)
                bias = mx.native_bias(mod)
                native = ops.mx_gemm(a, b, bias)
                emulated = ops.conv2d_fwd_pack(xq.reshape(1, 1, -1, b.K), decoded(name, b, bias, (b.rows, 1, 1, b.K)), 1, 0,
                                               epilogue=L.EPI_NONE).reshape(native.shape)
            d = (native - emulated).double()
            x64, e64 = rows.double(), (rows - xq).double()
            new = torch.stack([(d * d).sum(), (emulated.double() ** 2).sum(), (x64 * x64).sum(), (e64 * e64).sum(), d.abs().max()])
            st = sums.get(name)
            if st is None:
                sums[name] = [new, int(native.shape[0])]
            else:
                st[0] = torch.cat([st[0][:4] + new[:4], torch.maximum(st[0][4:], new[4:])])
                st[1] += int(native.shape[0])
        return hook

    def enter():
        for m, (w, a) in zip(flags.mods, flags.held):
            m.use_weight_quant, m.use_act_quant = w, a
        for name, (_, m) in eligible.items():
            handles.append(m.register_forward_pre_hook(measure(name, m)))
    try:
        sweep.run([("found", enter)], measure=False)
    finally:
        for h in handles:
            h.remove()
    rep = OrderedDict()
    rep["modules"] = OrderedDict()
    for name, (uname, m) in eligible.items():
        if name not in sums:
            skipped[name] = "the pass never called the module"
            continue
        t, rows = sums[name]
        diff2, emu2, x2, e2, mad = (float(v) for v in t.cpu())
        rep["modules"][name] = {"unit": uname, "rows": rows, "K": int(m.weight.shape[1]), "N": int(m.weight.shape[0]),
                                "w_fmt": m.weight_quantizer.fmt, "act_fmt": act_fmt, "max_abs_diff": mad,
                                "rel_l2": 0.0 if diff2 == 0 else math.sqrt(diff2 / emu2) if emu2 > 0 else float("inf"),
                                "act_sqnr_db": _sqnr_db_float(x2, e2)}
        if convs and m.kind == "conv":
            k, stride, pad = mx.conv_geometry(m)
            rep["modules"][name].update(k=k, stride=stride, pad=pad, K=k * k * int(m.weight.shape[1]))
        if tconvs and m.kind == "tconv":
            k, stride, pad, opad = mx.tconv_geometry(m)
            rep["modules"][name].update(k=k, stride=stride, pad=pad, output_padding=opad, K=k * k * int(m.weight.shape[0]),
                                        N=int(m.weight.shape[1]))
    rep["skipped"] = skipped
    rep["act_fmt"], rep["n"], rep["batch"] = act_fmt, sweep.n, sweep.bs
    return rep
