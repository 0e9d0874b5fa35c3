"""`QuantModel`: module surgery that wraps a LIC model's layers in QuantModule / quant blocks
(reference surface: quantization/quant_model.py:10-98)."""
import torch.nn as nn

from lic import EntropyBottleneck

from .fold_bn import search_fold_and_remove_bn
from .quant_block import BaseQuantBlock, specials
from .quant_layer import GDN_TYPES, QuantModule, StraightThrough
from .widths import act_applied, act_modules, format_plan, is_trained, weighted_modules, width_plan

_WRAPPABLE = (nn.Conv2d, nn.ConvTranspose2d, nn.Linear, nn.LayerNorm, nn.PixelShuffle) + GDN_TYPES
_FUSABLE_ACT = (nn.LeakyReLU, nn.GELU, nn.ReLU, nn.ReLU6)


class QuantModel(nn.Module):
    def __init__(self, model: nn.Module, weight_quant_params: dict = {}, act_quant_params: dict = {}, is_fusing=True,
                 is_cheng=False):
        super().__init__()
        if is_fusing:
            search_fold_and_remove_bn(model)
        self.model = model
        self.quant_module_refactor(self.model, weight_quant_params, act_quant_params, is_cheng)

    def quant_module_refactor(self, module: nn.Module, weight_quant_params: dict = {}, act_quant_params: dict = {},
                              is_cheng=False):
        """Depth-first replacement.  Exact-type matches in `specials` become blocks; wrappable leaves become QuantModules;
        an activation that directly follows a QuantModule *at the same nesting level* is fused into it and replaced by a
        StraightThrough (so the unit schedule and fused activations equal the reference's, quant_model.py:34-62)."""
        last = None
        for name, child in module.named_children():
            if type(child) in specials:
                setattr(module, name, specials[type(child)](child, weight_quant_params, act_quant_params))
            elif isinstance(child, _WRAPPABLE):
                last = QuantModule(child, weight_quant_params, act_quant_params)
                setattr(module, name, last)
            elif isinstance(child, _FUSABLE_ACT):
                if last is not None:
                    last.activation_function = child
                    setattr(module, name, StraightThrough())
            elif isinstance(child, StraightThrough):
                continue
            else:
                self.quant_module_refactor(child, weight_quant_params, act_quant_params, is_cheng)

    def _quant_modules(self):
        return [m for m in self.model.modules() if isinstance(m, QuantModule)]

    def set_quant_state(self, weight_quant: bool = False, act_quant: bool = False):
        for m in self.model.modules():
            if isinstance(m, (QuantModule, BaseQuantBlock)):
                m.set_quant_state(weight_quant, act_quant)

    def act_quantizers(self):
        """(name, quantiser) of every activation quantiser: one per QuantModule and one per block wrapper."""
        return [(f"{name}.act_quantizer", m.act_quantizer) for name, m in self.named_modules()
                if isinstance(m, (QuantModule, BaseQuantBlock))]

    def set_act_mode(self, mode: str):
        """'dynamic' (default: the grid of every tensor is its own min / max) or 'static' (per-channel ranges frozen by the
        calibration flow, recon.py with args.act_mode='static'; an unfrozen static quantiser raises when it is applied)."""
        for _, q in self.act_quantizers():
            q.set_act_mode(mode)

    def act_ranges(self):
        """OrderedDict name -> (lo, hi, n_bits) of the frozen static ranges.  A quantiser applied at several places of its block (the
        joins of a residual block; probabilities and attn @ v of an attention) has one entry per place: 'name', 'name#1', ..."""
        from collections import OrderedDict
        out = OrderedDict()
        for name, q in self.act_quantizers():
            if not q.act_frozen():
                continue
            for site in sorted(q.act_range):
                r = q.act_range[site]
                c = r.numel() // 2
                out[name if site == 0 else f"{name}#{site}"] = (r[:c], r[c:], getattr(q, "dynamic_bits", 8))
        return out

    def act_report(self):
        """OrderedDict name -> the measured statistics of every frozen static range that was recorded (args.act_report):
        `export.activation_report`, under the site names of `act_ranges`."""
        from .reports import activation_report
        return activation_report(self)

    def unit_report(self):
        """OrderedDict unit name -> the measured output error of every calibrated unit that recorded it (args.unit_report): per output
        channel, learned rounding against round-to-nearest (`export.unit_report`)."""
        from .reports import unit_report
        return unit_report(self)

    def bias_report(self):
        """OrderedDict unit name -> what the bias correction of every unit that ran it did (args.bias_correct): the corrected layers'
        shifts and the unit's output error before and after (`export.bias_report`)."""
        from .reports import bias_report
        return bias_report(self)

    def clear_bias_correction(self):
        """Undo every bias correction: `org_bias` goes back into the bias of each corrected layer (bit for bit), the weight packs made
        from the corrected biases are dropped, `bias_shift` and the units' `bias_stats` are removed."""
        for m in self.modules():
            if isinstance(m, QuantModule) and "bias_shift" in m.__dict__:
                m.bias.data.copy_(m.org_bias)
                m.drop_weight_pack()
                del m.bias_shift
            if "bias_stats" in m.__dict__:
                del m.bias_stats

    def units(self):
        """OrderedDict name -> reconstruction unit, in the order the calibration visits them (recon_model of the reference's
        main2.py:227-253): every child that is a QuantModule or a BaseQuantBlock is a unit under its dotted name, anything else is
        descended into; QuantModules without a weight (pixel shuffles) are left out."""
        from collections import OrderedDict
        out = OrderedDict()

        def walk(mod, prefix):
            for n, c in mod.named_children():
                if isinstance(c, (QuantModule, BaseQuantBlock)):
                    if not (isinstance(c, QuantModule) and c.org_weight is None):
                        out[prefix + n] = c
                else:
                    walk(c, prefix + n + ".")
        walk(self.model, "")
        return out

    def rd_report(self, images, lmbda=0.01, act_quant=False, batch=8, units=None):
        """What every unit costs in rate and distortion when it alone is quantised, next to the full-precision and the fully
        quantised model, measured on `images` (`export.rd_report`)."""
        from .reports import rd_report
        return rd_report(self, images, lmbda=lmbda, act_quant=act_quant, batch=batch, units=units)

    def bit_report(self, images, widths=(4, 6, 8), lmbda=0.01, batch=8, units=None):
        """What every unit costs in rate and distortion at each of several weight widths when it alone is quantised (round to nearest,
        weights only), with each width's size and weight error: the table `export.allocate_bits` chooses from (`export.bit_report`).
        len(units) * len(widths) + 1 passes over `images`; taken before calibration."""
        from .reports import bit_report
        return bit_report(self, images, widths=widths, lmbda=lmbda, batch=batch, units=units)

    def set_weight_bits(self, bits):
        """Give the weights of the units their widths before calibration: `bits` is one whole number in 2 .. MAX_BITS for every unit, or
        a mapping unit name -> width (what `export.allocate_bits(...)['bits']` is; units it does not name keep theirs).  Names and widths
        are validated and a unit that holds a trained module is refused (ValueError) before anything is written; then every weighted
        QuantModule of each named unit gets `bitwidth_refactor(b)`, `inited = False` (its scale is initialised at the new width on its
        next use) and `drop_weight_pack()`.  Activation quantisers are not touched."""
        what, known = "set_weight_bits", self.units()
        plan = width_plan(what, known, bits)
        for n, _ in plan:
            if any(is_trained(m) for m in weighted_modules(known[n])):
                raise ValueError(f"{what}: unit {n!r} holds a trained module: its rounding belongs to the width it was calibrated at")
        for n, b in plan:
            for m in weighted_modules(known[n]):
                m.weight_quantizer.bitwidth_refactor(int(b))
                m.weight_quantizer.inited = False
                m.drop_weight_pack()

    def format_report(self, images, formats=("mxfp4", "mxfp6_e2m3", "mxfp8_e4m3"), lmbda=0.01, batch=8, units=None):
        """What every unit costs in rate and distortion in each of several MX block formats when it alone is quantised (round to nearest,
        weights only), with each format's size and weight error: `bit_report` with formats in place of widths (`export.format_report`).
        len(units) * len(formats) + 1 passes over `images`; taken before calibration."""
        from .reports import format_report
        return format_report(self, images, formats=formats, lmbda=lmbda, batch=batch, units=units)

    def mx_native_report(self, images, act_fmt="mxfp8_e4m3", batch=8, units=None, convs=False, tconvs=False):
        """How far the MX codes on the matrix cores (`mx.native_linear`: the block-scaled matrix instruction, input quantised to
        `act_fmt`) are from their fp32 emulation, for every eligible Linear / 1x1 conv of the chosen units -- with convs=True also for
        every eligible k x k conv (`mx.native_conv`), with tconvs=True for every eligible transposed conv (`mx.native_tconv`) --, in
        one pass over `images` in the state the model is in (`reports.mx_native_report`)."""
        from .reports import mx_native_report
        return mx_native_report(self, images, act_fmt=act_fmt, batch=batch, units=units, convs=convs, tconvs=tconvs)

    def set_mx_activations(self, act_fmt, mode="native", units=None):
        """Run the modules' own forward on MX activations: every weighted QuantModule of the chosen units (`units`: a list of names of
        `units()`, None for all) that `mx.native_refusal`, `native_conv_refusal` or `native_tconv_refusal` accepts gets the plain
        attribute `mx_activations = (act_fmt, mode)`.  Its no-grad forward, while `use_weight_quant` is on, then takes the
        pre-activation output from its input quantised to the MX format `act_fmt` in blocks of 32 along the input channels --
        mode 'native': the MX codes of input and weight on the block-scaled matrix instruction (`mx.native_linear` / `native_conv` /
        `native_tconv`); mode 'emulated': the decoded input through the module's fp32 kernel -- followed by the module's tail
        (se_module, activation function, output quantiser), un-fused.  With `use_weight_quant` off the forward is what it was.
        act_fmt=None clears the attribute on every weighted module of the chosen units.  Whether a unit is trained does not matter.
        -> OrderedDict: 'native' module name -> 'linear' | 'conv' | 'tconv'; 'left' module name -> why the module keeps its forward
        (GDN, LayerNorm, a 3-channel stem, ragged channel counts, a weight that is in no MX format).
        ValueError before anything is written for an unknown act_fmt or mode, an unknown unit, and (act_fmt not None) a named unit
        without an eligible module.  An input that requires grad raises NotImplementedError in a switched module; `reconstruct`
        refuses a model that holds one."""
        from collections import OrderedDict
        from . import mx
        from hipops import ops
        what, known = "set_mx_activations", self.units()
        if act_fmt is not None:
            ops.mx_format(what, act_fmt)
        if not isinstance(mode, str) or mode not in mx.MX_ACT_MODES:
            raise ValueError(f"{what}: mode must be one of {list(mx.MX_ACT_MODES)}, got {mode!r}")
        if units is None:
            chosen = list(known)
        else:
            if isinstance(units, (str, bytes)) or not hasattr(units, "__iter__"):
                raise ValueError(f"{what}: units must be None or a list of unit names, got {units!r}")
            chosen = list(units)
            unknown = [n for n in chosen if n not in known]
            if unknown:
                raise ValueError(f"{what}: unknown unit name(s) {unknown}; QuantModel.units() has {list(known)}")
        rep = OrderedDict(native=OrderedDict(), left=OrderedDict())
        plan = []
        for uname in chosen:
            found = False
            for mn, m in known[uname].named_modules():
                if not isinstance(m, QuantModule) or m.org_weight is None:
                    continue
                name = f"{uname}.{mn}" if mn else uname
                kind, why = mx.native_kind(m)
                plan.append((m, kind))
                if kind is None:
                    rep["left"][name] = why
                else:
                    rep["native"][name], found = kind, True
            if units is not None and act_fmt is not None and not found:
                raise ValueError(f"{what}: unit {uname!r} holds no eligible module: "
                                 f"{ {n: w for n, w in rep['left'].items() if n == uname or n.startswith(uname + '.')} }")
        for m, kind in plan:
            m.mx_activations = None if (act_fmt is None or kind is None) else (act_fmt, mode)
        return rep

    def set_weight_format(self, formats, rounding="nearest"):
        """Leave the weights of the units in an MX block format: `formats` is one name for every unit, or a mapping unit
        name -> name (units it does not name keep theirs); a name is one of `hipops._lib.MX_FORMATS` or 'int'.  A format swaps the
        `weight_quantizer` of every weighted QuantModule of the unit for an `mx.MXQuantizer` and keeps the replaced quantiser on the
        module (`int_weight_quantizer`); 'int' puts that object back (a unit that holds no MX quantiser is left alone).  Names are
        validated and a unit that holds a trained module is refused (ValueError) before anything is written; every swap calls
        `drop_weight_pack()`.  Activation quantisers are not touched.

        rounding: 'nearest' (default: round to nearest, for evaluation) or 'learned' -- the unit gets `mx.MXAdaRoundQuantizer`s, which
        round to nearest until `block_reconstruction` / `layer_reconstruction` has learned the rounding of the unit on its MX grid.
        Anything else is a ValueError before anything is written.  Both classes swap back and re-swap alike."""
        from .mx import MX_FORMATS, MX_ROUNDINGS, MXAdaRoundQuantizer, MXQuantizer, is_mx_any as is_mx
        what, known = "set_weight_format", self.units()
        if not isinstance(rounding, str) or rounding not in MX_ROUNDINGS:
            raise ValueError(f"{what}: rounding must be one of {list(MX_ROUNDINGS)}, got {rounding!r}")
        make = MXAdaRoundQuantizer if rounding == "learned" else MXQuantizer
        plan = format_plan(what, known, formats, MX_FORMATS + ("int",))
        for n, _ in plan:
            if any(is_trained(m) for m in weighted_modules(known[n])):
                raise ValueError(f"{what}: unit {n!r} holds a trained module: its rounding belongs to the grid it was calibrated on")
        for n, fmt in plan:
            for m in weighted_modules(known[n]):
                q = m.weight_quantizer
                if fmt == "int":
                    if not is_mx(q):
                        continue
                    m.weight_quantizer = m.int_weight_quantizer
                    del m.int_weight_quantizer
                else:
                    if not is_mx(q):
                        m.int_weight_quantizer = q
                    m.weight_quantizer = make(fmt, tconv=m.if_tconv)
                m.drop_weight_pack()

    def weight_bits(self):
        """OrderedDict unit name -> {'bits': OrderedDict module name (inside the unit; '' for a layer unit) -> n_bits, 'weights': the
        unit's weight elements, 'size_bits': sum of n_bits x elements}, and 'total' -> {'weights', 'size_bits', 'avg_bits'}."""
        from collections import OrderedDict
        out = OrderedDict()
        tw = ts = 0
        for name, u in self.units().items():
            row = {"bits": OrderedDict(), "weights": 0, "size_bits": 0}
            for mn, m in u.named_modules():
                if isinstance(m, QuantModule) and m.org_weight is not None:
                    b, cnt = int(m.weight_quantizer.n_bits), int(m.weight.numel())
                    row["bits"][mn] = b
                    row["weights"] += cnt
                    row["size_bits"] += b * cnt
            out[name] = row
            tw, ts = tw + row["weights"], ts + row["size_bits"]
        out["total"] = {"weights": tw, "size_bits": ts, "avg_bits": ts / tw if tw else 0.0}
        return out

    def act_width_report(self, images, widths=(4, 6, 8), batch=8):
        """The one-pass screening table of activation widths: per site, the error of its grid at each of several widths, from one pass
        of the quantised model over `images` (`export.act_width_report`)."""
        from .reports import act_width_report
        return act_width_report(self, images, widths=widths, batch=batch)

    def act_bit_report(self, images, widths=(4, 6, 8), lmbda=0.01, weight_quant=False, batch=8, units=None):
        """What every unit costs in rate and distortion at each of several activation widths when its activation quantisers alone are
        on, with each width's size and activation error: the table `export.allocate_act_bits` chooses from (`export.act_bit_report`).
        len(units) * len(widths) + 1 passes over `images`; taken on a calibrated model."""
        from .reports import act_bit_report
        return act_bit_report(self, images, widths=widths, lmbda=lmbda, weight_quant=weight_quant, batch=batch, units=units)

    def set_act_bits(self, bits):
        """Give the activation grids of the units their widths: `bits` is one whole number in 2 .. MAX_BITS for every unit, or a mapping
        unit name -> width (what `export.allocate_act_bits(...)['bits']` is; units it does not name keep theirs).  Names and widths are
        validated before anything is written; then every activation quantiser of each named unit (the `act_quantizer` of each
        QuantModule / BaseQuantBlock in it) gets `dynamic_bits = b`, and its `act_stats` (measured at the old width) are dropped.
        Frozen ranges stay as they are.  Allowed before and after calibration: an activation width carries no rounding state.  Weight
        quantisers are not touched."""
        known = self.units()
        for n, b in width_plan("set_act_bits", known, bits):
            for _, m in act_modules(known[n]):
                m.act_quantizer.dynamic_bits = int(b)
                m.act_quantizer.act_stats = {}

    def act_bits(self):
        """OrderedDict unit name -> {'bits': OrderedDict module name (inside the unit; '' for the unit itself) -> dynamic_bits of its
        activation quantiser, 'applied': the module names whose quantiser a forward with act_quant=True applies (trained, not
        disabled)}."""
        from collections import OrderedDict
        out = OrderedDict()
        for name, u in self.units().items():
            ms = act_modules(u)
            out[name] = {"bits": OrderedDict((mn, int(getattr(m.act_quantizer, "dynamic_bits", 8))) for mn, m in ms),
                         "applied": [mn for mn, m in ms if act_applied(m)]}
        return out

    def save_packed(self, path):
        """Write the packed checkpoint of this model: every weight's integer levels packed at their own width, the grids, the biases
        and the frozen activation ranges -- no fp32 weight (`packed.save_packed`).  -> the sizes written."""
        from .packed import save_packed
        return save_packed(self, path)

    def load_packed(self, path):
        """Install a packed checkpoint into this model, which must be of the file's architecture and not calibrated; it then computes bit
        for bit what the saved model computed (`packed.load_packed`).  A refusal leaves the model as it was."""
        from .packed import load_packed
        return load_packed(self, path)

    def save_mx_packed(self, path):
        """Write the packed checkpoint of a model whose weights stand on MX block formats, on integer grids, or on both: per MX module
        the element codes packed at their own width and the blocks' scale bytes, learned rounding included -- no fp32 weight
        (`mx_packed.save_mx_packed`).  -> the sizes written."""
        from .mx_packed import save_mx_packed
        return save_mx_packed(self, path)

    def load_mx_packed(self, path):
        """Install a checkpoint of `save_mx_packed` into this model, which must be of the file's architecture, on the GPU and not
        calibrated; it then computes bit for bit what the saved model computed (`mx_packed.load_mx_packed`).  A refusal leaves the
        model as it was."""
        from .mx_packed import load_mx_packed
        return load_mx_packed(self, path)

    def forward(self, input):
        return self.model(input)

    def aux_loss(self):
        return sum(m.loss() for m in self.modules() if isinstance(m, EntropyBottleneck))

    def set_first_last_layer_to_8bit(self):
        mods = self._quant_modules()
        mods[0].weight_quantizer.bitwidth_refactor(8)
        mods[0].act_quantizer.bitwidth_refactor(8)
        mods[-1].weight_quantizer.bitwidth_refactor(8)
        mods[-2].act_quantizer.bitwidth_refactor(8)

    def disable_network_output_quantization(self):
        self._quant_modules()[-1].disable_act_quant = True
