"""`QuantModel`: module surgery that wraps a LIC model's layers in QuantModule / quant blocks
(reference surface: quantization/quant_model.py:10-98)."""
import torch.nn as nn

from lic import EntropyBottleneck

from .fold_bn import search_fold_and_remove_bn
from .quant_block import BaseQuantBlock, specials
from .quant_layer import GDN_TYPES, QuantModule, StraightThrough

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
        from .export import activation_report
        return activation_report(self)

    def unit_report(self):
        """OrderedDict unit name -> the measured output error of every calibrated unit that recorded it (args.unit_report): per output
        channel, learned rounding against round-to-nearest (`export.unit_report`)."""
        from .export import unit_report
        return unit_report(self)

    def bias_report(self):
        """OrderedDict unit name -> what the bias correction of every unit that ran it did (args.bias_correct): the corrected layers'
        shifts and the unit's output error before and after (`export.bias_report`)."""
        from .export import bias_report
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
        from .export import rd_report
        return rd_report(self, images, lmbda=lmbda, act_quant=act_quant, batch=batch, units=units)

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
