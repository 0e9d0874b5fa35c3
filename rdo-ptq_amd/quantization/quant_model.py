"""`QuantModel`: module surgery that wraps a LIC model's layers in QuantModule / quant blocks
(reference surface: quantization/quant_model.py:10-98)."""
import torch.nn as nn

from lic import EntropyBottleneck

from .fold_bn import search_fold_and_remove_bn
from .quant_block import BaseQuantBlock, QuantRB, QuantRBWS, QuantSwinTransformerBlock, QuantWindowAttention, specials
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

    def set_mx_activations(self, act_fmt, mode="native", units=None, chain=False, gdn=False, swin=False, attention=False, p_fmt=None, fused_attention=False,
                           residual_units=False):
        """Run the modules' own forward on MX activations: every weighted QuantModule of the chosen units (`units`: a list of names of
        `units()`, None for all) that `mx.native_refusal`, `native_conv_refusal` or `native_tconv_refusal` accepts gets the plain
        attribute `mx_activations = (act_fmt, mode)`.  Its no-grad forward, while `use_weight_quant` is on, then takes the
        pre-activation output from its input quantised to the MX format `act_fmt` in blocks of 32 along the input channels --
        mode 'native': the MX codes of input and weight on the block-scaled matrix instruction (`mx.native_linear` / `native_conv` /
        `native_tconv`); mode 'emulated': the decoded input through the module's fp32 kernel -- followed by the module's tail
        (se_module, activation function, output quantiser), un-fused.  With `use_weight_quant` off the forward is what it was.
        act_fmt=None clears the attribute on every weighted module of the chosen units.  Whether a unit is trained does not matter.
        -> OrderedDict: 'native' module name -> 'linear' | 'conv' | 'tconv' (| 'gdn'); 'left' module name -> why the module keeps its forward
        (GDN, LayerNorm, a 3-channel stem, ragged channel counts, a weight that is in no MX format).
        chain=True (mode 'native' only) also sets the plain attribute `mx_chain` on every `QuantRB` / `QuantRBWS` block of the chosen
        units whose (conv1, conv2) `mx.native_chain_refusal` accepts: its no-grad forward then runs the pair as `mx.native_chain` --
        conv1 writes LReLU(conv1(x)) packed in act_fmt, conv2 reads it; the same bits in three launches instead of five -- while both
        convs carry this (act_fmt, 'native'), `use_weight_quant` is on and the block's activation quantiser is inactive.  The result
        then gains 'chained': block name -> (conv1 name, conv2 name).  chain=False and act_fmt=None clear `mx_chain` on the chosen units'
        blocks.  `mx_chain` is not stored by `save_mx_packed`: a loaded model is un-chained and computes the same bits.
        gdn=True also switches every GDN / IGDN module `mx.native_gdn_refusal` accepts, reported under 'native' as 'gdn': mode 'native'
        runs `mx.native_gdn` (one launch, the norm pool on the block-scaled instruction from the squares quantised to act_fmt and
        gamma' re-quantised onto the MX grid), mode 'emulated' the fp32 GDN kernel on the decoded operands.  gdn=False (the default)
        leaves every GDN under 'left' as before.
        swin=True (mode 'native' only) also sets the plain attribute `mx_swin` on every `QuantSwinTransformerBlock` of the chosen units that
        `mx.native_swin_refusal` accepts: its no-grad forward then runs norm1 -> qkv as `mx.native_ln_linear` (two launches instead of
        three) and everything behind the attention as one `mx.native_swin_mlp` launch instead of eight, while qkv, fc1 and fc2 carry this
        (act_fmt, 'native'), `use_weight_quant` is on and no activation quantiser rounds in between.  The result gains 'swin': block
        name -> (norm2, fc1, fc2 names); the block's norm1 / norm2 are reported under 'native' as 'layernorm', a refused block under
        'left' with the reason.  swin=False and act_fmt=None clear `mx_swin`; it is not stored by `save_mx_packed`.
        attention=True (mode 'native' only; independent of swin) also sets the plain attribute `mx_attention = (act_fmt, p_fmt)` (p_fmt None:
        act_fmt) on every `QuantWindowAttention` of the chosen units that `mx.native_attention_refusal` accepts and whose qkv is switched:
        its no-grad forward then runs Q K^T, the softmax and P V as one `mx.native_attention` launch -- Q, K and V quantised to act_fmt, the
        probabilities to p_fmt, both products on the block-scaled matrix instruction -- while qkv carries this (act_fmt, 'native') and
        `use_weight_quant` is on.  A switched attention does NOT compute what the fp32 attention computes: four more tensors are rounded.
        The result gains 'attention': attention name -> (act_fmt, p_fmt); a refused one goes under 'left' with the reason.
        attention=False and act_fmt=None clear `mx_attention`; it is not stored by `save_mx_packed`.
        fused_attention=True (needs swin=True and attention=True, and p_fmt None or act_fmt) also sets the plain attribute `mx_swin_attn` on
        every accepted Swin block that `mx.native_swin_attn_refusal` accepts too: its no-grad forward then runs norm1, qkv, the attention
        core, proj and the residual add as one `mx.native_swin_attn` launch instead of five, so the block is two launches, with the bits of
        the five -- while the conditions of swin and attention hold and proj carries this (act_fmt, 'native').  The result gains
        'swin_attn': block name -> (norm1, qkv, proj names); a refused block keeps the five launches and goes under 'left' with the
        reason.  Cleared like `mx_swin`; not stored by `save_mx_packed`.  Measured at the Lu2022 width (B = 4, 128 x 128, C = 192, 8 heads,
        window 8, shift 0 and 4, FP8 and FP4; profiles/mx_swin_attn_bench.log): the one launch is SLOWER at every one
        of those shapes, 2.05-2.18 x the five launches' time -- one workgroup a CU by LDS.  The keyword is for a forward in two launches
        a block with the same bits, not for speed; it is off by default.
        residual_units=True (mode 'native' only) also sets the plain attribute `mx_resunit` on every `_ResidualUnit` of an `AttentionBlock`
        (Cheng2020-attn) whose three convs are among the chosen units and switched and which `mx.native_residual_unit_refusal` accepts: its
        no-grad forward then runs relu(x + conv1x1(relu(conv3x3(relu(conv1x1(x)))))) as one `mx.native_residual_unit` launch instead of
        eleven (three per conv, the eager add and ReLU), the two intermediate tensors packed in LDS, with the bits of the eleven -- while
        the three convs carry this (act_fmt, 'native'), `use_weight_quant` is on, no activation quantiser rounds on them and the input is
        not tracked.  The result gains 'residual_units': unit name -> the three conv names; a refused unit goes under 'left' with the
        reason.  residual_units=False and act_fmt=None clear `mx_resunit`; it is not stored by `save_mx_packed`.  An input that is
        not a channels-last view costs one layout copy before the launch; switched units hand each other channels-last views.  Measured
        against the six `ops` launches the kernel is bit for bit (B = 4, 16 x 16 and 64 x 64, N = 128 and 192, FP8 and FP4;
        profiles/mx_resunit_bench.log): called from Python 0.49-0.94 x their time (1.04 x for FP8 at N = 192, 64 x
        64), which is the host issuing one launch for six; both replayed as graphs, kernels only, the one launch is SLOWER at six of the
        eight shapes (1.09-2.06 x) and faster only at N = 128, 64 x 64 (0.82 x).  The keyword is for a unit in one launch with the same
        bits, not for a faster kernel; it is off by default.
        ValueError before anything is written for an unknown act_fmt, p_fmt or mode, a residual_units that is no bool or is True in another
        mode than 'native', a fused_attention that is no bool, is True without
        swin=True and attention=True or with a p_fmt other than act_fmt, an unknown unit, a gdn that is no bool, a chain, swin
        or attention that is no bool or is True in another mode than 'native', a p_fmt without attention=True, and (act_fmt not None) a named unit without an eligible module.  An input that requires grad raises NotImplementedError in a switched module; `reconstruct`
        refuses a model that holds one."""
        from collections import OrderedDict
        from . import mx
        from hipops import ops
        from lic.layers import _ResidualUnit
        what, known = "set_mx_activations", self.units()
        if act_fmt is not None:
            ops.mx_format(what, act_fmt)
        if not isinstance(mode, str) or mode not in mx.MX_ACT_MODES:
            raise ValueError(f"{what}: mode must be one of {list(mx.MX_ACT_MODES)}, got {mode!r}")
        if not isinstance(chain, bool) or (chain and mode != "native"):
            raise ValueError(f"{what}: chain must be True or False, and True in mode 'native' only; got chain={chain!r}, mode={mode!r}")
        if not isinstance(gdn, bool):
            raise ValueError(f"{what}: gdn must be True or False, got {gdn!r}")
        if not isinstance(swin, bool) or (swin and mode != "native"):
            raise ValueError(f"{what}: swin must be True or False, and True in mode 'native' only; got swin={swin!r}, mode={mode!r}")
        if not isinstance(attention, bool) or (attention and mode != "native"):
            raise ValueError(f"{what}: attention must be True or False, and True in mode 'native' only; got attention={attention!r}, mode={mode!r}")
        if p_fmt is not None:
            ops.mx_format(what, p_fmt)
            if not attention:
                raise ValueError(f"{what}: p_fmt={p_fmt!r} is the format of the attention's probabilities and needs attention=True")
        if not isinstance(fused_attention, bool) or (fused_attention and not (swin and attention and p_fmt in (None, act_fmt))):
            raise ValueError(f"{what}: fused_attention must be True or False, and True only with swin=True, attention=True and a p_fmt that is "
                             f"None or act_fmt; got fused_attention={fused_attention!r}, swin={swin!r}, attention={attention!r}, p_fmt={p_fmt!r}")
        if not isinstance(residual_units, bool) or (residual_units and mode != "native"):
            raise ValueError(f"{what}: residual_units must be True or False, and True in mode 'native' only; got residual_units={residual_units!r}, "
                             f"mode={mode!r}")
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
        if chain:
            rep["chained"] = OrderedDict()
        if swin:
            rep["swin"] = OrderedDict()
        if attention:
            rep["attention"] = OrderedDict()
        if fused_attention:
            rep["swin_attn"] = OrderedDict()
        plan, blocks, swin_blocks, swin_norms, attentions = [], [], [], set(), []
        for uname in chosen:
            found = False
            for mn, m in known[uname].named_modules():
                name = f"{uname}.{mn}" if mn else uname
                if isinstance(m, (QuantRB, QuantRBWS)):
                    on = chain and act_fmt is not None and mx.native_chain_refusal(m.conv1, m.conv2) is None
                    blocks.append((m, on))
                    if on:
                        rep["chained"][name] = (f"{name}.conv1", f"{name}.conv2")
                if isinstance(m, QuantSwinTransformerBlock):
                    why = mx.native_swin_refusal(m) if (swin and act_fmt is not None) else "not asked for"
                    fused = why is None and fused_attention
                    if why is None:
                        rep["swin"][name] = (f"{name}.norm2", f"{name}.mlp.fc1", f"{name}.mlp.fc2")
                        swin_norms.update((f"{name}.norm1", f"{name}.norm2"))
                    elif swin and act_fmt is not None:
                        rep["left"][name] = why
                    if fused:
                        why_not = mx.native_swin_attn_refusal(m)
                        fused = why_not is None
                        if fused:
                            rep["swin_attn"][name] = (f"{name}.norm1", f"{name}.attn.qkv", f"{name}.attn.proj")
                        else:
                            rep["left"][name] = f"the attention half keeps its five launches: {why_not}"
                    swin_blocks.append((m, why is None, fused))
                if isinstance(m, QuantWindowAttention):
                    why = "not asked for"
                    if attention and act_fmt is not None:
                        why = mx.native_attention_refusal(m)
                        if why is None and mx.native_refusal(m.qkv) is not None:
                            why = f"qkv keeps its fp32 operands: {mx.native_refusal(m.qkv)}"
                        if why is None:
                            rep["attention"][name] = (act_fmt, act_fmt if p_fmt is None else p_fmt)
                        else:
                            rep["left"][name] = why
                    attentions.append((m, rep["attention"][name] if why is None else None))
                if not isinstance(m, QuantModule) or m.org_weight is None:
                    continue
                if name in swin_norms:                  # the LayerNorms of an accepted block run inside its fused launches
                    rep["native"][name] = "layernorm"
                    plan.append((m, None))
                    continue
                kind, why = mx.native_kind(m)
                if gdn and m.kind == "gdn":
                    why = mx.native_gdn_refusal(m)
                    kind = "gdn" if why is None else None
                plan.append((m, kind))
                if kind is None:
                    rep["left"][name] = why
                else:
                    rep["native"][name], found = kind, True
            if units is not None and act_fmt is not None and not found:
                raise ValueError(f"{what}: unit {uname!r} holds no eligible module: "
                                 f"{ {n: w for n, w in rep['left'].items() if n == uname or n.startswith(uname + '.')} }")
        resunits = []
        if residual_units:
            rep["residual_units"] = OrderedDict()
        for rname, r in self.model.named_modules():
            names = tuple(f"{rname}.conv.{i}" for i in (0, 2, 4))
            if not isinstance(r, _ResidualUnit) or not any(n in chosen for n in names):
                continue
            why = "not asked for"
            if residual_units and act_fmt is not None:
                why = mx.native_residual_unit_refusal(r)
                if why is None and not all(n in chosen and n in rep["native"] for n in names):
                    why = "its three convs are not all among the chosen units and switched"
                if why is None:
                    rep["residual_units"][rname] = names
                else:
                    rep["left"][rname] = why
            resunits.append((r, why is None))
        for m, kind in plan:
            m.mx_activations = None if (act_fmt is None or kind is None) else (act_fmt, mode)
        for b, on in blocks:
            b.mx_chain = on
        for b, on, fused in swin_blocks:
            b.mx_swin, b.mx_swin_attn = on, fused
        for a, on in attentions:
            a.mx_attention = on
        for r, on in resunits:
            r.mx_resunit = on
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
