"""What runs on a unit after its rounding has been learned; none of it is in the reference.  `recon._reconstruct` calls the five passes:
`correct_unit_bias`, `calibrate_act_ranges` (then `learn_act_ranges`), `report_act_ranges`, `report_unit`.

Each pass is built from the same pieces: `utils.quant_state` (the flags of the unit's modules, put back whatever happens),
`_run_unit` (the unit over a cached input tensor, batch by batch without a tape), `_output_moments` (its output against the cached
full-precision one), `_act_quantizers` / `_sites` (the activation quantisers and their sites in the order every collective relies on)
and `_rank_sums` (device sums and host counts over the ranks)."""
from collections import OrderedDict

import torch

from . import dp
from hipops import ops
from .quant_block import BaseQuantBlock, QuantRSTB
from .quant_layer import QuantModule, _nhwc, _sq
from .quantizer import AdaRoundQuantizer, to_rows
from .utils import distinct, quant_state

BIAS_CORRECT_MODES = ("weight", "output")
_MOMENTS = ("shift", "err", "energy")          # the rows of `ops.pair_moments`


def _check_learn(iters, lr):
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"act_iters must be a positive integer, got {iters!r}")
    if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not (0.0 < float(lr) < float("inf")):
        raise ValueError(f"act_lr must be a positive finite number, got {lr!r}")
    return iters, float(lr)


def _check_percentile(p):
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not (50.0 < float(p) <= 100.0):
        raise ValueError(f"act_percentile must be a number p with 50 < p <= 100, got {p!r}")
    return float(p)


def _is_rstb(unit):
    return isinstance(unit, QuantRSTB) or getattr(unit, "unit_kind", None) == "rstb"


def _run_unit(unit, x, batch, each=None):
    """One pass of `unit` over the cached inputs `x`, batch by batch and without a tape; `each(row slice, unit output)` sees every batch
    (without it the pass is for what the unit's quantisers and hooks take from it)."""
    rstb = isinstance(unit, QuantRSTB)
    with torch.no_grad():
        for i in range(0, x.shape[0], batch):
            h = x[i:i + batch]
            out = unit(h, (h.shape[2], h.shape[3])) if rstb else unit(h)
            if each is not None:
                each(slice(i, i + batch), out)
            del out                                              # (not held while the next batch runs)


def _output_moments(unit, inp_q, out_fp, batch):
    """-> (float64 [3, C] device sums shift | err | energy of `ops.pair_moments(out_fp batch, output batch)` over one pass on `inp_q`:
    the fp32 sums of the batches added in float64 in batch order; the pixels per channel)"""
    # (zero sums, not None: a rank with no rows still takes part in the collectives of its caller)
    acc, n = torch.zeros(3, out_fp.shape[1], dtype=torch.float64, device=out_fp.device), 0

    def add(rows, out):
        nonlocal acc, n
        ref = _nhwc(out_fp[rows])
        acc = acc + ops.pair_moments(ref, _nhwc(out)).double()
        n += ref.numel() // ref.shape[-1]
    _run_unit(unit, inp_q, batch, add)
    return acc, n


def _moment_fields(acc):
    return {f: v for f, v in zip(_MOMENTS, acc.cpu())}


def _rank_sums(sums, counts, device, dtype=torch.int64):
    """SUM over the ranks in one call: the tensors `sums` in place, in their order, then the host integers `counts` as one `dtype`
    tensor on `device` -> the counts over all ranks.  In one process nothing is launched and nothing is read back."""
    if dp.world()[1] <= 1:
        return list(counts)
    t = torch.tensor(list(counts), dtype=dtype, device=device)
    dp.reduce_act_stats(sums=list(sums) + [t])
    return [int(v) for v in t.tolist()]


def _act_quantizers(mods, frozen=False):
    """the distinct activation quantisers of the QuantModules and block wrappers `mods` (`quant_state.mods`: module order); `frozen`:
    those with frozen ranges only"""
    return [q for q in distinct(m.act_quantizer for m in mods) if not frozen or q.act_frozen()]


def _sites(quants, name):
    """[(quantiser, site)] over the sites of the per-site dict `name`, in a fixed order: the collectives of all ranks must line up"""
    return [(q, k) for q in quants for k in sorted(getattr(q, name))]


def _site_values(quants, name):
    return [getattr(q, name)[k] for q, k in _sites(quants, name)]


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
    with quant_state(unit, True, True) as state:
        quants = _act_quantizers(state.mods)
        for q in quants:
            q.act_observe()
        _run_unit(unit, inp_q, batch)
        dp.reduce_act_stats(ranges=_site_values(quants, "act_range"))
        seen = [q for q in quants if q.act_range]
        if act_range == "l2":
            for q in seen:
                q.act_search()
            _run_unit(unit, inp_q, batch)
            dp.reduce_act_stats(sums=_site_values(quants, "act_err"))
        elif act_range in ("percentile", "hist_mse"):
            for q in seen:
                q.act_histogram(percentile, rule="mse" if act_range == "hist_mse" else "percentile")
            _run_unit(unit, inp_q, batch)
            dp.reduce_act_stats(sums=_site_values(quants, "act_hist"))
        elif act_range == "auto":
            for q in seen:
                q.act_histogram(percentile, rule="mse", search=True)
            _run_unit(unit, inp_q, batch)
            dp.reduce_act_stats(sums=_site_values(quants, "act_err") + _site_values(quants, "act_hist"))
            for q in seen:
                q.act_score(q.act_candidates())
            _run_unit(unit, inp_q, batch)
            _reduce_scores(seen)
        for q in quants:
            q.act_freeze(keep_obs=keep_obs)


def _reduce_scores(quants):
    """the sums, counts and pixel counts of a scoring pass over the ranks, in the fixed site order"""
    if dp.world()[1] <= 1:
        return
    dp.reduce_act_stats(sums=_site_values(quants, "act_err") + _site_values(quants, "act_energy") + _site_values(quants, "act_clip"))
    sites = _sites(quants, "act_score_n")
    if sites:
        device = sites[0][0].act_err[sites[0][1]].device
        counts = _rank_sums([], [q.act_score_n[k] for q, k in sites], device, torch.int32)     # (the guard of the pass keeps the sum inside 32 bits)
        for (q, k), v in zip(sites, counts):
            q.act_score_n[k] = v


def report_act_ranges(unit, inp_q, batch=32):
    """Measure the frozen static activation ranges of a calibrated unit: one pass over its cached quantised inputs in the W8A8 state, every
    frozen quantiser scoring its own range (K = 1) and passing its frozen output on; the measured squared error, the energy, the counts of
    the values clipped at each end and the pixel count stay on the quantiser as `act_stats[site]` (summed over the ranks under data
    parallelism).  The ranges do not change; every quant state flag is left as it was found."""
    with quant_state(unit, True, True) as state:
        quants = _act_quantizers(state.mods, frozen=True)
        try:
            for q in quants:
                q.act_score()
            _run_unit(unit, inp_q, batch)
            _reduce_scores(quants)
        finally:
            for q in quants:
                if getattr(q, "act_phase", "idle") == "score":
                    q.act_freeze()


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
    adas = [(m, m.weight_quantizer) for m in unit.modules()
            if isinstance(m, QuantModule) and isinstance(m.weight_quantizer, AdaRoundQuantizer)]
    held = [(q, q.alpha) for _, q in adas]
    try:
        for m, q in adas:
            q.alpha = torch.nn.Parameter(_nearest_alpha(q, m.weight), requires_grad=q.alpha.requires_grad)
            m.drop_weight_pack()
        nearest, n = _output_moments(unit, inp_q, out_fp, batch)
    finally:
        for (m, _), (q, alpha) in zip(adas, held):
            q.alpha = alpha
            m.drop_weight_pack()
    learned, _ = _output_moments(unit, inp_q, out_fp, batch)
    n, = _rank_sums([nearest, learned], [n], nearest.device)
    unit.unit_stats = {"name": unit_name, "n": int(n), "nearest": _moment_fields(nearest), "learned": _moment_fields(learned)}
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
    with quant_state(m, weight=bool(quantised)):
        w = m._weights()[0].detach()
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
    names = {m: (n or "layer") for n, m in unit.named_modules() if isinstance(m, QuantModule)}
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
    ref_sums = {}
    # the full-precision pass ('output'), or a first quantised pass ('weight'), also fixes the order of the layers' first calls
    with quant_state(unit, mode != "output", False) as state:
        col = _TapCollector(layers, device, order_only=mode != "output")
        try:
            if mode == "output":
                _run_unit(unit, inp_fp, batch)                   # every S_ref in one pass
                col.close()
                state.set(True, False)
            before, n_out = _output_moments(unit, inp_q, out_fp, batch)
        finally:
            col.close()
        order = list(col.order) + [m for m in layers if m not in col.order]         # (no rows here: module order)
        if dp.world()[1] > 1:
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
            if order:
                dp.reduce_act_stats(sums=[ref_sums[m] for m in order])
        shifts = OrderedDict()
        for m in order:
            one = _TapCollector([m], device)
            try:
                _run_unit(unit, inp_q, batch)
            finally:
                one.close()
            s_q, n = one.get(m)
            n, = _rank_sums([s_q], [n], device)
            if n < 1:
                raise ValueError(f"correct_unit_bias: {unit_name}: no calibration rows reached {names[m]}")
            w_q = _bias_rows(m, True)
            w_ref = _bias_rows(m, False)
            shift, bias = ops.bias_shift(w_ref, w_q, ref_sums[m] if mode == "output" else s_q, s_q, n, m.org_bias.detach().float().contiguous())
            m.bias.data.copy_(bias)
            m.drop_weight_pack()              # (the memo keys on _version, which a .data write does not bump)
            m.bias_shift = shift.cpu()
            shifts[names[m]] = {"shift": m.bias_shift.clone(), "n": int(n), "kind": m.kind}
        after, _ = _output_moments(unit, inp_q, out_fp, batch)
        n_out, = _rank_sums([before, after], [n_out], device)
    unit.bias_stats = {"name": unit_name, "mode": mode, "n": int(n_out), "layers": shifts, "skipped": skipped,
                       "before": _moment_fields(before), "after": _moment_fields(after)}
    return unit.bias_stats


SWIN_LEARN_REFUSAL = ("a Swin (RSTB) unit learns its ranges only on request (learn_act_ranges(..., swin=True) / args.act_learn_swin=True: "
                      "every window attention of the unit then keeps two [windows, N, N, heads] tensors until the backward); "
                      "use act_range='max' or 'l2' for it otherwise")


def learn_act_ranges(unit, inp_q, out_fp, iters=500, lr=1e-3, batch=32, seed=0, idx_table=None, swin=False):
    """Train the frozen static activation ranges of a calibrated unit on its reconstruction error (the activation-grid step of BRECQ /
    QDrop, after the rounding has been learned).  The unit runs in the W8A8 state with its hard-rounded weights under torch's tape (the
    modules' tape forwards; every frozen quantiser as `ActQuantStaticFn`, straight-through round) on mini-batches inp_q[idx] of `batch`
    rows (never a ragged one; idx from a generator seeded with `seed`, or the rows of `idx_table` [iters, batch]); the loss is
    lp_loss(out, out_fp[idx], p=2); every site range the forward reached takes one projected Adam step per iteration
    (`ops.act_range_step`: step size relative to the observed width, the range stays inside the observed max range).  Under data
    parallelism the range gradients of all sites, concatenated in the fixed site order of `calibrate_act_ranges`, are summed over the
    ranks and divided by the world size before the step, so every rank holds the same grids.  The quantisers end frozen; every quant
    state flag is left as it was found.  A Swin (RSTB) unit is refused unless `swin` is True (a bool): its activation-quantised window
    attentions then run as `WindowAttentionProbsFn` -> quantiser -> `WindowAttentionPVFn` -> quantiser, the unit called as
    unit(x, (H, W))."""
    from hipops.autograd import SqDiffSumFn
    if not isinstance(swin, bool):
        raise ValueError(f"learn_act_ranges: swin must be True or False, got {swin!r}")
    rstb = _is_rstb(unit)
    if rstb and not swin:
        raise NotImplementedError(f"learn_act_ranges: {SWIN_LEARN_REFUSAL}")
    iters, lr = _check_learn(iters, lr)
    n = inp_q.shape[0]
    B = max(1, min(int(batch), n))
    if idx_table is None:
        g = torch.Generator().manual_seed(int(seed))
        idx_table = torch.stack([torch.randperm(n, generator=g)[:B] for _ in range(iters)])
    if idx_table.dim() != 2 or idx_table.shape[0] < iters:
        raise ValueError(f"learn_act_ranges: idx_table must be [iters >= {iters}, batch], got {tuple(idx_table.shape)}")
    idx_table = idx_table.to(device=inp_q.device, dtype=torch.long)
    world_size = dp.world()[1]
    with quant_state(unit, True, True) as state:
        quants = _act_quantizers(state.mods, frozen=True)
        try:
            for q in quants:
                q.act_learn()
            sites = _sites(quants, "act_range")
            moments = [(torch.zeros_like(q.act_obs[k]), torch.zeros_like(q.act_obs[k])) for q, k in sites]
            steps = [0] * len(sites)
            for it in range(iters):
                idx = idx_table[it]
                x = inp_q.index_select(0, idx).detach().requires_grad_(True)
                tgt = out_fp.index_select(0, idx)
                with torch.enable_grad():
                    out = unit(x, (x.shape[2], x.shape[3])) if rstb else unit(x)
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
