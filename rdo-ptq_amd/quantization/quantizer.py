"""Quantisers of the RDO-PTQ calibration path with the reference's class surface, computing through librdoptq_hip.

Mirrors /root/reference/task-oriented-PTQ/quantization/quantizer.py: `UniformAffineQuantizer` (:123-393),
`AdaRoundQuantizer` (:397-470), `ActQuantizer` (:81-121), `round_ste` (:64-68), `lp_loss` (:71-79),
`StraightThrough` (:12-17).  Weights are handed to the kernels in row-major "rows x inner" form where a row is one
quantisation channel: OHWI for conv weights (channel = dim 0), the matrix itself for GDN gammas / Linear weights.
There is no CPU implementation: tensors must live on the GPU."""
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from hipops import ops

GAMMA, ZETA = -0.1, 1.1
MAX_BITS = 16


class StraightThrough(nn.Module):
    def __init__(self, channel_num: int = 1):
        super().__init__()

    def forward(self, input):
        return input


def round_ste(x: torch.Tensor):
    return (x.round() - x).detach() + x


def lp_loss(pred, tgt, p=2.0, reduction="none"):
    diff = (pred - tgt).abs().pow(p)
    return diff.sum(1).mean() if reduction == "none" else diff.mean()


# ----------------------------------------------------------------------------- layout helpers
def to_rows(w: torch.Tensor, tconv: bool = False):
    """Weight (logical OIHW / [out,in] / 1-D) -> contiguous kernel layout whose dim 0 is the quantisation channel."""
    if w.dim() == 4:
        return (w.permute(1, 2, 3, 0) if tconv else w.permute(0, 2, 3, 1)).contiguous()   # tconv: channel = dim 1
    if w.dim() == 1:
        return w.reshape(1, -1).contiguous()
    return w.contiguous()


def from_rows(wr: torch.Tensor, like: torch.Tensor, tconv: bool = False):
    """Inverse of to_rows as a zero-copy view with the logical shape of `like`."""
    if like.dim() == 4:
        return wr.permute(3, 0, 1, 2) if tconv else wr.permute(0, 3, 1, 2)
    if like.dim() == 1:
        return wr.reshape(-1)
    return wr


def _scale_shape(w: torch.Tensor, tconv: bool):
    if w.dim() == 4:
        return (1, -1, 1, 1) if tconv else (-1, 1, 1, 1)
    if w.dim() == 1:
        return (-1,)
    return (-1, 1)


# ----------------------------------------------------------------------------- activation quantisation
def ActQuant(x: torch.Tensor, n_bits: int = 8):
    """Dynamic per-channel quant-dequant of a detached copy (channel = dim 1 for 4-D, last dim for 3-D, dim 1 for 2-D).
    The reference hard-wires 8 bits (`Handle_Parameter(param, b_w=8)`, quantizer.py:81) whatever --n_bits_a says; `n_bits` is
    the extension BASELINE config "W10A10" needs (UniformAffineQuantizer(dynamic_bits=10))."""
    x = x.detach()
    if x.dim() == 4:
        xr = x.permute(0, 2, 3, 1).contiguous()
        return ops.actquant_perchannel(xr, n_bits=n_bits).permute(0, 3, 1, 2)
    if x.dim() in (2, 3):
        return ops.actquant_perchannel(x.contiguous(), n_bits=n_bits)
    return ops.actquant_perchannel(x.reshape(-1, 1).contiguous(), n_bits=n_bits).reshape(x.shape)


def ActQuantizer(x: torch.Tensor, n_bits: int = 8):
    return ActQuant(x, n_bits)


def _act_rows(x: torch.Tensor, channels_last: bool = False):
    """x -> (contiguous channels-last tensor the kernels see, function taking a result back to x's layout); the channel rule of
    `ActQuant`.  `channels_last`: the last dim is the channel whatever the rank (the attention probabilities [B_, N, N, heads])."""
    x = x.detach()
    if channels_last or x.dim() in (2, 3):
        return x.contiguous(), (lambda y: y)
    if x.dim() == 4:
        return x.permute(0, 2, 3, 1).contiguous(), (lambda y: y.permute(0, 3, 1, 2))
    shape = x.shape
    return x.reshape(-1, 1).contiguous(), (lambda y: y.reshape(shape))


ACT_MODES = ("dynamic", "static")
ACT_HIST_RULES = ("percentile", "mse")      # what `act_freeze` selects from a histogram pass
ACT_AUTO_CANDIDATES = ("max", "l2", "percentile", "hist_mse")      # the rows of `act_candidates`, in the order that breaks ties


def act_l2_range(rng, err):
    """The range an 'l2' search freezes: each channel of the observed rng [2C] shrunk to its best candidate lo * s_k | hi * s_k of err
    [C, 10] (first minimum), an end that the scaling moved OUT of the observed range put back on it."""
    c = rng.numel() // 2
    table = torch.tensor([1.0 - 0.05 * i for i in range(ops.ACT_SEARCH_CANDIDATES)], dtype=torch.float32, device=rng.device)
    s = table[err.argmin(dim=1)]                                   # (float)(1 - 0.05 k): the kernel's factors
    lo, hi = torch.maximum(rng[:c] * s, rng[:c]), torch.minimum(rng[c:] * s, rng[c:])
    keep = lo > hi                                                 # (a candidate that left the observed range altogether)
    return torch.cat([torch.where(keep, rng[:c], lo), torch.where(keep, rng[c:], hi)])


def act_score_winner(err):
    """err [C, K] (measured error sums) -> long [C]: the row of the smallest sum; among equal sums the earliest row; a NaN sum never
    wins; a channel whose sums are all NaN gets row 0 (the max range).  Written out: `torch.argmin` does not promise the first index."""
    best = torch.full((err.shape[0],), float("inf"), dtype=err.dtype, device=err.device)
    win = torch.zeros(err.shape[0], dtype=torch.long, device=err.device)
    found = torch.zeros(err.shape[0], dtype=torch.bool, device=err.device)
    for k in range(err.shape[1]):
        e = err[:, k]
        better = ~torch.isnan(e) & (~found | (e < best))
        best, win, found = torch.where(better, e, best), torch.where(better, torch.full_like(win, k), win), found | better
    return win


# ----------------------------------------------------------------------------- uniform affine quantiser
class UniformAffineQuantizer(nn.Module):
    """Asymmetric uniform fake-quantiser; scales are initialised lazily on the first weight it sees."""

    def __init__(self, n_bits: int = 8, symmetric: bool = False, channel_wise: bool = False, scale_method: str = "max",
                 leaf_param: bool = False, tconv: bool = False, act: bool = False, prob: float = 1.0,
                 dynamic_bits: int = None, act_mode: str = "dynamic"):
        super().__init__()
        # width of the dynamic activation grid: None = the reference's fixed 8 bits (its ActQuant ignores n_bits_a,
        # quantizer.py:81,158-159); an explicit value is this build's extension (e.g. 10 for W10A10)
        assert dynamic_bits is None or 2 <= dynamic_bits <= MAX_BITS, "bitwidth not supported"
        self.dynamic_bits = 8 if dynamic_bits is None else int(dynamic_bits)
        # the reference stops at 8 bits (quantizer.py:139); BASELINE config 3 (W10A10) needs wider weight grids, which the
        # kernels handle unchanged (levels are fp32-valued integers): accepted up to 16 bits as an extension
        assert 2 <= n_bits <= MAX_BITS, "bitwidth not supported"
        self.sym = symmetric
        self.n_bits = n_bits
        self.n_levels = 2 ** n_bits
        self.delta = None
        self.zero_point = None
        self.inited = False
        self.leaf_param = leaf_param
        self.channel_wise = channel_wise
        self.scale_method = scale_method
        self.tconv = tconv
        self.act = act
        self.prob = prob
        self.is_training = False
        # activation grids: "dynamic" = the reference's ActQuant (min / max of the very tensor being quantised); "static" = per-channel
        # ranges frozen from the calibration set (an extension; recon.py drives observing -> (searching ->) frozen).  One quantiser
        # object may sit at several places of its block (`site`): each place has its own range [2C] = lo | hi in `act_range`.
        if act_mode not in ACT_MODES:
            raise ValueError(f"unknown act_mode {act_mode!r} {ACT_MODES}")
        self.act_mode = act_mode
        # static only: "idle" (no range yet) | "observe" | "search" | "hist" | "search+hist" | "score" | "frozen" | "learn"
        self.act_phase = "idle"
        self.act_range = {}                # site -> fp32 [2C], lo | hi (leaf tensors with requires_grad while learning)
        self.act_err = {}                  # site -> fp32 [C, 10] while searching
        self.act_obs = {}                  # site -> fp32 [2C]: the observed max range, kept for / while learning the ranges
        # site -> int32 [C, 1024] while the percentile histograms are taken (`act_tail` = 1 - p / 100; `act_hist_n`: pixels counted per
        # site, on the host).  Absent on models pickled before they existed: read with getattr
        self.act_hist = {}
        self.act_tail = 0.0
        self.act_hist_n = {}
        # which selection follows the histogram pass: "percentile" | "mse" (ACT_HIST_RULES).  Absent on models pickled before it existed:
        # read with getattr, as "percentile"
        self.act_hist_rule = "percentile"
        # frozen ranges on torch's tape (hipops.autograd.ActQuantStaticFn, straight-through round) when the input is tracked: set by
        # recon.reconstruct for the duration of an R + lambda*D unit.  Absent on models pickled before it existed: read with getattr
        self.act_ste = False
        # the scoring pass (`act_score`): site -> candidate grids fp32 [K, 2C], measured error sums `act_err` [C, K], clipped counts int32
        # [C, K, 2], energies fp32 [C], pixels scored (on the host); `act_score_kind`: "auto" (act_freeze picks each channel's winner) or
        # "report" (act_freeze records `act_stats` of the frozen range).  act_stats: site -> {err, energy, clip_lo, clip_hi, n}, kept on
        # the frozen quantiser.  All absent on models pickled before they existed: read with getattr
        self.act_cand = {}
        self.act_clip = {}
        self.act_energy = {}
        self.act_score_n = {}
        self.act_score_kind = "auto"
        self.act_stats = {}
        # the width scan (`act_scan`): the widths being scanned (None: no scan is open) and site -> {err float64 [K, C], energy float64
        # [C], n: values seen per channel (on the host)}.  Absent on models pickled before they existed: read with getattr
        self.act_scan_widths = None
        self.act_scan_sums = {}

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        for name in ("delta", "zero_point"):
            t = getattr(self, name, None)
            if torch.is_tensor(t):
                setattr(self, name, fn(t))
        for name in ("act_range", "act_err", "act_obs", "act_hist", "act_cand", "act_clip", "act_energy"):
            d = getattr(self, name, None)
            if isinstance(d, dict):
                setattr(self, name, {k: fn(t) for k, t in d.items()})
        st = getattr(self, "act_stats", None)
        if isinstance(st, dict):
            self.act_stats = {k: {f: (fn(t) if torch.is_tensor(t) else t) for f, t in d.items()} for k, d in st.items()}
        return self

    # -- static activation grids ----------------------------------------------------------------------------------
    def set_act_mode(self, mode: str):
        if mode not in ACT_MODES:
            raise ValueError(f"unknown act_mode {mode!r} {ACT_MODES}")
        for name, val in (("act_phase", "idle"), ("act_range", {}), ("act_err", {}), ("act_obs", {}), ("act_hist", {})):     # (an artefact of an earlier version)
            if not hasattr(self, name):
                setattr(self, name, val)
        self.act_mode = mode

    def act_observe(self):
        """Start observing: every call quantises dynamically and merges the batch's per-channel min / max into the site's range."""
        self.act_phase, self.act_range, self.act_err, self.act_obs, self.act_hist = "observe", {}, {}, {}, {}
        self.act_cand, self.act_clip, self.act_energy, self.act_score_n, self.act_stats = {}, {}, {}, {}, {}

    def act_search(self):
        """Start the L2 search over the observed ranges: every call accumulates the ten candidates' squared errors and returns the
        max-range static output."""
        if not self.act_range:
            raise RuntimeError("act_search: nothing was observed")
        self.act_phase = "search"
        self.act_obs = {k: r.clone() for k, r in self.act_range.items()}
        self.act_err = {k: torch.zeros(r.numel() // 2, ops.ACT_SEARCH_CANDIDATES, device=r.device) for k, r in self.act_range.items()}

    def act_histogram(self, percentile: float = 99.99, rule: str = "percentile", search: bool = False):
        """Start the histogram pass over the observed ranges: every call counts its values per channel into the site's 1024 bins and
        returns the max-range static output (what the search phase returns).  `act_freeze()` then clips a share 1 - percentile / 100 of
        the counted values at each end of every channel, in whole bins (rule "percentile"), or drops the whole bins from each end that
        minimise the modelled squared error on this quantiser's grid width (rule "mse": `percentile` is not used).  `search`: the same
        calls also accumulate the L2 search's error sums (phase "search+hist": both read the same max-range inputs), for
        `act_candidates`."""
        if rule not in ACT_HIST_RULES:
            raise ValueError(f"unknown act_histogram rule {rule!r} {ACT_HIST_RULES}")
        if not self.act_range:
            raise RuntimeError("act_histogram: nothing was observed")
        self.act_phase = "search+hist" if search else "hist"
        if search:
            self.act_err = {k: torch.zeros(r.numel() // 2, ops.ACT_SEARCH_CANDIDATES, device=r.device) for k, r in self.act_range.items()}
        self.act_hist_rule = rule
        self.act_tail = 1.0 - float(percentile) / 100.0
        self.act_obs = {k: r.clone() for k, r in self.act_range.items()}
        self.act_hist = {k: ops.act_hist_init(r.numel() // 2, r.device) for k, r in self.act_range.items()}
        self.act_hist_n = {k: 0 for k in self.act_range}

    def _act_count(self, xr, rng, site):
        """one batch into the site's histogram; the counters are 32-bit, and under data parallelism the ranks' histograms are summed"""
        from . import dp
        n = self.act_hist_n[site] + xr.numel() // xr.shape[-1]
        if n * dp.world()[1] > 2 ** 31 - 1:
            raise OverflowError(f"static activation quantiser (site {site}): {n} values per channel on each of {dp.world()[1]} ranks "
                                "do not fit the histogram's 32-bit counters")
        ops.actquant_hist(xr, rng, self.act_hist[site])
        self.act_hist_n[site] = n

    def act_candidates(self):
        """After a "search+hist" pass: site -> fp32 [4, 2C], the ranges that 'max', 'l2', 'percentile' (with the pass's percentile) and
        'hist_mse' (on this quantiser's grid width) would freeze, in the order ACT_AUTO_CANDIDATES."""
        if getattr(self, "act_phase", "idle") != "search+hist":
            raise RuntimeError("act_candidates: no search and histogram pass was made (act_histogram(search=True))")
        bits = int(getattr(self, "dynamic_bits", 8))
        out = {}
        for k, rng in self.act_range.items():
            rng = rng.detach()
            out[k] = torch.stack([rng, act_l2_range(rng, self.act_err[k]),
                                  ops.act_percentile_select(self.act_hist[k], rng, getattr(self, "act_tail", 0.0)),
                                  ops.act_hist_mse_select(self.act_hist[k], rng, bits)]).contiguous()
        return out

    def act_score(self, cands=None):
        """Start the scoring pass: every call adds, per site, the MEASURED squared error of the site's K candidate grids `cands[site]`
        [K, 2C] on the values it sees (`ops.actquant_score`: the static quantiser's own expression), the counts of the values clipped at
        each end and the energy, and returns the static output on the range the site holds.  Before a range is frozen (after observing:
        `cands` from `act_candidates`) that is the max range, as in the search and histogram phases, and `act_freeze()` then gives each
        channel the candidate of least measured error.  On a frozen quantiser (`cands` None: every site scores its own frozen range, K =
        1) the frozen output goes downstream, and `act_freeze()` records `act_stats` and leaves the ranges as they are."""
        if not getattr(self, "act_range", None):
            raise RuntimeError("act_score: nothing was observed")
        report = self.act_frozen()
        if cands is None:
            if not report:
                raise RuntimeError("act_score: candidates are needed until the ranges are frozen")
            cands = {k: r.detach().reshape(1, -1) for k, r in self.act_range.items()}
        if sorted(cands) != sorted(self.act_range):
            raise ValueError(f"act_score: candidates for the sites {sorted(cands)}, ranges for {sorted(self.act_range)}")
        for k, cnd in cands.items():
            if cnd.dim() != 2 or not 1 <= cnd.shape[0] <= ops.ACT_SCORE_MAX or cnd.shape[1] != self.act_range[k].numel():
                raise ValueError(f"act_score (site {k}): candidates must be [1..{ops.ACT_SCORE_MAX}, {self.act_range[k].numel()}], got "
                                 f"{tuple(cnd.shape)}")
        self.act_cand = {k: cnd.detach().to(torch.float32).contiguous() for k, cnd in cands.items()}
        shape = {k: (cnd.shape[1] // 2, cnd.shape[0]) for k, cnd in self.act_cand.items()}
        dev = {k: cnd.device for k, cnd in self.act_cand.items()}
        self.act_err = {k: torch.zeros(c, kk, device=dev[k]) for k, (c, kk) in shape.items()}
        self.act_clip = {k: torch.zeros(c, kk, 2, dtype=torch.int32, device=dev[k]) for k, (c, kk) in shape.items()}
        self.act_energy = {k: torch.zeros(c, device=dev[k]) for k, (c, kk) in shape.items()}
        self.act_score_n = {k: 0 for k in shape}
        self.act_hist, self.act_hist_n = {}, {}
        if not report:
            self.act_obs = {k: r.detach().clone() for k, r in self.act_range.items()}
        self.act_score_kind = "report" if report else "auto"
        self.act_phase = "score"

    def _act_score_one(self, xr, site, bits):
        """one batch into the site's score sums; the counts are 32-bit, and under data parallelism the ranks' counts are summed"""
        from . import dp
        n = self.act_score_n[site] + xr.numel() // xr.shape[-1]
        if n * dp.world()[1] > 2 ** 31 - 1:
            raise OverflowError(f"static activation quantiser (site {site}): {n} values per channel on each of {dp.world()[1]} ranks "
                                "do not fit the score's 32-bit counts")
        ops.actquant_score(xr, self.act_cand[site], self.act_err[site], self.act_clip[site], self.act_energy[site], n_bits=int(bits))
        self.act_score_n[site] = n

    def _act_close_score(self, keep_obs):
        """the end of a scoring pass: 'auto' assembles each channel's range from its winning candidate; 'report' records the statistics"""
        for k, err in self.act_err.items():
            cnd = self.act_cand[k]
            c = cnd.shape[1] // 2
            if getattr(self, "act_score_kind", "auto") == "report":
                clip = self.act_clip[k]
                self.act_stats[k] = {"err": err[:, 0].clone(), "energy": self.act_energy[k].clone(), "clip_lo": clip[:, 0, 0].clone(),
                                     "clip_hi": clip[:, 0, 1].clone(), "n": int(self.act_score_n[k])}
            else:
                win = act_score_winner(err).unsqueeze(0)
                self.act_range[k] = torch.cat([cnd[:, :c].gather(0, win).reshape(-1), cnd[:, c:].gather(0, win).reshape(-1)])
        self.act_err, self.act_cand, self.act_clip, self.act_energy, self.act_score_n = {}, {}, {}, {}, {}
        self.act_score_kind = "auto"
        if not keep_obs:
            self.act_obs = {}
        self.act_phase = "frozen" if self.act_range else "idle"

    def act_learn(self):
        """Start learning the frozen ranges: every site's range becomes a leaf tensor with requires_grad that the tracked forward
        differentiates to (ActQuantStaticFn) and `ops.act_range_step` updates in place; `act_obs` holds the observed max range of every
        site -- what a search kept (`act_freeze(keep_obs=True)`), else the frozen range itself (a 'max' range is its own max range).
        `act_freeze()` ends the phase."""
        if not self.act_frozen():
            raise RuntimeError("act_learn: the ranges are not frozen (calibrate them first)")
        obs = getattr(self, "act_obs", None) or {}
        self.act_obs = {k: (obs[k] if k in obs else r.detach().clone()) for k, r in self.act_range.items()}
        self.act_range = {k: r.detach().clone().requires_grad_(True) for k, r in self.act_range.items()}
        self.act_phase = "learn"

    def act_freeze(self, keep_obs: bool = False):
        """Fix the ranges.  After a search each channel shrinks to its best candidate lo * s_k | hi * s_k (first minimum, as `_init_search`
        keeps the first strictly better score).  Scaling towards zero moves an end that does not straddle zero (lo > 0 or hi < 0) OUT of
        the observed range, where no calibration value lies: such an end stays at the observed one, so a frozen range always lies inside
        its max range.  After a histogram pass each site becomes its percentile range (`ops.act_percentile_select`), which lies inside the
        max range as well, or, under the rule "mse", its histogram-MSE range on the grid width `dynamic_bits` (`ops.act_hist_mse_select`).
        A quantiser that was never applied stays without a range ("idle").  After learning the ranges are detached as they
        stand.  After a scoring pass (`act_score`) each channel takes the candidate of least measured error (smallest sum; among equal sums
        the earliest of max, l2, percentile, hist_mse; never a NaN sum; the max range if all are NaN), or, on a quantiser that was frozen
        already, the ranges stay and `act_stats` is recorded.  `keep_obs`: keep the observed max ranges for a learning phase that follows (they are not part of a frozen quantiser)."""
        self.act_range = {k: r.detach() for k, r in self.act_range.items()}
        if getattr(self, "act_phase", "idle") == "score":
            if not hasattr(self, "act_stats"):
                self.act_stats = {}
            return self._act_close_score(keep_obs)
        if getattr(self, "act_phase", "idle") == "search+hist":
            raise RuntimeError("act_freeze: a search + histogram pass only feeds act_candidates(); score them first (act_score)")
        for k, err in self.act_err.items():
            self.act_range[k] = act_l2_range(self.act_range[k], err)
        for k, hist in (getattr(self, "act_hist", None) or {}).items():
            if getattr(self, "act_hist_rule", "percentile") == "mse":
                self.act_range[k] = ops.act_hist_mse_select(hist, self.act_range[k], int(getattr(self, "dynamic_bits", 8)))
            else:
                self.act_range[k] = ops.act_percentile_select(hist, self.act_range[k], getattr(self, "act_tail", 0.0))
        self.act_err, self.act_hist, self.act_hist_n = {}, {}, {}
        if not keep_obs:
            self.act_obs = {}
        self.act_phase = "frozen" if self.act_range else "idle"

    def act_frozen(self):
        return getattr(self, "act_mode", "dynamic") == "static" and getattr(self, "act_phase", "idle") == "frozen"

    def act_scan(self, widths):
        """Open a width scan: every application with act=True then adds, per site, what the grid it quantises on costs the values it
        sees at each of `widths` (`ops.actquant_width_scan`: the squared error of the static expression on that grid at every width, and
        the energy) into float64 device sums.  The grid is the site's frozen range in static mode and the call's own per-channel min | max
        in dynamic mode (what `ops.actquant_perchannel` quantises on).  What the quantiser returns is not changed.  RuntimeError on a
        static quantiser that is not frozen and while another phase (observe, search, hist, score, learn) is active."""
        widths = ops.width_list("act_scan", widths, MAX_BITS)
        phase = getattr(self, "act_phase", "idle")
        if getattr(self, "act_mode", "dynamic") == "static":
            if phase != "frozen":
                raise RuntimeError(f"act_scan: the static quantiser is not frozen (phase {phase!r}): calibrate it first")
        elif phase not in ("idle", "frozen"):
            raise RuntimeError(f"act_scan: the phase {phase!r} is active")
        self.act_scan_widths, self.act_scan_sums = widths, {}

    def act_scan_close(self):
        """Close the scan -> site -> {'err': float64 [K, C], 'energy': float64 [C], 'n': values seen per channel}, on the device; the sums
        are cleared.  A site that was not applied has no entry."""
        sums = getattr(self, "act_scan_sums", None) or {}
        self.act_scan_widths, self.act_scan_sums = None, {}
        return sums

    def _act_scan_one(self, xr, rng, site):
        """one call's scan into the site's float64 sums"""
        err, energy = ops.actquant_width_scan(xr, rng, self.act_scan_widths)
        st = self.act_scan_sums.get(site)
        if st is None:
            st = self.act_scan_sums[site] = {"err": torch.zeros(err.shape[1], err.shape[0], dtype=torch.float64, device=err.device),
                                             "energy": torch.zeros(energy.shape[0], dtype=torch.float64, device=err.device), "n": 0}
        if st["energy"].numel() != energy.numel():
            raise ValueError(f"act_scan (site {site}): scanned {st['energy'].numel()} channels before, got {energy.numel()}")
        st["err"] += err.t().double()
        st["energy"] += energy.double()
        st["n"] += xr.numel() // xr.shape[-1]

    def _act_dynamic_scan(self, x, site, channels_last):
        """the dynamic quantiser with a scan open: the same kernels on the same operands as `ActQuantizer` (the same bits out), with the
        min | max they leave in the workspace as the scanned grid"""
        xr, back = _act_rows(x, channels_last)
        Cc = xr.shape[-1]
        ws = torch.empty(ops.actquant_workspace(Cc), device=xr.device, dtype=torch.float32)
        out = ops.actquant_perchannel(xr, ws=ws, n_bits=getattr(self, "dynamic_bits", 8))
        self._act_scan_one(xr, ws[:2 * Cc], site)
        return back(out)

    def _act_static(self, x, site, channels_last):
        xr, back = _act_rows(x, channels_last)
        bits, Cc, phase = getattr(self, "dynamic_bits", 8), xr.shape[-1], self.act_phase
        rng = self.act_range.get(site)
        if rng is not None and rng.numel() != 2 * Cc:
            raise ValueError(f"static activation quantiser (site {site}): calibrated for {rng.numel() // 2} channels, got {Cc}")
        if phase == "observe":
            if rng is None:
                rng = self.act_range[site] = ops.act_range_init(Cc, xr.device)
            return back(ops.actquant_observe(xr, rng, n_bits=bits))
        if rng is None:
            raise RuntimeError(f"static activation quantiser (site {site}) has no frozen range: calibrate it first "
                               "(recon.py with args.act_mode='static'); there is no fall-back to the dynamic grid")
        if phase in ("search", "search+hist"):
            ops.actquant_search(xr, rng, self.act_err[site], n_bits=bits)
        if phase in ("hist", "search+hist"):
            self._act_count(xr, rng, site)
        if phase == "score":
            self._act_score_one(xr, site, bits)
        if getattr(self, "act_scan_widths", None):
            self._act_scan_one(xr, rng.detach(), site)
        if torch.is_grad_enabled() and (phase == "learn" or (phase == "frozen" and getattr(self, "act_ste", False) and x.requires_grad)):
            from hipops.autograd import ActQuantStaticFn
            return ActQuantStaticFn.apply(x, rng, bits, channels_last)
        return back(ops.actquant_static(xr, rng.detach(), n_bits=bits))

    # -- scale initialisation -------------------------------------------------------------------------------------
    def _rows(self, x):
        wr = to_rows(x, self.tconv) if (self.channel_wise and x.dim() != 1) else x.reshape(1, -1).contiguous()
        return wr

    def init_quantization_scale(self, x: torch.Tensor, channel_wise: bool = False):
        rows2d = (to_rows(x, self.tconv) if (channel_wise and x.dim() != 1) else x.reshape(1, -1)).contiguous()
        flat = rows2d.reshape(rows2d.shape[0], -1)
        m = self.scale_method
        if "max" in m and "scale" not in m and not self.sym:
            delta, zp = ops.uaq_init_minmax(flat, self.n_levels)
        else:
            delta, zp = self._init_search(flat)
        shape = _scale_shape(x, self.tconv) if channel_wise else ()
        return delta.reshape(shape), zp.reshape(shape)

    def _init_search(self, flat):
        """'max' variants with scaling/symmetry, 'gaussian', and the 10-step shrink searches ('mse' = L3.5, 'l1', 'l2'),
        vectorised over channels (the reference loops over channels in Python, quantizer.py:260-265)."""
        m, L = self.scale_method, self.n_levels
        eps = torch.tensor(1e-8, device=flat.device)
        if m == "gaussian":
            # tensor arithmetic in fp32 throughout, as in the reference (quantizer.py:318-335; its 'scale' branch is dead there)
            mu, var = flat.mean(1), flat.var(1)
            lo, hi = torch.clamp(mu - 6 * var, max=0), torch.clamp(mu + 6 * var, min=0)
            if self.sym:
                amax = torch.maximum(lo.abs(), hi)
                lo, hi = torch.where(lo < 0, -amax, torch.zeros_like(lo)), amax
            delta = torch.maximum((hi - lo) / (L - 1), eps)
            return delta, (-lo / delta).round()
        if "max" in m:
            # the reference holds x_min / x_max as Python floats (double) from here on: scaling, symmetrisation and the range
            # are evaluated in double and rounded to fp32 ONCE (quantizer.py:282-293); doing the scaling in fp32 can move delta
            # by an ulp and flip a zero point that sits on x.5
            lo, hi = torch.clamp(flat.amin(1), max=0).double(), torch.clamp(flat.amax(1), min=0).double()
            if "scale" in m:
                lo, hi = lo * (self.n_bits + 2) / 8, hi * (self.n_bits + 2) / 8
            if self.sym:
                amax = torch.maximum(lo.abs(), hi)
                lo, hi = torch.where(lo < 0, -amax, torch.zeros_like(lo)), amax
            delta = torch.maximum(((hi - lo) / (L - 1)).float(), eps)
            # the reference divides a Python float by the tensor, which torch evaluates as delta.reciprocal() * (-x_min)
            # (quantizer.py:296) -- one more rounding, it decides ties at x.5
            return delta, (delta.reciprocal() * (-lo).float()).round()
        if m not in ("mse", "l1", "l2"):
            raise NotImplementedError(m)
        hi0, lo0 = flat.amax(1, keepdim=True), flat.amin(1, keepdim=True)
        best = torch.full((flat.shape[0],), 1e10, device=flat.device)
        delta = torch.zeros_like(best)
        zp = torch.zeros_like(best)
        for i in range(10):
            hi, lo = hi0 * (1.0 - i * 0.05), lo0 * (1.0 - i * 0.05)
            d = torch.maximum((hi - lo) / (L - 1), eps)
            z = (-lo / d).round()
            xq = (torch.clamp(torch.round(flat / d) + z, 0, L - 1) - z) * d
            err = (flat - xq).abs()
            score = err.pow(3.5).mean(1) if m == "mse" else (err.mean(1) if m == "l1" else err.pow(2).mean(1))
            better = score < best
            best = torch.where(better, score, best)
            delta = torch.where(better, d.squeeze(1), delta)
            zp = torch.where(better, z.squeeze(1), zp)
        return delta, zp

    # -- forward ---------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, act: bool = False, site: int = 0, channels_last: bool = False):
        if act:
            if getattr(self, "act_mode", "dynamic") == "static":
                return self._act_static(x, site, channels_last)
            if getattr(self, "act_scan_widths", None):
                return self._act_dynamic_scan(x, site, channels_last)
            if channels_last:
                return ops.actquant_perchannel(x.detach().contiguous(), n_bits=getattr(self, "dynamic_bits", 8))
            return ActQuantizer(x, getattr(self, "dynamic_bits", 8))
        if not self.inited:
            if self.leaf_param:
                return x
            self.delta, self.zero_point = self.init_quantization_scale(x.detach(), self.channel_wise)
            self.inited = True
        wr = self._rows(x.detach())
        desc = ops.ada_desc(wr.reshape(wr.shape[0], -1), self.n_levels, conv_layout=False)
        wq = ops.uaq_fakequant(desc, wr, self.delta.reshape(-1).contiguous().expand(wr.shape[0]).contiguous(),
                               self.zero_point.reshape(-1).contiguous().expand(wr.shape[0]).contiguous())
        if self.channel_wise and x.dim() != 1:
            return from_rows(wq, x, self.tconv)
        return wq.reshape(x.shape)

    def bitwidth_refactor(self, refactored_bit: int):
        assert 2 <= refactored_bit <= MAX_BITS, "bitwidth not supported"
        self.n_bits = refactored_bit
        self.n_levels = 2 ** refactored_bit

    def extra_repr(self):
        return (f"bit={self.n_bits}, scale_method={self.scale_method}, symmetric={self.sym}, "
                f"channel_wise={self.channel_wise}, leaf_param={self.leaf_param}")


# ----------------------------------------------------------------------------- AdaRound
class AdaRoundQuantizer(nn.Module):
    """Learned rounding.  `alpha` is an nn.Parameter with the logical shape of the weight; its storage is the kernel
    layout (OHWI for conv weights), shared with the calibration engine that trains it."""

    def __init__(self, uaq: UniformAffineQuantizer, weight_tensor: torch.Tensor, round_mode="learned_round_sigmoid",
                 alpha_rows: torch.Tensor = None):
        super().__init__()
        self.n_bits, self.sym, self.n_levels = uaq.n_bits, uaq.sym, uaq.n_levels
        self.delta, self.zero_point = uaq.delta, uaq.zero_point
        self.tconv, self.channel_wise = uaq.tconv, uaq.channel_wise
        self.round_mode = round_mode
        self.soft_targets = False
        self.gamma, self.zeta, self.beta = GAMMA, ZETA, 2 / 3
        self._like = weight_tensor
        if round_mode != "learned_hard_sigmoid":
            raise NotImplementedError(round_mode)
        wr = self._rows(weight_tensor.detach())
        if alpha_rows is None:
            logging.info("Init alpha to be FP32")
            alpha_rows = ops.adaround_init_alpha(self._desc(wr), wr, self._row_scales(wr)[0])
        self.alpha = nn.Parameter(self._unrows(alpha_rows, weight_tensor))

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        for name in ("delta", "zero_point"):
            t = getattr(self, name, None)
            if torch.is_tensor(t):
                setattr(self, name, fn(t))
        return self

    def _rows(self, x):
        return to_rows(x, self.tconv) if (self.channel_wise and x.dim() != 1) else x.reshape(1, -1).contiguous()

    def _unrows(self, r, like):
        return from_rows(r, like, self.tconv) if (self.channel_wise and like.dim() != 1) else r.reshape(like.shape)

    def _desc(self, wr):
        return ops.ada_desc(wr.reshape(wr.shape[0], -1), self.n_levels, conv_layout=False)

    def _row_scales(self, wr):
        n = wr.shape[0]
        return (self.delta.reshape(-1).expand(n).contiguous(), self.zero_point.reshape(-1).expand(n).contiguous())

    def forward(self, x):
        wr = self._rows(x.detach())
        ar = self._rows(self.alpha.detach())
        d, z = self._row_scales(wr)
        wq = ops.adaround_fwd(self._desc(wr), wr, ar, d, z, self.soft_targets)
        return self._unrows(wq, x)

    def get_soft_targets(self):
        return torch.clamp(torch.sigmoid(self.alpha) * (self.zeta - self.gamma) + self.gamma, 0, 1)

    def extra_repr(self):
        return f"bit={self.n_bits}"
