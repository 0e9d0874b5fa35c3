"""Reference of learned rounding on the MX grids (include/rdo_ptq_mxround.h), shared by tests/test_mx_round_args.py and
tests/test_gpu_mx_round.py: float64 in torch on the CPU, built on tests/mx_reference.py.

The grid of a format is enumerated (every magnitude code decoded by `mx_reference.dequantize`), the neighbours of an element are found by
a search in that sorted table times the block's scale: nothing of the kernels' bit arithmetic is restated.  The step is
`oracle.rdo_oracle.adaround_step_reference`, as it is, with per-element delta = gap, zp = 64 and n_levels = 129 on the non-pinned
elements: floor(w / gap) in fp32 times gap is lo, |lo / gap| <= 16, so the level clamp can never engage and its wq is lo + gap h."""
import torch

import mx_reference as R
from oracle import rdo_oracle as O

ZP, N_LEVELS = 64.0, 129
PINNED_ALPHA = 30.0            # `MxQOp` only: where the oracle's loop keeps the alpha of a pinned element (the kernels keep 0 and skip it)


def magnitudes(fmt):
    """the representable magnitudes of `fmt` in ascending order (float64): codes 0 .. the code of the maximum"""
    _, eb, M, _, _, vmax = R.FORMATS[fmt]
    codes = torch.arange(2 ** (eb + M), dtype=torch.uint8).reshape(1, -1)
    mags = R.dequantize(codes, torch.full((1, R.blocks(codes.shape[1])), 127, dtype=torch.uint8), fmt).double().reshape(-1)
    mags = mags[mags <= vmax]                                             # (E4M3's NaN code, E5M2's infinities and NaNs lie above)
    assert bool((mags[1:] > mags[:-1]).all()) and float(mags[-1]) == vmax and float(mags[0]) == 0.0
    return mags


def neighbours(w, fmt):
    """w fp32 [rows, inner] on the CPU -> dict: lo, gap fp32 [rows, inner], pinned bool, scales uint8 [rows, blocks] (those of
    `mx_reference.quantize`).  A block that is not finite: lo NaN, gap 0, pinned False."""
    assert w.dtype == torch.float32 and w.dim() == 2 and not w.is_cuda
    rows, inner = w.shape
    scales = R.quantize(w, fmt)["scales"]
    sc = scales.to(torch.int64).repeat_interleave(R.BLOCK, dim=1)[:, :inner]
    bad = sc == 255
    X = torch.ldexp(torch.ones(sc.shape, dtype=torch.float64), torch.where(bad, torch.zeros_like(sc), sc - 127))
    mags = magnitudes(fmt)
    grid = torch.cat([-mags.flip(0)[:-1], mags])                          # the signed grid of X = 1, ascending, one zero
    x = torch.where(bad, torch.zeros_like(X), w.double() / X)             # exact: X is a power of two
    k = torch.searchsorted(grid, x.contiguous(), right=True) - 1          # the largest grid index with grid[k] <= x; -1 below the grid
    top = grid.numel() - 1
    pinned = ((k >= top) | (k < 0)) & ~bad
    lo = grid[k.clamp(0, top)]
    hi = grid[(k + 1).clamp(0, top)]
    gap = torch.where(pinned, torch.zeros_like(lo), hi - lo)
    lo64, gap64 = lo * X, gap * X
    lo32, gap32 = lo64.float(), gap64.float()
    assert torch.equal(lo32.double(), lo64) and torch.equal(gap32.double(), gap64), "lo / gap not exactly representable in float32"
    nan = torch.full_like(lo32, float("nan"))
    return {"lo": torch.where(bad, nan, lo32), "gap": torch.where(bad, torch.zeros_like(gap32), gap32), "pinned": pinned, "scales": scales}


def init_alpha(w, lo, gap):
    """rest = (w - lo) / gap in fp32 (the subtraction rounds once), alpha0 = -log(1.2 / (rest + 0.1) - 1) as `O.adaround_init_alpha` forms it,
    in torch fp32: there an exact tie gives 1.2f / 0.6f = 2 and so alpha0 = 0 exactly (in float64 it is -4e-16: the hard weight would go
    down); 0 where gap == 0.  -> fp32"""
    live = gap > 0
    rest = torch.where(live, (w - lo) / torch.where(live, gap, torch.ones_like(gap)), torch.full_like(w, 0.5))
    a = -torch.log((O.ZETA - O.GAMMA) / (rest - O.GAMMA) - 1)
    return torch.where(live, a, torch.zeros_like(a))


def soft_h(alpha):
    return O.adaround_soft_targets(alpha.double())


def forward(lo, gap, alpha, soft, reparam=None):
    """float64 soft / hard weight lo + gap h (hard: exact in fp32), through max(., bound)^2 - pedestal with `reparam`"""
    h = soft_h(alpha) if soft else (alpha >= 0).double()
    q = lo.double() + gap.double() * h
    return q if reparam is None else q.clamp(min=float(reparam[0])) ** 2 - float(reparam[1])


def step(lo, gap, alpha, m, v, G, sched_row, *, grad_scale, round_weight, reparam=None):
    """One step in float64: `O.adaround_step_reference` on the non-pinned elements (gap > 0) with w = lo + gap / 2 (any point of the
    interval gives floor(w / gap) = lo / gap), delta = gap, zp = 64, n_levels = 129.  -> its dict with every tensor scattered back to the
    full shape: pinned elements keep alpha, m, v and have wq = lo (through the reparam); `live` marks the non-pinned ones."""
    live = gap > 0
    sel = lambda t: t[live]
    lo_l, gap_l = sel(lo), sel(gap)
    w_mid = lo_l + gap_l * 0.5                                            # exact in fp32 except at the very bottom of the subnormals
    assert torch.equal(torch.floor(w_mid / gap_l) * gap_l, lo_l) and float((lo_l / gap_l).abs().max()) <= 16
    ref = O.adaround_step_reference(w_mid, gap_l, torch.full_like(gap_l, ZP), sel(alpha), sel(m), sel(v), sel(G), sched_row, n_levels=N_LEVELS,
                                    grad_scale=grad_scale, round_weight=round_weight, reparam=reparam)
    out = {"live": live, "round_loss": ref["round_loss"]}
    keep = {"alpha": alpha.double(), "m": m.double(), "v": v.double(), "wq": forward(lo, gap, alpha, True, reparam)}
    for k in ("dalpha_data", "g_round", "g_total", "m", "v", "alpha", "wq"):
        full = keep[k].clone() if k in keep else torch.zeros(lo.shape, dtype=torch.float64)
        full[live] = ref[k]
        out[k] = full
    out["masks"] = {}
    for k, t in ref["masks"].items():
        full = torch.full(lo.shape, 0.5, dtype=torch.float64)            # (a pinned element sits on no kink)
        full[live] = t
        out["masks"][k] = full
    return out


class MxQOp(O.QOp):
    """An `O.QOp` whose AdaRound state lives on an MX grid, so that the unmodified `O.reconstruct_unit` runs a unit on it: lo / gap from
    the original weight's rows (`to_rows` order: OHWI, a transposed conv's [in, out, kh, kw] weight by its dim 1), alpha0 by `init_alpha`,
    the weight lo + gap h(alpha) (pinned: lo).  `fmt` is a class attribute of the subclass `of(fmt)` makes."""
    fmt = None

    @classmethod
    def of(cls, fmt):
        return type(f"MxQOp_{fmt}", (cls,), {"fmt": fmt})

    def _rows(self, t):
        w = self.weight
        if w.dim() == 4:
            return (t.permute(1, 2, 3, 0) if self.kind == "tconv" else t.permute(0, 2, 3, 1)).contiguous()
        return t.reshape(1, -1).contiguous() if w.dim() == 1 else t.contiguous()

    def _unrows(self, r):
        w = self.weight
        if w.dim() == 4:
            co, kh, kw, ci = (w.shape[1], w.shape[2], w.shape[3], w.shape[0]) if self.kind == "tconv" else (w.shape[0], w.shape[2], w.shape[3], w.shape[1])
            r = r.reshape(co, kh, kw, ci)
            return r.permute(3, 0, 1, 2) if self.kind == "tconv" else r.permute(0, 3, 1, 2)
        return r.reshape(w.shape)

    def init_scale(self):
        if getattr(self, "lo", None) is None:
            wr = self._rows(self.weight.detach().float())
            nb = neighbours(wr.reshape(wr.shape[0], -1), self.fmt)
            self.lo, self.gap = (self._unrows(nb[k]).contiguous() for k in ("lo", "gap"))
        return self

    def to_adaround(self):
        self.init_scale()
        a0 = init_alpha(self.weight.detach().float(), self.lo, self.gap).float()
        # a pinned element does not exist for the optimiser, but `reconstruct_unit` sums the rounding loss over every alpha: PINNED_ALPHA
        # puts h at exactly 1 (no loss, no slope), and gap = 0 keeps the data gradient at exactly 0, so Adam never moves it
        self.alpha = torch.where(self.gap > 0, a0, torch.full_like(a0, PINNED_ALPHA)).requires_grad_(True)
        self.mode, self.soft = "ada", True
        return self

    def qweight(self):
        if self.mode == "fp":
            return self.weight
        self.init_scale()
        if self.mode == "uaq":
            wr = self._rows(self.weight.detach().float())
            return self._unrows(R.quantize(wr.reshape(wr.shape[0], -1), self.fmt)["wq"])
        h = O.adaround_soft_targets(self.alpha) if self.soft else (self.alpha >= 0).float()
        return self.lo + self.gap * h
