"""Calibration engine: the AdaRound hot loop of one reconstruction unit as a recorded HIP op list.

This replaces the Python/autograd loop body of the reference (`for i in range(iters)` at
/root/reference/task-oriented-PTQ/quantization/layer_opt.py:287-309 and block_opt.py:287-311):

    idx -> gather cached (x_q, x_fp) -> QDrop mix -> unit forward with soft-rounded weights -> rec + task + round loss
        -> backward -> Adam on the rounding logits alpha

Forward, the hand-derived backward, the loss and the optimiser are enqueued as one native plan per iteration
(hipops.plan.Plan -> rdo_plan_run, hipGraph replay), with every per-iteration scalar (temperature b, Adam bias corrections,
mini-batch indices) read on the device from tables indexed by a device-side iteration counter: zero host work or syncs
inside the loop.  Units: a single `QuantModule` ('layer': conv, transposed conv, GDN / IGDN, with a fused LeakyReLU / ReLU) and the
Cheng2020 blocks QuantRB / QuantRBWS / QuantRBU; the Lu2022 RSTB blocks and every unit whose task loss runs through the rest of
its sub-coder are handled by `swin_engine.TapeEngine`, a subclass that reuses the ops, buffers and plans defined here.

This file holds what one iteration IS (weight holders, buffers, forms, the `_fb_*` bodies, step and record) and the fp16 range of
the planes (probe, poll, restart).  How the recorded plans are DRIVEN where one `Plan.run` does not do is in two base classes of
`UnitEngine`: `engine_dp.DpLoop` (data parallel) and `engine_rd.RdTask` (the opt-in R + lambda*D task loss).

Loss = round + rec + task exactly as the reference computes it for Sequential-indexed CompressAI models, where the task
term degenerates to a second copy of the reconstruction term: `coef = 2`.

Data parallel (world_size > 1): each rank holds its shard of the caches; per iteration the chained data-gradient of all
alphas of the unit is written into one flat bucket, all-reduced (RCCL over xGMI, SUM) and applied with scale 1/world_size;
the rounding regulariser is data independent and is added locally after the reduction."""
import math
import os
from collections import OrderedDict

import torch

from hipops import _lib as L
from hipops import ops
from hipops.plan import Plan

from . import dp
from .engine_dp import DpLoop, DpStallError  # noqa: F401  (DpStallError: re-exported)
from .engine_rd import RdTask
from .quant_layer import QuantModule
from .quantizer import AdaRoundQuantizer, from_rows, to_rows

UNIT_KINDS = ("layer", "rb", "rbws", "rbu", "rstb")


class IdxStream:
    """Mini-batch index tables drawn from torch's GLOBAL CPU generator exactly as the reference draws them -- one `torch.randperm(n)` per
    iteration (layer_opt.py:289) -- with the NEXT unit's table drawn ahead of time while the GPU runs the current unit's loop (20 000
    draws of randperm(256) cost the host ~0.1 s per unit, 2 % of the full schedule, with the GPU idle).

    Exactness: the look-ahead works on a PRIVATE generator started from a copy of the global generator's state; it is adopted only if the
    next request asks for the same (n, B, iters) AND the global generator's state is still that copy (nobody drew from it or re-seeded it in
    between) -- the global generator is then moved to the private generator's final state, i.e. exactly where the draws would have left
    it.  Anything else discards the look-ahead and draws from the global generator as before."""
    _spec = None

    @classmethod
    def begin(cls, n, B, iters):
        g = torch.Generator()
        state0 = torch.get_rng_state()
        g.set_state(state0)
        cls._spec = dict(key=(int(n), int(B), int(iters)), state0=state0, gen=g, rows=[])

    @classmethod
    def step(cls, k):
        """draw up to k more rows of the look-ahead (called between the enqueues of `UnitEngine.run`)"""
        sp = cls._spec
        if sp is None:
            return
        n, B, iters = sp["key"]
        k = min(int(k), iters - len(sp["rows"]))
        g = sp["gen"]
        sp["rows"].extend(torch.randperm(n, generator=g)[:B] for _ in range(k))

    @classmethod
    def take(cls, n, B, iters):
        sp, cls._spec = cls._spec, None
        if sp is not None and sp["key"] == (int(n), int(B), int(iters)) and torch.equal(torch.get_rng_state(), sp["state0"]):
            g = sp["gen"]
            sp["rows"].extend(torch.randperm(n, generator=g)[:B] for _ in range(iters - len(sp["rows"])))
            torch.set_rng_state(g.get_state())
            return torch.stack(sp["rows"])
        return torch.stack([torch.randperm(n)[:B] for _ in range(iters)])


# Forms of an activation tensor inside a unit (`UnitEngine._forms`): as an fp32 tensor, as H2 planes (two fp16 planes of the scaled
# tensor), as both, or -- the pre-activation of a conv whose tail runs in the same launch -- not in memory at all
ABSENT, F32, PLANES, BOTH = 0, 1, 2, 3


class Act:
    """One activation tensor of a unit in the form(s) the unit's table gives it: `f32` (tensor or None) and / or `planes` (ops.H2 or
    None).  The recording helpers take an `Act` or a bare fp32 tensor and choose the kernel by the form of their operands."""
    __slots__ = ("name", "shape", "f32", "planes")

    def __init__(self, name, shape, f32=None, planes=None):
        self.name, self.shape, self.f32, self.planes = name, tuple(shape), f32, planes


def _act_of(x):
    return x if isinstance(x, Act) else Act(None, x.shape, x)


def _f32(x):
    return x.f32 if isinstance(x, Act) else x


def _planes_only(x):
    """the planes of a tensor that has no fp32 form, else None: a reader that can take either takes the fp32 tensor where there is one"""
    return x.planes if isinstance(x, Act) and x.f32 is None else None


def conv_out_hw(H, W, K, stride, pad):
    """output size of a K x K conv over an H x W map"""
    return ops.tap_out_size(H, K, stride, pad), ops.tap_out_size(W, K, stride, pad)


def zero_insert_hw(H, W, K, stride, pad, opad=0):
    """(q, Hu, Wu): a transposed conv (K, stride, pad, output_padding `opad`) of an H x W map -- or the input gradient of the strided conv
    with that geometry from its H x W output gradient -- is the stride-1 / pad-0 conv, taps flipped, of the map with stride - 1 zeros
    between its elements, q = K - 1 - pad around it and `opad` more behind it: Hu x Wu."""
    q = K - 1 - pad
    if q < 0:
        raise NotImplementedError("calibration engine: transposed conv with padding > kernel_size - 1")
    return q, ops.tap_out_size(H, K, stride, pad, True, opad) + K - 1, ops.tap_out_size(W, K, stride, pad, True, opad) + K - 1


def _split_lin(w, planes):
    ops.split_h2_linear(w, planes=planes)


def _split_conv(w, planes, row_groups=0):
    """by the format the buffer was allocated in: ops.H2 for the plane-input kernels (row_groups: `_Weights.row_groups`), bf16 three-way
    for the fp32-input ones"""
    if isinstance(planes, ops.H2):
        ops.split_h2_conv(w, planes=planes, row_groups=row_groups)
    else:
        ops.split_bf16x3(w, planes)


class _Weights:
    """One module's weight in the kernels' layouts, with every plane buffer the kernels may want of it: what the trainable `_Op` and
    the frozen `swin_engine._FpOp` share, so that `UnitEngine._conv` / `._dgrad` take either.  A subclass provides `wq` and, where
    it has an input gradient, `wd` (the weights the kernels read now, as `wq4()` / `wd4()`) and `plane_scale()`."""
    is_gdn = False
    is_mx = False                              # `_MxOp`: the AdaRound state lives on an MX grid (lo / gap in place of delta / zp)
    name = None                                # (a trainable op has one: its key in `UnitEngine.ops`)
    # plane buffer -> (the weight it is split from: an attribute or a method, how), in the order `split_planes` issues its launches; the
    # buffers are made on first use while a plan is being recorded
    PLANE_BUFFERS = {"lin_fwd": ("wq4", _split_lin),          # fragment-ordered fp16 planes of a Linear / 1 x 1 conv for rdo_linear_h2
                     "lin_bwd": ("wd4", _split_lin),          # (large token matrices)
                     "wp_planes": ("wp", _split_conv),        # of the phase weight of a transposed conv: bf16 three-way ...
                     "wp_h2": ("wp", _split_conv),            # ... and fp16 two-way
                     "wbp_planes": ("wbp", _split_conv),      # of the phase weight of a frozen strided conv's input gradient (bf16)
                     "wq_planes": ("wq4", _split_conv),       # of the weight ...
                     "wd_planes": ("wd4", _split_conv)}       # ... and of its dgrad layout

    def __init__(self, qm: QuantModule):
        self.qm = qm
        self.tconv = None                     # (stride, padding, output_padding) of a ConvTranspose2d
        self.tc_phase = self.wp = self.bias_p = self.wbp = self.wd = None
        # 4: a sub-pixel conv whose pixel shuffle sits in its kernel's stores (`UnitEngine._fb_gdn_block`, include/rdo_ptq_subpel.h) -- its
        # forward planes `wq_planes` and its gradient slabs have the rows in 4 groups, `bias_g` is the bias in that order; everything
        # else of the op (w, alpha, the Adam moments, wq, wd) keeps the logical row order.  Set while a plan is recorded.
        self.row_groups, self.bias_g = 0, None
        self.drop_planes()

    def drop_planes(self):
        for n in self.PLANE_BUFFERS:
            setattr(self, n, None)

    def _layout(self, bias):
        """w [co][kh][kw][ci], w4, rows, K, stride, pad, tconv, bias of a conv, a transposed conv or a Linear"""
        qm = self.qm
        w = qm.org_weight.detach()
        self.stride, self.pad = 1, 0
        if qm.kind == "linear":
            self.w = w.reshape(w.shape[0], 1, 1, w.shape[1]).contiguous()      # a Linear is a 1x1 conv over the token matrix
        elif qm.kind == "tconv":
            kw = qm.fwd_kwargs
            if kw["groups"] != 1 or tuple(kw["dilation"]) != (1, 1):
                raise NotImplementedError("calibration engine: grouped / dilated transposed convolutions")
            self.tconv = (int(kw["stride"][0]), int(kw["padding"][0]), int(kw["output_padding"][0]))
            # a transposed conv is the forward conv kernel (stride 1, pad 0) on the zero-inserted input with the taps
            # flipped: keep every per-weight tensor of the engine in that flipped [co][kh'][kw'][ci] layout
            self.w = to_rows(w, tconv=True).flip(1, 2).contiguous()
        else:
            self.w = to_rows(w)                # OHWI
            self.stride, self.pad = qm.conv_geometry()
        self.rows, self.K, self.w4 = self.w.shape[0], self.w.shape[1], tuple(self.w.shape)
        self.bias = None if bias is None else bias.detach().contiguous()

    def _init_phase(self):
        """Transposed conv whose output is stride x the input: run as a stride-1 conv with the "phase weight" [Cout * s^2][K'][K'][Cin]
        + pixel shuffle (include/rdo_ptq_hip.h, rdo_tconv_expand) instead of zero insertion + dense conv: `tc_phase` (None where the
        geometry does not allow it), `wp` from the current weights, `bias_p`."""
        self.tc_phase = ops.TconvPhase.get(self.K, *self.tconv, True, self.w.device)
        if self.tc_phase is not None:
            self.wp4 = self.tc_phase.w_shape(self.rows, self.w4[3])
            self.wp = torch.empty(self.wp4, device=self.w.device, dtype=torch.float32)
            self.bias_p = None if self.bias is None else self.bias.repeat_interleave(self.tc_phase.S2).contiguous()
            self.expand_phase()

    def expand_phase(self):
        """phase weight of a transposed conv (and its planes) from the current weights"""
        ops.tconv_expand(self.wq4(), self.tc_phase, out=self.wp)
        self.split_planes(("wp_planes", "wp_h2"))

    def split_planes(self, names=PLANE_BUFFERS):
        """split the current weights into every plane buffer of `names` that exists"""
        for n in names:
            planes = getattr(self, n)
            if planes is None:
                continue
            src, split = self.PLANE_BUFFERS[n]
            w = getattr(self, src)
            if n == "wq_planes" and self.row_groups:
                split(w() if callable(w) else w, planes, self.row_groups)
            else:
                split(w() if callable(w) else w, planes)

    def lin_planes(self, fwd: bool):
        """Planes of this Linear's weight (fwd) / of its transpose (input gradient) for rdo_linear_h2: allocated on first use -- while
        the plan is being recorded --, filled by `split_planes` (eagerly after the recording; a trainable op's then inside the plan behind
        every step)."""
        if self.qm.kind not in ("linear", "gdn") and not (self.qm.kind == "conv" and self.K == 1):
            raise RuntimeError("lin_planes: a Linear, a 1x1 conv or the 1x1 pool of a GDN")
        co, _, _, ci = self.w4
        scale = self.plane_scale()
        if fwd:
            if self.lin_fwd is None:
                self.lin_fwd = ops.H2(torch.empty((2, ci // 32, co // 16, 64, 8), device=self.w.device, dtype=torch.int16), scale)
            return self.lin_fwd
        if self.lin_bwd is None:
            self.lin_bwd = ops.H2(torch.empty((2, co // 32, ci // 16, 64, 8), device=self.w.device, dtype=torch.int16), scale)
        return self.lin_bwd

    def enable_planes(self, fwd: bool, dgrad: bool, h2: bool = False):
        """Allocate the plane buffers (called while the plan is being recorded: no kernel may run here; `split_planes` fills them once
        eagerly after the recording, and a trainable op's again inside the plan after every AdaRound step).  h2: fp16 two-way planes of
        w * plane_scale() for the plane-input kernels (conv_fwd_h2.hip); else the bf16 three-way planes of the fp32-input kernels."""
        def alloc(like, cur):
            if cur is not None:
                if isinstance(cur, ops.H2) != h2:
                    raise RuntimeError(f"calibration engine: op '{self.name}' needs its weight planes in two formats")
                return cur
            if h2:
                return ops.H2(torch.empty((2,) + tuple(like.shape), device=like.device, dtype=torch.int16), self.plane_scale())
            return torch.empty((3,) + tuple(like.shape), device=like.device, dtype=torch.int16)
        if fwd:
            self.wq_planes = alloc(self.wq, self.wq_planes)
        if dgrad and self.wd is not None:
            self.wd_planes = alloc(self.wd, self.wd_planes)

    def wq4(self):
        return self.wq.reshape(self.w4)

    def wd4(self):
        # [ci][kh][kw][co] for convs, gamma'^T viewed [C][1][1][C]
        co, kh, kw, ci = self.w4
        return self.wd.reshape(ci, kh, kw, co)


class _Op(_Weights):
    """Device state of one trainable QuantModule inside a unit: the AdaRound state in the kernel layout of its weight."""

    def __init__(self, name, qm: QuantModule, need_dgrad: bool):
        super().__init__(qm)
        self.name, self.need_dgrad = name, need_dgrad
        self.is_gdn = qm.kind == "gdn"
        self.is_ln = qm.kind == "layernorm"
        if qm.kind not in ("conv", "gdn", "tconv", "linear", "layernorm"):
            raise NotImplementedError(f"calibration engine: QuantModule kind '{qm.kind}' is not supported yet")
        wq = qm.weight_quantizer
        if not getattr(wq, "inited", True):    # (an AdaRoundQuantizer -- a unit calibrated before, in a second pass -- carries its scales)
            wq(qm.weight)                      # lazy scale init, as the reference's first forward would do
        if self.is_ln or self.is_gdn:
            w = qm.org_weight.detach()
            self.w = w.reshape(1, -1).contiguous() if self.is_ln else to_rows(w)     # gamma: one quantisation "channel" (per tensor) / [C,C]
            self.rows = self.w.shape[0]
            self.stride, self.pad, self.K = 1, 0, 1
            self.w4 = tuple(self.w.shape) if self.is_ln else (self.rows, 1, 1, self.rows)
            self.bias = None if (self.is_gdn or qm.bias is None) else qm.bias.detach().contiguous()
        else:
            self._layout(qm.bias)
        dev = self.w.device
        # layer-wise scales (main2.py without --channel_wise): one (delta, zero_point) repeated over the rows
        self.channel_wise = bool(wq.channel_wise)
        self.delta = wq.delta.reshape(-1).to(dev).expand(self.rows).contiguous()
        self.zp = wq.zero_point.reshape(-1).to(dev).expand(self.rows).contiguous()
        self.n_levels = wq.n_levels
        if self.is_gdn:
            self.inverse = bool(qm.fwd_kwargs["inverse"])
            self.beta, reparam = qm.gdn_constants()
            self.beta = self.beta.to(dev).contiguous()
            self.desc = ops.ada_desc(self.w, self.n_levels, reparam=reparam)
        else:
            self.desc = ops.ada_desc(self.w, self.n_levels, conv_layout=False) if self.is_ln else ops.ada_desc(self.w, self.n_levels)
        # bound of |soft-quantised weight| over the whole run (every level of every row's grid; through the GDN re-parametrisation
        # where there is one) -> the power-of-two scale of this op's fp16 weight planes
        lv = torch.maximum(self.zp.abs(), (self.n_levels - 1 - self.zp).abs()) * self.delta
        wb = float(lv.max())
        if self.is_gdn:
            wb = max(wb, float(self.desc.reparam_bound)) ** 2
        self.wscale = ops.pow2_scale(wb)
        self.alpha = torch.empty_like(self.w)
        self.m = torch.zeros_like(self.w)
        self.v = torch.zeros_like(self.w)
        self.wq = torch.empty_like(self.w)
        # wd: dgrad layout for convs, transpose for gamma (always needed: GDN backward uses gamma'^T)
        self.wd = torch.empty_like(self.w) if (need_dgrad or self.is_gdn) else None
        self.init_alpha()
        self.set_weight(True)
        self.slabs = self.slabs_p = None
        self.dalpha = None                     # data parallel: this op's view of the unit's gradient bucket (`UnitEngine._build_ops`)
        # phase form of a transposed conv: the AdaRound state stays in the kernel layout of the transposed conv; the phase weight is
        # re-expanded after every step, its gradient folded back
        if self.tconv is not None and os.environ.get("RDO_TCONV_PHASE", "1") != "0":
            self._init_phase()

    def plane_scale(self):
        return self.wscale

    def init_alpha(self):
        """alpha of round to nearest: where a unit starts and restarts"""
        ops.adaround_init_alpha(self.desc, self.w, self.delta, self.alpha)

    def set_weight(self, soft):
        """soft- or hard-rounded weight of the current alpha into wq / wd"""
        ops.adaround_fwd(self.desc, self.w, self.alpha, self.delta, self.zp, bool(soft), self.wq, self.wd)

    def step(self, eng, scale):
        """this op's own launch of the fused AdaRound step (the per-op path of `UnitEngine._step_ops`)"""
        ops.adaround_step(self.desc, self.w, self.delta, self.zp, self.slabs, scale, eng.weight, eng.sched, eng.it, self.alpha, self.m, self.v,
                          self.wq, self.wd, eng.round_log, self.wq_planes, self.wd_planes)

    def refresh_planes(self):
        """soft weights -> every plane buffer the recorded kernels read (the exact bf16 three-way splits of the split-bf16 MFMA path,
        the fp16 planes of the plane-input kernels): eagerly after the recording, then inside the plan behind every step"""
        self.split_planes()

    def numel(self):
        return self.w.numel()


class _MxOp(_Op):
    """A trainable QuantModule whose weight quantiser is an `mx.MXAdaRoundQuantizer`: the AdaRound state on the grid of an MX block
    format (include/rdo_ptq_mxround.h).  `lo` and `gap` (fp32, the layout of `w`) take the place of `delta` and `zp`; alpha, m, v, wq and
    wd are as in `_Op`.  The blocks run along the rows of `to_rows(weight, tconv)`, so the neighbours are computed on those rows and, for
    a transposed conv, flipped with the same `.flip(1, 2)` as every other tensor of the op (a block spans taps whenever Cin % 32 != 0)."""
    is_mx = True

    def __init__(self, name, qm: QuantModule, need_dgrad: bool):
        _Weights.__init__(self, qm)
        self.name, self.need_dgrad = name, need_dgrad
        self.is_gdn, self.is_ln = qm.kind == "gdn", False
        if qm.kind not in ("conv", "gdn", "tconv", "linear"):
            raise NotImplementedError(f"calibration engine: learned rounding on MX grids is not built for QuantModule kind '{qm.kind}'")
        q = qm.weight_quantizer
        self.fmt = q.fmt
        if self.is_gdn:
            self.w = to_rows(qm.org_weight.detach())
            self.rows = self.w.shape[0]
            self.stride, self.pad, self.K = 1, 0, 1
            self.w4 = (self.rows, 1, 1, self.rows)
            self.bias = None
        else:
            self._layout(qm.bias)
        self.channel_wise = True
        self.delta = self.zp = None
        self.n_levels = q.n_levels
        rows = to_rows(qm.org_weight.detach(), self.tconv is not None)            # unflipped: where the blocks are
        lo, gap = ops.mx_neighbours(rows.reshape(rows.shape[0], -1), self.fmt)
        lo, gap = lo.reshape(rows.shape), gap.reshape(rows.shape)
        if self.tconv is not None:
            lo, gap = lo.flip(1, 2), gap.flip(1, 2)
        self.lo, self.gap = lo.reshape(self.w.shape).contiguous(), gap.reshape(self.w.shape).contiguous()
        if self.is_gdn:
            self.inverse = bool(qm.fwd_kwargs["inverse"])
            self.beta, reparam = qm.gdn_constants()
            self.beta = self.beta.to(self.w.device).contiguous()
            self.desc = ops.ada_desc(self.w, self.n_levels, reparam=reparam)
        else:
            self.desc = ops.ada_desc(self.w, self.n_levels)
        # bound of |soft weight| over the whole run: both neighbours of every element (through the GDN re-parametrisation)
        wb = float(torch.maximum(self.lo.abs(), (self.lo + self.gap).abs()).max())
        if not math.isfinite(wb):
            raise ValueError(f"calibration engine: the weight of op '{name}' is not finite")
        if self.is_gdn:
            wb = max(wb, float(self.desc.reparam_bound)) ** 2
        self.wscale = ops.pow2_scale(wb)
        self.alpha = torch.empty_like(self.w)
        self.m = torch.zeros_like(self.w)
        self.v = torch.zeros_like(self.w)
        self.wq = torch.empty_like(self.w)
        self.wd = torch.empty_like(self.w) if (need_dgrad or self.is_gdn) else None
        self.init_alpha()
        self.set_weight(True)
        self.slabs = self.slabs_p = None
        self.dalpha = None
        if self.tconv is not None and os.environ.get("RDO_TCONV_PHASE", "1") != "0":
            self._init_phase()

    def init_alpha(self):
        ops.mx_round_init_alpha(self.w, self.lo, self.gap, self.alpha)

    def set_weight(self, soft):
        ops.mx_round_fwd(self.desc, self.lo, self.gap, self.alpha, bool(soft), self.fmt, wq=self.wq, wd=self.wd)

    def step(self, eng, scale):
        ops.mx_round_step(self.desc, self.lo, self.gap, self.slabs, scale, eng.weight, eng.sched, eng.it, self.alpha, self.m, self.v,
                          self.wq, self.wd, eng.round_log)


def _make_op(name, qm, need_dgrad):
    from .mx import is_mx_learned
    return (_MxOp if is_mx_learned(qm.weight_quantizer) else _Op)(name, qm, need_dgrad)


class UnitEngine(DpLoop, RdTask):
    def __init__(self, kind, modules, cache_q, cache_fp, cache_out, *, batch_size, iters, weight=0.01, b_range=(20, 2),
                 warmup=0.2, input_prob=0.5, lr=1e-3, seed=0, idx_table=None, include_act_func=True, group=None,
                 use_graph=True, force_dp_split=False, task_p=2.0, batch_offset=0, dp_overlap=None, fuse_tail=True, batch_step=True, use_h2=True, rd=None):
        if kind not in UNIT_KINDS:
            raise NotImplementedError(f"calibration engine: unit kind '{kind}'")
        for t in (cache_q, cache_fp, cache_out):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4):
                raise RuntimeError("calibration engine: caches must be contiguous fp32 NHWC CUDA tensors")
        self.kind, self.mods = kind, modules
        self.cq, self.cf, self.co = cache_q, cache_fp, cache_out
        self.B, self.iters = int(batch_size), int(iters)
        self.task_p = float(task_p)            # exponent of the task term (main2.py --task_loss); rec_loss is always p = 2
        self.weight, self.input_prob, self.seed = float(weight), float(input_prob), int(seed) & 0xFFFFFFFF
        self.include_act = include_act_func
        self.use_graph = use_graph
        self.batch_offset = int(batch_offset)  # first row of this rank's share of the global mini-batch (QDrop counter)
        self.dp_overlap = None if dp_overlap is None else bool(dp_overlap)
        if os.environ.get("RDO_USE_H2") is not None:
            use_h2 = os.environ["RDO_USE_H2"] != "0"      # A/B switch for whole runs (bench.py)
        self.use_h2 = bool(use_h2)             # big units on H2 tensors (plane-input LDS-DMA GEMM kernels); False: fp32 activations only
        self.P = {}                            # name -> planes of the H2 form of an activation buffer
        self.batch_step = bool(batch_step)     # one AdaRound-step launch per unit (False: one per weight tensor)
        self.fuse_splitk = os.environ.get("RDO_FUSE_SPLITK", "1") != "0"   # split-K conv + unit tail: the conv's second pass inside the tail
        self.fuse_h2_tail = os.environ.get("RDO_H2_TAIL", "1") != "0"       # last conv of a H2 ResidualBlock unit + its tail in one launch
        self.fold_iter = os.environ.get("RDO_FOLD_ITER", "1") != "0"     # iteration-counter hand-over instead of an increment launch
        # round 6: the NEXT iteration's mini-batch is assembled by the AdaRound-step launch (rdo_adaround_step_batch_gather) -- one launch
        # less per iteration, the gather's stream under the step's latency; iteration 0's mini-batch by a stand-alone gather (`_prime`)
        self.fold_gather = os.environ.get("RDO_GATHER_IN_STEP", "1") != "0"
        # the GDN / IGDN block of an RBWS / RBU unit -- norm pool, loss tail, gamma'^T GEMM and dx -- in one launch (ops.gdn_fwd_bwd) where
        # both GEMMs would run on rdo_linear_h2; 0: the four launches
        self.gdn_fused = os.environ.get("RDO_GDN_FUSED", "1") != "0"
        # the four pixel (un)shuffles of an RBU unit in the stores of the kernels that write their inputs (the two sub-pixel convs, the
        # one-launch GDN block, the dgrad of the 3 x 3 conv: `_fb_gdn_block`); 0: a launch each
        self.subpel_fused = os.environ.get("RDO_SUBPEL_FUSED", "1") != "0"
        self._next_gather = None
        self._rd_init(rd, include_act_func)    # opt-in R + lambda*D task loss (loss_mode='rd', engine_rd.RdTask): separate kernels, fp32
        if rd is not None:
            fuse_tail = self.use_h2 = False
        self.fuse_tail = bool(fuse_tail)       # False: the separate epilogue / loss / activation-backward kernels (A/B, tests)
        self.dev = cache_q.device
        n = cache_q.shape[0]
        if idx_table is None and self.B > n:
            # fewer cached samples than the batch: the reference's randperm(n)[:batch_size] simply yields all n (layer_opt.py:289)
            self.B = n
        if idx_table is None:
            # same CPU-generator stream as the reference: one torch.randperm(n) per iteration (layer_opt.py:289)
            idx_table = IdxStream.take(n, self.B, self.iters)
        idx_table = torch.as_tensor(idx_table).to(torch.int32)
        if tuple(idx_table.shape) != (self.iters, self.B):
            raise ValueError(f"idx_table must be [{self.iters},{self.B}], got {tuple(idx_table.shape)}")
        if int(idx_table.max()) >= n or int(idx_table.min()) < 0:
            raise ValueError("idx_table refers to images outside the cache")
        self.idx = idx_table.to(self.dev).contiguous()
        self.sched = ops.make_sched(self.iters, warmup, b_range, lr, self.dev)
        # iteration counter and its shadow (rdo_ptq_hip.h, "iteration-counter hand-over"): when the unit's AdaRound step is one batched
        # launch it leaves it + 1 in the shadow and the next gather publishes it -- no separate increment launch
        self._it2 = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self.it, self.it_shadow = self._it2[0:1], self._it2[1:2]
        self.loss_log = torch.zeros(self.iters, L.LOG_SLOTS, device=self.dev)      # kernels spread atomics over the slots
        self.task_log = torch.zeros(self.iters, L.LOG_SLOTS, device=self.dev)      # task term where it is a separate quantity
        self._task_is_rec = False              # True: task == rec on the same tensors, both logged as 2 * rec in loss_log
        self.round_log = torch.zeros(self.iters, L.LOG_SLOTS, device=self.dev)
        self.group = group
        self.world = 1
        if group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(group)
        # the data-parallel op sequence (grad -> all-reduce -> apply) can be forced on a single rank to test it
        self.split = self.world > 1 or force_dp_split
        self._dp_init()
        # this unit's own fp16-overflow word (rdo_h2_bind_flag): raised by every H2 producer of its plans, polled during long runs
        # (pairs: finite magnitude, non-finite mark; pair 0 for the weight planes, one pair per activation tensor kept as planes)
        self._ovf = torch.zeros(2 * self.OVF_PAIRS, dtype=torch.int32, device=self.dev)
        self._ovf_slot = {}                    # plane tensor name -> its pair
        self.h2_restarts = 0                   # times the unit was restarted after an overflow (0 in every measured run so far)
        self._done = 0
        self._ovf_checked = -1                 # position (`_done`) at which the rank-synchronised overflow verdict was last formed
        with ops.h2_flag(self._ovf[0:2]):
            self._build_ops()
            self._alloc()
            self.forms = {}                    # activation buffer name -> form, where it is not F32 (`_forms`; set per recording)
            self.scales = {}                   # activation buffer name -> power-of-two scale of its H2 planes
            self._amax = {}                    # ... and the magnitude it was derived from
            self._probing = False
            self._probe_scales()
            self._start()

    def _start(self):
        """record the plans at the current scales and make the unit ready for the iteration its counter stands at"""
        self._record()
        for op in self.ops.values():
            op.refresh_planes()          # current soft weights -> planes (eager, before the first iteration)
        self._prime()                    # folded gather: the mini-batch of that iteration

    # ------------------------------------------------------------------------------------------------------------------
    def _build_ops(self):
        m, k = self.mods, self.kind
        o = OrderedDict()
        if k == "layer":
            o["layer"] = _make_op("layer", m["layer"], False)
        elif k == "rb":
            o["conv1"] = _make_op("conv1", m["conv1"], False)
            o["conv2"] = _make_op("conv2", m["conv2"], True)
            if m.get("skip") is not None:
                o["skip"] = _make_op("skip", m["skip"], False)
        elif k == "rbws":
            o["conv1"] = _make_op("conv1", m["conv1"], False)
            o["conv2"] = _make_op("conv2", m["conv2"], True)
            o["gdn"] = _make_op("gdn", m["gdn"], False)
            if m.get("skip") is not None:
                o["skip"] = _make_op("skip", m["skip"], False)
        elif k == "rbu":
            o["subpel_conv"] = _make_op("subpel_conv", m["subpel_conv"], False)
            o["conv"] = _make_op("conv", m["conv"], True)
            o["igdn"] = _make_op("igdn", m["igdn"], False)
            o["upsample"] = _make_op("upsample", m["upsample"], False)
        for op in o.values():
            if op.need_dgrad and (op.stride != 1 or 2 * op.pad != op.K - 1):
                raise NotImplementedError("calibration engine: dgrad is built for stride-1 'same' convolutions only")
        mx = [n for n, op in o.items() if op.is_mx]
        if mx and len(mx) != len(o):
            raise NotImplementedError(f"calibration engine: ops {mx} are on MX grids and {[n for n in o if n not in mx]} on integer grids: "
                                      "a unit is calibrated on one kind of grid")
        if mx and (self.split or self.rd is not None):
            # the MX step is the per-op fused launch only (rdo_mx_round_step): no gradient-only / apply pair, no batched form
            raise NotImplementedError("calibration engine: learned rounding on MX grids is not built for " +
                                      ("data-parallel calibration (world_size > 1)" if self.split else "loss_mode='rd'"))
        self.ops = o
        # Data parallel: one flat bucket of d(rec+task)/d(alpha) per unit.  The op whose weight gradient is the LAST kernel of the
        # backward pass (the block's first conv) sits at the end of the bucket: everything in front of it is complete before that
        # wgrad starts, so its all-reduce overlaps the wgrad (two recorded plans, `_split_point`).
        # Only where that last wgrad is long enough to hide a collective behind (>= 64^2 activations at batch 4): on the small units
        # the second all-reduce and the second gradient launch cost more than the overlap saves.
        late = {"rb": "conv1", "rbws": "conv1", "rbu": "subpel_conv"}.get(k)
        overlap = self.dp_overlap
        if overlap is None and late is not None:   # default: by the size of that last weight gradient; True / False force it (tests, A/B)
            lo = o[late]
            ho, wo = self._out_hw(lo, self.cq.shape[1], self.cq.shape[2])
            overlap = 2.0 * self.B * ho * wo * lo.numel() >= self.DP_OVERLAP_MIN_FLOP
        self._late = late if (self.split and overlap and self.rd is None) else None
        if self.split:
            self.bucket = dp.GradBucket(OrderedDict((n, op.numel()) for n, op in o.items()), late=self._late, device=self.dev, group=self.group)
            for n, op in o.items():
                op.dalpha = self.bucket.view(n)

    def _buf(self, *shape):
        return torch.empty(shape, device=self.dev, dtype=torch.float32)

    def _out_hw(self, op, H, W):
        return conv_out_hw(H, W, op.K, op.stride, op.pad)

    def _alloc(self):
        B = self.B
        _, H, W, Cin = self.cq.shape
        self.x_in = self._buf(B, H, W, Cin)
        o, t = self.ops, {}
        if self.kind == "layer":
            op = o["layer"]
            if op.tc_phase is not None:
                s_ = op.tc_phase.stride
                Ho, Wo = H * s_, W * s_
                t["yp"] = self._buf(B, H, W, op.wp4[0])
                t["dyp"] = self._buf(B, H, W, op.wp4[0])
            elif op.tconv is not None:
                q_, Hu, Wu = zero_insert_hw(H, W, op.K, *op.tconv)
                t["xu"] = self._buf(B, Hu, Wu, Cin)
                self.tc_geom = (op.tconv[0], q_, Hu, Wu)
                Ho, Wo = Hu - op.K + 1, Wu - op.K + 1
            elif op.is_gdn:
                Ho, Wo = H, W
                t["norm"] = self._buf(B, H, W, Cin)
                t["t"] = self._buf(B, H, W, Cin)
            else:
                Ho, Wo = self._out_hw(op, H, W)
            t["y"] = self._buf(B, Ho, Wo, op.rows)
            t["dy"] = self._buf(B, Ho, Wo, op.rows)
            t["dpre"] = self._buf(B, Ho, Wo, op.rows)
        elif self.kind == "rb":
            C = o["conv1"].rows
            for n_ in ("h1", "pre2", "out", "dout", "dpre2", "dh1"):
                t[n_] = self._buf(B, H, W, C)
            if "skip" in o:
                t["sk"] = self._buf(B, H, W, C)
        elif self.kind == "rbws":
            c1 = o["conv1"]
            Ho, Wo = self._out_hw(c1, H, W)
            C = c1.rows
            for n_ in ("h1", "c2", "out", "dout", "t", "dc2", "dh1"):      # (norm, acc: `_tmp`, where the GDN block is not one launch)
                t[n_] = self._buf(B, Ho, Wo, C)
            if "skip" in o:
                t["sk"] = self._buf(B, Ho, Wo, C)
        elif self.kind == "rbu":
            sp = o["subpel_conv"]
            C4 = sp.rows
            r = int(self.mods["upscale"])
            C = C4 // (r * r)
            # (sp = lrelu(subpel conv) before the shuffle, up, dout and dh1 only feed a pixel (un)shuffle launch: `_tmp`)
            t["h1"] = self._buf(B, H * r, W * r, C)
            t["ups"] = self._buf(B, H * r, W * r, C)
            for n_ in ("c", "out", "t", "dc"):
                t[n_] = self._buf(B, H * r, W * r, C)
            t["dsp"] = self._buf(B, H, W, C4)
            t["dup"] = self._buf(B, H, W, C4)
            self.r = r
        self.t = t
        for op in self.ops.values():
            op.slabs = None     # allocated at record time when the activation shapes are known

    GDN_TMP = ("norm", "acc")
    SUBPEL_TMP = ("sp", "up", "dout", "dh1")

    def _tmp(self, name, like):
        """`norm` / `acc` of an RBWS / RBU unit: they only carry values from one launch of the GDN block to the next, so they are made
        on first use -- by the probe iterations and by a plan that runs the block as separate launches -- and not at all by a plan
        that runs it as one (`_fb_gdn_block`).  The same for the inputs of an RBU unit's four pixel (un)shuffle launches (SUBPEL_TMP)
        and a plan that has those in its kernels' stores."""
        if name not in self.t:
            self.t[name] = self._buf(*like.shape)
        return self.t[name]

    def _slabs(self, op, x_shape):
        ns = ops.wgrad_nsplit(tuple(x_shape), op.w4, op.stride, op.pad)
        op.slabs = self._buf(ns, *op.w4)
        return op.slabs

    # ------------------------------------------------------------------------------------------------------------------
    lin_conv = os.environ.get("RDO_CONV1X1_LIN_H2", "1") != "0"

    def _lin_conv_ok(self, op, x):
        """A 1 x 1 / stride 1 conv over a large pixel matrix is a token-matrix Linear: rdo_linear_h2 (per-pixel dynamic scale, no probed scale)
        instead of the fp32 / split-bf16 conv kernels -- the 192 <-> 96 convs of Cheng2020-attn's attention blocks (BASELINE config 3)."""
        if not (self.lin_conv and not self._probing and op.qm.kind == "conv" and op.K == 1 and op.stride == 1 and op.pad == 0 and op.tconv is None):
            return False
        C = x.shape[-1]
        rows = math.prod(x.shape[:-1])
        return rows >= self.LIN_GDN_MIN_ROWS and ops.linear_h2_supported(rows, C, op.w4[0])

    unit1x1 = int(os.environ.get("RDO_UNIT1X1", "2"))       # 0 off, 1 only 16^2 maps and K = 96, 2 wherever the shape is supported (default)

    def _unit1x1_ok(self, op, x):
        """A plain 1 x 1 / stride-1 conv as a LAYER unit with the default objective: rdo_unit1x1 (forward + tail + weight-gradient slabs in
        one launch; on split fp16 where Cout is a multiple of 96, else in exact fp32: ops.unit1x1_form) -- the 192 <-> 96 convs of
        Cheng2020-attn's attention blocks (BASELINE config 3)."""
        if not (self.unit1x1 and self.fused and self.include_act and self.kind == "layer" and op.qm.kind == "conv" and op.K == 1
                and op.stride == 1 and op.pad == 0 and op.tconv is None and not op.is_gdn):
            return False
        M, K = math.prod(x.shape[:-1]), x.shape[-1]
        # per unit-iteration inside the config-3 schedule (us, three launches -> one): 16^2 maps 31 -> 29 (192 -> 96), 29 -> 22 (96 -> 192),
        # 32 -> 30 (192 -> 192); 64^2 maps 54 -> 47 at K = 96; at K = 192 on the 64^2 maps the first version (serial load / store loops) lost to
        # rdo_linear_h2 + linear_wgrad_h2 (54 -> 58), with its loads batched it wins there too: schedule 9.13 (off) / 8.81 (K = 96 and 16^2
        # only: RDO_UNIT1X1=1) / 8.76 ms per step (everywhere: the default, 2)
        return (self.unit1x1 == 2 or M <= 4096 or K <= 96) and ops.unit1x1_supported(M, K, op.w4[0])

    def _conv(self, op, x, out, epilogue=L.EPI_NONE, aux=None, residual=None, pre=None, square=False, bias=True):
        """out = (epilogue of) the conv of x with op's soft weights.  x as planes: the plane-input kernel, which writes `out` as fp32 and /
        or planes; else the fp32-input kernels (planes of `out` then by a split of their own)."""
        x, out = _act_of(x), _act_of(out)
        b = (op.beta if op.is_gdn else op.bias) if bias else None
        if x.planes is not None:
            op.enable_planes(True, False, h2=True)
            return ops.conv2d_fwd_h2(x.planes, x.shape, op.w4, op.wq_planes, b, op.stride, op.pad, epilogue=epilogue, aux=_f32(aux),
                                     residual=_f32(residual), out=out.f32, pre=_f32(pre), out_planes=out.planes)
        if epilogue == L.EPI_NONE and aux is None and residual is None and pre is None and not square and self._lin_conv_ok(op, x):
            return ops.linear_h2(x.f32.view(-1, x.shape[-1]), op.lin_planes(True), b, out=out.f32.view(-1, out.shape[-1]))
        if ops.uses_bf16x6(x.shape, op.w4, op.stride, op.pad):
            op.enable_planes(True, False)
        y = ops.conv2d_fwd(x.f32, op.wq4(), b, op.stride, op.pad, epilogue=epilogue, aux=_f32(aux), residual=_f32(residual),
                           square_input=square, out=out.f32, pre=_f32(pre), wplanes=op.wq_planes)
        if out.planes is not None:
            ops.split_h2(out.f32, out.planes)
        return y

    def _wgrad_into(self, slabs, x, dy, w4, stride, pad, square=False):
        """weight-gradient slabs of a conv from its input and its output gradient: the plane kernel when both come as planes"""
        x, dy = _act_of(x), _act_of(dy)
        if x.planes is not None and dy.planes is not None:
            ops.conv2d_wgrad_h2(x.planes, x.shape, dy.planes, w4, stride, pad, slabs=slabs)
        else:
            ops.conv2d_wgrad(x.f32, dy.f32, w4, stride, pad, square_input=square, slabs=slabs)

    def _wgrad(self, op, x, dy, square=False):
        if op.slabs is None:
            self._slabs(op, x.shape)
        self._wgrad_into(op.slabs, x, dy, op.w4, op.stride, op.pad, square)

    def _dgrad(self, op, dy, out, epilogue=L.EPI_NONE, aux=None):
        """out = (epilogue of) the input gradient of op's conv; `aux` (the tensor whose sign the LeakyReLU mask needs) as fp32, else its
        planes (the sign is read off plane 0)"""
        dy, out = _act_of(dy), _act_of(out)
        wd4, pad = tuple(op.wd4().shape), op.K - 1 - op.pad
        if dy.planes is not None:
            op.enable_planes(False, True, h2=True)
            return ops.conv2d_fwd_h2(dy.planes, dy.shape, wd4, op.wd_planes, None, 1, pad, epilogue=epilogue, aux=_f32(aux),
                                     aux_planes=_planes_only(aux), out=out.f32, out_planes=out.planes)
        if ops.uses_bf16x6(dy.shape, wd4, 1, pad):
            op.enable_planes(False, True)
        return ops.conv2d_fwd(dy.f32, op.wd4(), None, 1, pad, epilogue=epilogue, aux=_f32(aux), out=out.f32, wplanes=op.wd_planes)

    # ---- the two 1x1 GEMMs of a GDN / IGDN (norm pool beta' + gamma' . x^2 and, backward, t . gamma'): token-matrix Linears over the
    # channels.  From LIN_GDN_MIN_ROWS pixels on they run on rdo_linear_h2 (per-pixel dynamic scale, three fp16 products) instead of the
    # conv kernels (split-bf16 six products at 128^2, fp32 MFMA tiles below).  RDO_GDN_LIN_H2=0 switches it off.
    LIN_GDN_MIN_ROWS = int(os.environ.get("RDO_GDN_LIN_MIN_ROWS", 4096))
    lin_gdn = os.environ.get("RDO_GDN_LIN_H2", "1") != "0"

    def _gdn_lin_ok(self, g, x):
        C = x.shape[-1]
        rows = math.prod(x.shape[:-1])
        return (self.lin_gdn and not self._probing and rows >= self.LIN_GDN_MIN_ROWS and g.w4[0] == C and ops.linear_h2_supported(rows, C, C))

    def _gdn_pool(self, g, x, norm):
        """norm = beta' + gamma' . x^2"""
        if self._gdn_lin_ok(g, x):
            C = x.shape[-1]
            return ops.linear_h2(x.view(-1, C), g.lin_planes(True), g.beta, out=norm.view(-1, C), square_input=True)
        return self._conv(g, x, norm, square=True)

    def _gdn_acc(self, g, tbuf, acc):
        """acc = t . gamma'   (wd = gamma'^T as [C][1][1][C]): rdo_linear_h2 over the fp32 t where that applies (`_forms` then keeps t
        off planes), else the 1 x 1 "input gradient" of the pool"""
        tbuf = _act_of(tbuf)
        if tbuf.planes is None and self._gdn_lin_ok(g, tbuf):
            C = tbuf.shape[-1]
            return ops.linear_h2(tbuf.f32.view(-1, C), g.lin_planes(False), None, out=acc.view(-1, C))
        return self._dgrad(g, tbuf, acc)

    def _tconv_forward(self, op, x, y, epilogue=L.EPI_NONE):
        """y [B, sH, sW, Cout] <- (activation of) the transposed conv of x with the soft weights: stride-1 conv with the phase weight,
        then the pixel shuffle (LeakyReLU / ReLU commute with it)."""
        ph, x = op.tc_phase, _act_of(x)
        if x.planes is not None:
            if op.wp_h2 is None:
                op.wp_h2 = ops.H2(torch.empty((2,) + tuple(op.wp4), device=self.dev, dtype=torch.int16), op.wscale)
            ops.conv2d_fwd_h2(x.planes, x.shape, op.wp4, op.wp_h2, op.bias_p, 1, ph.pad, epilogue=epilogue, out=self.t["yp"])
        else:
            if ops.uses_bf16x6(x.shape, op.wp4, 1, ph.pad) and op.wp_planes is None:
                op.wp_planes = torch.empty((3,) + tuple(op.wp4), device=self.dev, dtype=torch.int16)
            ops.conv2d_fwd(x.f32, op.wp, op.bias_p, 1, ph.pad, epilogue=epilogue, out=self.t["yp"], wplanes=op.wp_planes)
        self._shuffle(self.t["yp"], ph.stride, y)

    def _tconv_wgrad(self, op, x, dy):
        """slabs of dL/d(kernel-layout weight) from dy [B, sH, sW, Cout]: unshuffle, weight gradient of the phase conv, fold"""
        ph, dyp = op.tc_phase, self._act("dyp")
        self._unshuffle(dy, ph.stride, dyp)
        if op.slabs is None:
            ns = ops.wgrad_nsplit(tuple(x.shape), op.wp4, 1, ph.pad)
            op.slabs_p = self._buf(ns, *op.wp4)
            op.slabs = self._buf(ns, *op.w4)
        self._wgrad_into(op.slabs_p, x, dyp, op.wp4, 1, ph.pad)
        ops.tconv_fold(op.slabs_p, ph, op.rows, op.w4[3], out=op.slabs)

    def _after_step(self, lin_done=False):
        """recorded right behind the AdaRound step: phase weights of transposed convs follow the new soft weights (lin_done: the batched
        step has written the rdo_linear_h2 planes itself)"""
        for op in self.ops.values():
            if op.tc_phase is not None:
                op.expand_phase()
            if not lin_done:
                op.split_planes(("lin_fwd", "lin_bwd"))    # Linears on rdo_linear_h2: fragment-ordered planes of the new soft weights

    def _loss(self, pred, grad):
        if self.rd is not None:
            # rec_loss here; the task term is the rate-distortion loss of the whole model, evaluated on the host's tape between the
            # two recorded plans and added to the gradient at the top of the second one
            ops.lp2_loss_grad(pred, self.co, self.idx, self.it, 1.0, grad, self.loss_log)
            self._rd_pred = pred
            self.g_task = torch.zeros_like(pred)
            self.plan_rd = self._next_plan()
            ops.add(grad, self.g_task, out=grad)
            return
        # rec_loss + task_loss on the same tensors (fp_out is the identity for these coders)
        if self.task_p == 2.0:
            self._task_is_rec = True
            ops.lp2_loss_grad(pred, self.co, self.idx, self.it, 2.0, grad, self.loss_log)
        else:
            ops.lp_loss_grad(pred, self.co, self.idx, self.it, 1.0, 1.0, self.task_p, grad, self.loss_log, self.task_log)

    @property
    def fused(self):
        """Fused unit tails (csrc/fused_tail.hip) cover the reference's default objective: rec_loss + task_loss with exponent 2."""
        return self.task_p == 2.0 and self.fuse_tail

    def _shuffle(self, x, r, out):
        out = _act_of(out)
        if out.planes is not None or (r == 2 and x.shape[-1] % 16 == 0):
            return ops.pixel_shuffle_h2(x, out=out.f32, out_planes=out.planes)
        return ops.pixel_shuffle(x, r, out.f32)

    def _unshuffle(self, x, r, out):
        x, out = _f32(x), _act_of(out)
        if out.planes is not None or (r == 2 and x.shape[-1] % 4 == 0):
            return ops.pixel_unshuffle2(x, out.f32, out_planes=out.planes)
        return ops.pixel_unshuffle(x, r, out.f32)

    def _tail_act(self, pre, res, act, dpre, gout=None):
        """out = act(pre) + res, rec + task loss against the cached FP output, dL/dout (if wanted) and dL/dpre in one pass.  A residual
        that exists as planes only is summed back from them (exactly)."""
        dpre = _act_of(dpre)
        self._task_is_rec = True
        ops.loss_act_bwd(_f32(pre), _f32(res), self.co, self.idx, self.it, 2.0, act, self.loss_log, grad_out=gout, dpre=dpre.f32, dpre_planes=dpre.planes,
                         residual_planes=_planes_only(res))

    def _conv_tail(self, op, x, pre, res, act, dpre, gout=None):
        """Last conv of a unit + its fused tail.  On planes with `pre` None (`_forms`): one launch, the pre-activation never reaches
        memory.  On fp32, when the conv is split over K, its second pass (sum the partial slabs, add the bias) moves into the tail's
        first load: one launch and one round trip of the pre-activation tensor less."""
        x = _act_of(x)
        if x.planes is not None and pre is None:
            op.enable_planes(True, False, h2=True)
            self._task_is_rec = True
            ops.conv2d_fwd_h2_tail(x.planes, x.shape, op.w4, op.wq_planes, op.bias, op.stride, op.pad, res.planes, self.co, self.idx, self.it,
                                   2.0, act, dpre.planes, self.loss_log)
            return
        if x.planes is not None or self._lin_conv_ok(op, x):   # (or a 1 x 1 conv over a large pixel matrix: rdo_linear_h2, then the tail)
            self._conv(op, x, pre)
            self._tail_act(pre, res, act, dpre, gout=gout)
            return
        x, res = x.f32, _f32(res)
        if ops.uses_bf16x6(tuple(x.shape), op.w4, op.stride, op.pad):
            op.enable_planes(True, False)
        ks, _ = ops.conv_fwd_ksplit(tuple(x.shape), op.w4, op.stride, op.pad, op.wq_planes is not None, self.dev)
        if self.fuse_splitk and ks >= 2 and not op.is_gdn and pre.shape[-1] % 4 == 0:      # quads of channels (bias, partial sums)
            ws, ks = ops.conv2d_fwd_partials(x, op.wq4(), op.stride, op.pad, wplanes=op.wq_planes)
            self._task_is_rec = True
            ops.loss_act_bwd_splitk(ws, ks, op.bias, tuple(pre.shape), res, self.co, self.idx, self.it, 2.0, act, self.loss_log,
                                    grad_out=gout, dpre=_f32(dpre))
            return
        self._conv(op, x, pre)
        self._tail_act(pre, res, act, dpre, gout=gout)

    def _tail_gdn(self, x, norm, res, inverse, gout, tbuf):
        tbuf = _act_of(tbuf)
        self._task_is_rec = True
        ops.loss_gdn_bwd(x, norm, _f32(res), self.co, self.idx, self.it, 2.0, inverse, self.loss_log, gout, t=tbuf.f32, t_planes=tbuf.planes)

    # ------------------------------------------------------------------------------------------------------------------ H2 path
    # FLOPs of the unit's last weight gradient from which the bucket all-reduce is split in two (see _build_ops): 43.5 GFLOP (~200 us)
    # for the 3x3 convs of the 128^2 units hides a collective; 10.9 GFLOP (~45 us, the 64^2 units) is about the latency of the second
    # all-reduce the split adds, and the 3 -> 192 stem of g_a.0 is 26 us
    DP_OVERLAP_MIN_FLOP = 30e9
    # plane-input kernels from this many output elements of the conv (pixels x channels) on
    H2_MIN_OUT = int(os.environ.get("RDO_H2_MIN_OUT", 4096 * 192))
    h2_lean = os.environ.get("RDO_H2_LEAN", "1") != "0"     # tensors whose only readers take planes are not also written as fp32
    layer_h2 = os.environ.get("RDO_LAYER_H2", "1") != "0"   # plain k x k layer units over enough pixels on the plane kernels (plan "layer")

    OVF_PAIRS = 8

    # the planes of dyp (dL/dpre of a phase-form transposed conv, unshuffled) go by the name of dpre: a permutation of the same values,
    # so the magnitude probed on dpre gives their scale, and their overflow words are dpre's
    PLANES_AS = {"dyp": "dpre"}

    def _act(self, name):
        """Activation buffer `name` of this unit in the form(s) `self.forms` gives it (None: not in memory).  Planes are made on first
        use: scale from the probe iterations, their own overflow words (pairs handed out in that order)."""
        buf = self.x_in if name == "x" else self.t[name]
        form = self.forms.get(name, F32)
        if form == ABSENT:
            return None
        planes = None
        if form & PLANES:
            pname = self.PLANES_AS.get(name, name)
            if pname not in self.P:
                k = self._ovf_slot.setdefault(pname, 1 + len(self._ovf_slot))
                self.P[pname] = ops.h2_empty(buf.shape, self.dev, self.scales[pname], flag=self._ovf[2 * k:2 * k + 2])
            planes = self.P[pname]
        return Act(name, buf.shape, buf if form & F32 else None, planes)

    def _conv_ok_h2(self, op, x_shape, dgrad=False):
        if dgrad:
            w4, stride, pad = tuple(op.wd4().shape), 1, op.K - 1 - op.pad
        else:
            w4, stride, pad = op.w4, op.stride, op.pad
        if not ops.conv_h2_supported(tuple(x_shape), w4, stride, pad):
            return False
        d = ops.conv_desc(tuple(x_shape), w4, stride, pad)
        return d.B * d.Ho * d.Wo * d.Cout >= self.H2_MIN_OUT

    def _plan_h2(self):
        """Which big convs of this unit run on H2 tensors (decided once, at record time)."""
        o, k = self.ops, self.kind
        if not (self.use_h2 and self.fused):
            return None
        xs = tuple(self.x_in.shape)
        if k == "layer":
            # a transposed conv in phase form (stride 2): the 3 x 3 phase conv and its weight gradient on planes
            op = o["layer"]
            if (op.tc_phase is not None and op.tc_phase.stride == 2 and xs[-1] % 16 == 0 and ops.conv_h2_supported(xs, op.wp4, 1, op.tc_phase.pad)
                    and ops.wgrad_h2_supported(xs, op.wp4, 1, op.tc_phase.pad) and xs[0] * xs[1] * xs[2] * op.wp4[0] >= self.H2_MIN_OUT):
                return "tconv"
            # a plain k x k conv (k > 1) over enough pixels -- the 3 x 3 96 -> 96 convs of Cheng2020-attn's attention blocks at 64^2 (BASELINE
            # config 3; fp32 MFMA 50 + 65 us forward + weight gradient, planes 40 + 32: tools/bench_layer96.py): input and dL/dpre as planes
            if (self.layer_h2 and op.tconv is None and not op.is_gdn and op.qm.kind == "conv" and op.K > 1 and xs[-1] % 16 == 0
                    and "dpre" in self.t and self._conv_ok_h2(op, xs) and ops.wgrad_h2_layer_supported(xs, op.w4, op.stride, op.pad)):
                return "layer"
            return None
        if k == "rb" and "skip" not in o:
            c1, c2 = o["conv1"], o["conv2"]
            hs = tuple(self.t["h1"].shape)
            if (self._conv_ok_h2(c1, xs) and self._conv_ok_h2(c2, hs) and self._conv_ok_h2(c2, hs, dgrad=True)
                    and ops.wgrad_h2_supported(xs, c1.w4, c1.stride, c1.pad) and ops.wgrad_h2_supported(hs, c2.w4, 1, c2.pad)):
                return "rb"
        if k in ("rbws", "rbu"):
            cv, g = (o["conv2"], o["gdn"]) if k == "rbws" else (o["conv"], o["igdn"])
            hs = tuple(self.t["h1"].shape)
            if (hs[-1] % 16 == 0 and (k != "rbu" or self.r == 2) and self._conv_ok_h2(cv, hs) and self._conv_ok_h2(cv, hs, dgrad=True)
                    and ops.wgrad_h2_supported(hs, cv.w4, 1, cv.pad)):
                return k
        return None

    def _forms(self, plan, widest=False):
        """Which activation tensors of this unit exist as planes, as both, or not at all under the plan `_plan_h2` has chosen: name ->
        form; every tensor that is not named is F32.  The one place that knows it: `_act` hands the bodies their tensors in these forms
        and the helpers pick their kernels from them.  widest: with every optional part of the plan on planes -- the tensors
        `_probe_scales` probes (a scale that is never used costs nothing)."""
        o, t = self.ops, self.t
        lean = PLANES if self.h2_lean else BOTH              # tensors whose only readers take planes are not also written as fp32
        if plan == "layer":                                  # conv, tail and weight gradient on planes
            return {"x": PLANES, "dpre": PLANES}
        if plan == "tconv":                                  # the phase conv and its weight gradient on planes
            return {"x": PLANES, "dyp": PLANES}
        if plan == "rb":
            # x and h1: the residual add of the tail sums the planes back (exactly), the LeakyReLU mask of the dgrad epilogue reads the
            # sign off plane 0.  pre2 only where conv2 and the tail are not one launch
            c2 = o["conv2"]
            one = self.fuse_h2_tail and ops.conv_h2_tail_supported(tuple(t["h1"].shape), c2.w4, c2.stride, c2.pad)
            return {"x": lean, "h1": lean, "pre2": ABSENT if one else F32, "dpre2": PLANES, "dh1": PLANES}
        # "rbws" / "rbu": the second conv, its weight gradient and dgrad run on planes.  Where the shapes qualify (x_h2, g_h2), so do the
        # convs that read the unit input -- the first conv of an RBWS with >= 16 input channels, the two sub-pixel convs of an RBU --,
        # each with its weight gradient, and the gamma'^T GEMM of the GDN backward.  What does not qualify (thin stems, small 1x1 GEMMs)
        # stays on fp32 activations.
        rbu = plan == "rbu"
        xs, hs = tuple(self.x_in.shape), tuple(t["h1"].shape)
        first, g = ((o["subpel_conv"], o["upsample"]), o["igdn"]) if rbu else ((o["conv1"],), o["gdn"])
        x_h2 = widest or (xs[-1] % 16 == 0 and all(self._conv_ok_h2(c, xs) and ops.wgrad_h2_supported(xs, c.w4, c.stride, c.pad) for c in first))
        # gamma'^T GEMM: on rdo_linear_h2 over the fp32 t where that applies (then t is not written as planes at all), else on the plane kernel
        g_h2 = widest or (self._conv_ok_h2(g, hs, dgrad=True) and not self._gdn_lin_ok(g, t["h1"]))
        # h1 (its LeakyReLU mask is read off plane 0): as fp32 too behind an fp32-input first conv, which splits it in a launch of its own
        f = {"x": BOTH if x_h2 else F32, "h1": lean if (rbu or x_h2) else BOTH, "t": BOTH if g_h2 else F32, "dc" if rbu else "dc2": PLANES}
        if rbu:
            f.update(dup=PLANES if x_h2 else F32, dsp=PLANES if x_h2 else F32)
        else:
            f["dh1"] = PLANES if x_h2 else F32
        return f

    def _fb_layer(self):
        op, t = self.ops["layer"], self.t
        x, dpre = self._act("x"), self._act("dpre")
        self._gather(x)
        if op.is_gdn:
            # a GDN / IGDN that is its own unit (sequential Minnen2018-style coders): only gamma is trained, no dx needed
            x = x.f32
            if self.fused:
                self._gdn_pool(op, x, t["norm"])                                                 # norm pool only
                self._tail_gdn(x, t["norm"], None, op.inverse, t["dy"], t["t"])
            else:
                self._conv(op, x, t["y"], epilogue=L.EPI_IGDN if op.inverse else L.EPI_GDN, aux=x, pre=t["norm"], square=True)
                self._loss(t["y"], t["dy"])
                ops.gdn_bwd_t(t["dy"], x, t["norm"], op.inverse, t["t"])
            self._wgrad(op, x, t["t"], square=True)
            return
        if op.tconv is not None and op.tc_phase is None:
            s_, q_, Hu, Wu = self.tc_geom
            x = _act_of(ops.zero_insert(x.f32, s_, q_, q_, Hu, Wu, out=t["xu"]))
        epi = op.qm.fused_epilogue() if self.include_act else None
        if epi is None and self.include_act and type(op.qm.activation_function).__name__ != "StraightThrough":
            raise NotImplementedError("calibration engine: only LeakyReLU(0.01) or ReLU may be fused into a layer unit")
        act = {None: ops.ACT_NONE, L.EPI_LRELU: ops.ACT_LRELU, L.EPI_RELU: ops.ACT_RELU}[epi]
        phase = op.tc_phase is not None                      # transposed conv without zero insertion
        if self._unit1x1_ok(op, x):                          # a 1 x 1 conv: forward, tail and weight-gradient slabs in one launch
            if op.slabs is None:
                op.slabs = self._buf(ops.unit1x1_nslab(math.prod(x.shape[:-1]), op.w4[0]), *op.w4)
            self._task_is_rec = True
            ops.unit1x1(x.f32, op.wq4(), op.bias, self.co, self.idx, self.it, 2.0, act, self.loss_log, op.slabs)
        elif self.fused and phase:
            self._tconv_forward(op, x, t["y"])                                                   # pre-activation
            self._tail_act(t["y"], None, act, t["dpre"])
            self._tconv_wgrad(op, x, t["dpre"])
        elif self.fused:
            self._conv_tail(op, x, t["y"], None, act, dpre)                                      # t["y"]: pre-activation, if it is stored
            self._wgrad(op, x, dpre)
        else:
            if phase:
                self._tconv_forward(op, x, t["y"], epilogue=L.EPI_NONE if epi is None else epi)
            else:
                self._conv(op, x, t["y"], epilogue=L.EPI_NONE if epi is None else epi)
            self._loss(t["y"], t["dy"])
            g = t["dy"]
            if epi is not None:
                (ops.lrelu_bwd if epi == L.EPI_LRELU else ops.relu_bwd)(t["dy"], t["y"], t["dpre"])
                g = t["dpre"]
            (self._tconv_wgrad if phase else self._wgrad)(op, x, g)

    def _fb_rb(self):
        o, t = self.ops, self.t
        c1, c2, skip = o["conv1"], o["conv2"], o.get("skip")
        x, h1, dpre2, dh1 = self._act("x"), self._act("h1"), self._act("dpre2"), self._act("dh1")
        self._gather(x)
        self._conv(c1, x, h1, epilogue=L.EPI_LRELU)
        res = x
        if skip is not None:
            self._conv(skip, x, t["sk"])
            res = t["sk"]
        if self.fused:
            self._conv_tail(c2, h1, self._act("pre2"), res, ops.ACT_LRELU, dpre2, gout=t["dout"] if skip is not None else None)
        else:
            self._conv(c2, h1, t["out"], epilogue=L.EPI_LRELU, residual=res, pre=t["pre2"])
            self._loss(t["out"], t["dout"])
            ops.lrelu_bwd(t["dout"], t["pre2"], t["dpre2"])
        if skip is not None:
            self._wgrad(skip, x, t["dout"])
        self._wgrad(c2, h1, dpre2)
        self._dgrad(c2, dpre2, dh1, epilogue=L.EPI_LRELU_BWD, aux=h1)
        self._split_point()
        self._wgrad(c1, x, dh1)

    def _fb_gdn_block(self):
        """RBWS (conv1 -> LeakyReLU -> conv2 -> GDN, + the input or its skip conv) and RBU (sub-pixel conv -> LeakyReLU -> conv -> IGDN,
        + the sub-pixel upsample conv of the input)."""
        o, t = self.ops, self.t
        rbu = self.kind == "rbu"
        if rbu:
            first, cv, g, side, r = o["subpel_conv"], o["conv"], o["igdn"], o["upsample"], self.r
        else:
            first, cv, g, side = o["conv1"], o["conv2"], o["gdn"], o.get("skip")
        h1, dc, tt, x = self._act("h1"), self._act("dc" if rbu else "dc2"), self._act("t"), self._act("x")
        c = t["c" if rbu else "c2"]
        # the branch beside the two convs (skip conv / upsample conv) is recorded in front of the second conv on planes, behind it on fp32
        # activations: the launches are independent and either order computes the same values; each form keeps the order its plans
        # have always had, so that the op list of a unit stays comparable from one version of this file to the next
        side_first = self.h2_plan is not None
        # norm pool, tail, gamma'^T GEMM and dx in ONE launch where both GEMMs would run on rdo_linear_h2 (same bits; norm and acc do not
        # exist).  dL/dout is written only where something reads it: the weight gradient of the side branch
        one = (self.fused and self.gdn_fused and self._gdn_lin_ok(g, c) and tt.planes is None
               and ops.gdn_fwd_bwd_supported(math.prod(c.shape[:-1]), c.shape[-1]))
        px = rbu and self._subpel_plan(one, x, h1, dc, first, side, cv)
        self._gather(x)
        if px:
            # sub-pixel convs with their rows in 4 groups: the pixel shuffle is an address change in the epilogue's stores, sp and up never
            # exist (LeakyReLU commutes with the shuffle)
            for op in (first, side):
                op.enable_planes(True, False, h2=True)
                ops.conv2d_fwd_h2_px(x.planes, x.shape, op.w4, op.wq_planes, L.STORE_SHUFFLE, op.bias_g, op.stride, op.pad,
                                     epilogue=L.EPI_LRELU if op is first else L.EPI_NONE, out=h1.f32 if op is first else t["ups"],
                                     out_planes=h1.planes if op is first else None)
            self._conv(cv, h1, c)
            res = t["ups"]
        elif rbu:
            sp, up = self._tmp("sp", t["dsp"]), self._tmp("up", t["dsp"])
            self._conv(first, x, sp, epilogue=L.EPI_LRELU)         # LeakyReLU commutes with the pixel shuffle
            if side_first:
                self._conv(side, x, up)
            self._shuffle(sp, r, h1)
            if side_first:
                self._shuffle(up, r, t["ups"])
            self._conv(cv, h1, c)
            if not side_first:
                self._conv(side, x, up)
                self._shuffle(up, r, t["ups"])
            res = t["ups"]
        else:
            self._conv(first, x, h1, epilogue=L.EPI_LRELU)         # (fp32 input: the planes of h1 by a split of their own)
            if side is not None and side_first:
                self._conv(side, x.f32, t["sk"])
            self._conv(cv, h1, c)
            if side is not None and not side_first:
                self._conv(side, x.f32, t["sk"])
            res = x if side is None else t["sk"]
        dout = self._tmp("dout", c) if (rbu and not px) else t.get("dout")
        if px:                                                        # dL/dout leaves the launch as the planes of its unshuffle
            self._task_is_rec = True
            dup = self._act("dup")
            ops.gdn_fwd_bwd_px(c, g.lin_planes(True), g.lin_planes(False), g.beta, _f32(res), self.co, self.idx, self.it, 2.0, True, self.loss_log,
                               tt.f32, dup.planes, dx=dc.f32, dx_planes=dc.planes)
        elif one:
            self._task_is_rec = True
            ops.gdn_fwd_bwd(c, g.lin_planes(True), g.lin_planes(False), g.beta, _f32(res), self.co, self.idx, self.it, 2.0, rbu, self.loss_log,
                            tt.f32, grad_out=dout if (rbu or side is not None) else None, dx=dc.f32, dx_planes=dc.planes)
        elif self.fused:
            self._gdn_pool(g, c, self._tmp("norm", c))
            self._tail_gdn(c, t["norm"], res, rbu, dout, tt)
        else:
            self._conv(g, c, t["out"], epilogue=L.EPI_IGDN if rbu else L.EPI_GDN, aux=c, residual=res, pre=self._tmp("norm", c), square=True)
            self._loss(t["out"], dout)
        if px:
            self._wgrad(side, x, dup)                                 # (slab rows in the order of dup's channels: in 4 groups)
        elif rbu:
            dup = self._act("dup")
            self._unshuffle(dout, r, dup)
            self._wgrad(side, x, dup)
        elif side is not None:
            self._wgrad(side, x.f32, dout)
        if not self.fused:                                            # the fused tail has already written t
            ops.gdn_bwd_t(dout, c, t["norm"], rbu, tt.f32)
        if not one:
            self._gdn_acc(g, tt, self._tmp("acc", c))                 # t . gamma'
            if dc.planes is not None or c.numel() % 4 == 0:
                ops.gdn_bwd_dx_h2(dout, c, t["norm"], t["acc"], rbu, dx=dc.f32, dx_planes=dc.planes)   # 16-byte accesses
            else:
                ops.gdn_bwd_dx(dout, c, t["norm"], t["acc"], rbu, dc.f32)
        self._wgrad(g, c, tt.f32, square=True)                        # dgamma'[k][i] = sum_m t_k x_i^2
        self._wgrad(cv, h1, dc)
        if px:                                                        # the dgrad's epilogue stores the unshuffle; fp32 dh1 never exists
            dsp = self._act("dsp")
            cv.enable_planes(False, True, h2=True)
            ops.conv2d_fwd_h2_px(dc.planes, dc.shape, tuple(cv.wd4().shape), cv.wd_planes, L.STORE_UNSHUFFLE, None, 1, cv.K - 1 - cv.pad,
                                 epilogue=L.EPI_LRELU_BWD, aux=h1.f32, aux_planes=_planes_only(h1), out_planes=dsp.planes)
            self._wgrad(first, x, dsp)
            return
        if rbu:
            if "dh1" not in t:
                self._tmp("dh1", c)
            dh1 = self._act("dh1")
            self._dgrad(cv, dc, dh1, epilogue=L.EPI_LRELU_BWD, aux=h1)
            dsp = self._act("dsp")
            self._unshuffle(dh1, r, dsp)
            self._split_point()
            self._wgrad(first, x, dsp)
        else:
            dh1 = self._act("dh1")
            self._dgrad(cv, dc, dh1, epilogue=L.EPI_LRELU_BWD, aux=h1)
            self._split_point()
            self._wgrad(first, x, dh1)

    def _subpel_plan(self, one, x, h1, dc, first, side, cv):
        """Does this RBU unit take the plan that has its four pixel (un)shuffles in the stores of the kernels around them -- as a whole, or
        not at all?  It does on the H2 plan with the unit input on planes and the GDN block as one launch, where the four kernels take
        the shapes (conv_h2_px_supported, gdn_fwd_bwd_px_supported) and the unit's step is the batched launch that knows rows in 4
        groups.  Not while probing, not on fp32 activations, not under data parallelism (the gradient-only launch reads the slabs in
        logical order).  Marks the two sub-pixel convs (`_Weights.row_groups`) either way: a plan is recorded from a clean slate."""
        for op in self.ops.values():
            op.row_groups, op.bias_g = 0, None
        if not (self.subpel_fused and not self._probing and self.h2_plan == "rbu" and self.r == 2 and one and not self.split and self._handover
                and x.planes is not None and h1.planes is not None and dc.planes is not None
                and self.forms.get("dup") == PLANES and self.forms.get("dsp") == PLANES):
            return False
        xs, wd4 = tuple(x.shape), tuple(cv.wd4().shape)
        if not (all(ops.conv_h2_px_supported(xs, op.w4, op.stride, op.pad, L.STORE_SHUFFLE) for op in (first, side))
                and ops.conv_h2_px_supported(tuple(dc.shape), wd4, 1, cv.K - 1 - cv.pad, L.STORE_UNSHUFFLE)
                and ops.gdn_fwd_bwd_px_supported(tuple(dc.shape))):
            return False
        for op in (first, side):
            op.row_groups = 4
            op.bias_g = None if op.bias is None else op.bias[ops.group_rows(op.rows).to(op.bias.device)].contiguous()
        return True

    def _probe_amax(self, names):
        """One eager iteration of the unit on fp32 activations and the plain fp32 kernels (no planes, no AdaRound step) at the CURRENT
        weights and iteration counter -> largest magnitude of every tensor the plan keeps as planes (CPU tensor)."""
        saved = ops.set_tuning("conv_x6", 0)
        self._probing = True
        try:
            self._forward_backward()
        finally:
            self._probing = False
            ops.set_tuning("conv_x6", saved)
        return torch.stack([(self.x_in if n == "x" else self.t[n]).abs().max() for n in names]).cpu()

    def _set_weights(self, soft):
        """soft-rounded (the state the loop runs in) or hard-rounded weights in every op's wq / wd (set-up only)"""
        for op in self.ops.values():
            op.set_weight(soft)
            if op.tc_phase is not None:
                op.expand_phase()

    def _probe_scales(self):
        """fp16 planes need a per-tensor power-of-two scale (include/rdo_ptq_hip.h, "H2 tensors"), fixed before the plan is recorded.
        TWO probe iterations bracket what the run will see: one at the initial soft weights (= the full-precision weights: the
        reconstruction error is whatever the quantised input alone causes -- nothing at all for the first unit of a model) and one at
        the HARD-rounded weights (every weight up to delta / 2 off: the error level the soft weights move towards while b decays --
        the practical upper end of the run's gradients).  The scale puts the larger of the two magnitudes at 2^7: x512 before fp16
        overflows, and fp32-chain accuracy down to 2^-2, i.e. for tensors up to 512 x smaller than probed (tools/f16_probe.hip).
        A tensor that is exactly zero in both probes gives no scale: the unit then runs on fp32 activations.  Should a run outgrow
        its scales all the same, `_recover` restarts the unit (scales from the recorded magnitudes, then fp32 activations): loud, never a lost run."""
        plan = self._plan_h2()
        if plan is None:
            return
        names = [self.PLANES_AS.get(n, n) for n, f in self._forms(plan, widest=True).items() if f & PLANES]
        amax = self._probe_amax(names)
        self._set_weights(soft=False)
        try:
            amax = torch.maximum(amax, self._probe_amax(names))
        finally:
            self._set_weights(soft=True)
        self._clear_probe()
        for n_ in self.GDN_TMP:                               # (the probe ran the GDN block as separate launches; the plan may not: `_tmp`)
            if self.kind in ("rbws", "rbu"):
                self.t.pop(n_, None)
        if self.kind == "rbu":
            for n_ in self.SUBPEL_TMP:                        # (... and the pixel (un)shuffles)
                self.t.pop(n_, None)
        if self.world > 1:
            # every rank probes its own shard: agree on the magnitudes (MAX) so that all ranks record the same scales, take the same
            # "all-zero tensor" decision below and -- after an overflow, whose words are MAX-reduced too -- re-derive the same new scales
            a = amax.to(self.dev)
            a = torch.where(torch.isfinite(a), a, torch.full_like(a, float("inf")))
            torch.distributed.all_reduce(a, op=torch.distributed.ReduceOp.MAX, group=self.group)
            amax = a.cpu()
        if not torch.isfinite(amax).all():
            raise RuntimeError("calibration engine: non-finite activations in the probe iteration")
        if bool((amax <= 0).any()):
            import logging
            logging.getLogger("rdo_ptq.engine").warning(
                "unit with an all-zero tensor in both probe iterations (%s): no fp16 plane scale can be derived, running it on fp32 activations",
                [n for n, a in zip(names, amax) if float(a) <= 0])
            self.use_h2 = False
            return
        self._amax = {n: float(a) for n, a in zip(names, amax)}
        self.scales = {n: ops.pow2_scale(a) for n, a in self._amax.items()}

    def _clear_probe(self):
        """a probe leaves no trace: logs, counters, gradient slabs (the recorded kernels may want another split count)"""
        self.loss_log.zero_(); self.task_log.zero_(); self.round_log.zero_(); self._it2.zero_()
        for op in self.ops.values():
            op.slabs = None

    # ---- fp16 range: poll, restart ------------------------------------------------------------------------------------------------
    H2_POLL = int(os.environ.get("RDO_H2_POLL", 512))        # iterations between two reads of the overflow word inside one run() call

    H2_RESTARTS = 2                                           # restarts on re-scaled planes before the unit goes to fp32 activations

    def _overflowed(self):
        """Has an H2 producer of this unit met a value outside fp16's range?  (A 64-byte read: synchronises.)  Data parallel: MAX over
        the ranks -- every rank restarts, with the same new scales, or none does."""
        if not self.P:
            return False
        v = self._ovf.clone()
        if self.world > 1:
            torch.distributed.all_reduce(v, op=torch.distributed.ReduceOp.MAX, group=self.group)
        self._ovf_seen = v.cpu().tolist()
        return any(self._ovf_seen)

    def _recover(self):
        """A value left the fp16 range of its planes: the iterations since the unit's start are invalid.  Restart the unit from its
        initial state (alpha from the weights, zero Adam moments, iteration 0: the index table and the counter-RNG masks make the
        re-run the same run).  The overflow words say what happened: a tensor's word 0 is the largest finite |x s| that did not fit
        -> its magnitude is now known exactly and its scale is re-derived from it with x8 head-room; a tensor that only met
        inf / NaN sits downstream of such an overflow and is re-scaled by the largest growth seen in the unit.  After H2_RESTARTS such
        restarts, or when nothing finite was recorded (the data themselves are not finite), the unit re-runs on fp32 activations
        (`use_h2 = False`: the split-bf16 / fp32-MFMA kernels cannot overflow).  The reference's arithmetic is plain fp32
        (quant_layer.py:123)."""
        import logging
        lg = logging.getLogger("rdo_ptq.engine")
        seen = self._ovf_seen
        self.h2_restarts += 1
        grown = {}                                            # tensor -> observed magnitude / the magnitude its scale was made for
        for name, k in self._ovf_slot.items():
            if seen[2 * k]:
                grown[name] = ops.overflow_magnitude(seen[2 * k]) / self.scales[name] / self._amax[name]
        if self.h2_restarts <= self.H2_RESTARTS and grown and not (seen[0] or seen[1]):
            r = max(grown.values())
            for name, k in self._ovf_slot.items():
                if name in grown or seen[2 * k + 1]:
                    self._amax[name] *= 8.0 * grown.get(name, r)
            self.scales = {n: ops.pow2_scale(a) for n, a in self._amax.items()}
            lg.warning("calibration unit outgrew the fp16 range of its H2 planes within %d iterations (%s): restarting it with scales %s",
                       self._done, {n: f"x{g:.3g}" for n, g in grown.items()}, self.scales)
        else:
            self.use_h2 = False
            lg.warning("calibration unit left the fp16 range of its H2 planes%s: restarting it on fp32 activations",
                       " again" if self.h2_restarts > 1 else " with non-finite values")
        for op in self.ops.values():
            op.init_alpha()
            op.m.zero_(); op.v.zero_()
            op.drop_planes()
        self._set_weights(soft=True)
        self.P, self._ovf_slot = {}, {}
        self._clear_probe()
        self._ovf.zero_()
        self._done = 0
        self._ovf_checked = -1
        self._dp_graph = self._rd_graph = None
        self._start()

    def _check_overflow(self):
        """Where results leave the engine: an overflow not yet seen by the polls of `run` is handled here.  COLLECTIVE under data
        parallelism (the MAX all-reduce of `_overflowed`), so it must only be reached at rank-invariant points: it is run once per
        position of the unit (`sync_overflow`, called by recon.py behind `run()` on every rank, and by `finish`) and the verdict is
        cached -- `logs` / `logs_terms` called afterwards, on any subset of the ranks, issue no overflow collective.
        Restart ladder (`_recover`): H2_RESTARTS restarts on re-derived scales, then one on fp32 activations (`use_h2 = False`, no
        planes left, `_overflowed` is False by construction).  An overflow word raised with no plane tensor alive would be a library
        fault."""
        self.dp_drain()
        if self._ovf_checked == self._done:
            return
        while self._overflowed():
            if not self.use_h2:
                raise RuntimeError("calibration engine: an H2 overflow word is raised on the fp32-activation path (library fault)")
            target = self._done
            with ops.h2_flag(self._ovf[0:2]):
                self._recover()
            self.run(target)
            torch.cuda.synchronize()
        self._ovf_checked = self._done

    def sync_overflow(self):
        """The rank-synchronised fp16-range verdict for the iterations run so far (see `_check_overflow`): call it on EVERY rank at the
        same point of the schedule before any rank-dependent use of `logs*()`."""
        self._check_overflow()

    def _forward_backward(self):
        """Record (or, probing, run on fp32 activations: no plan, every tensor F32) one iteration's forward and backward pass."""
        self.h2_plan = None if self._probing else self._plan_h2()
        self.forms = {} if self.h2_plan is None else self._forms(self.h2_plan)
        {"layer": self._fb_layer, "rb": self._fb_rb, "rbws": self._fb_gdn_block, "rbu": self._fb_gdn_block}[self.kind]()

    def _items(self, opl):
        # (lin_fwd / lin_bwd: the fragment-ordered planes of a Linear / GDN gamma on rdo_linear_h2 -- written by the step's own launch)
        return [dict(d=op.desc, w=op.w, delta=op.delta, zp=op.zp, slabs=op.slabs, alpha=op.alpha, m=op.m, v=op.v, wq=op.wq, wd=op.wd,
                     wq_planes=op.wq_planes, wd_planes=op.wd_planes, dalpha=op.dalpha,
                     lin_fwd=op.lin_fwd, lin_bwd=op.lin_bwd) for op in opl]

    STEP_BATCH = 8          # weight tensors per rdo_adaround_step_batch launch (kMaxBatch of adaround.hip)

    def _batchable(self, opl):
        """The tensors can go through rdo_adaround_step_batch: in ONE launch up to STEP_BATCH of them, else in ceil(n / STEP_BATCH) launches
        (an RSTB with six blocks has 37 trainable tensors: 37 single-tensor steps, 24 transposes and 48 plane splits per iteration before)."""
        return self.batch_step and len(opl) >= 1 and all(op.numel() % 4 == 0 and not op.is_mx for op in opl)

    def _step_batches(self, opl, scale, mode):
        """The batched step (mode 0) / update (mode 2) of `opl`.  The iteration counter moves by hand-over (the FIRST launch leaves
        it + 1 in the shadow word -- every launch of the step only reads the counter --, the next gather publishes it) or, with the
        hand-over switched off, with the last launch."""
        for i in range(0, len(opl), self.STEP_BATCH):
            last = i + self.STEP_BATCH >= len(opl)
            if self._folded:
                # every launch of the step reads the published word; the LAST one carries the next mini-batch and moves the real counter
                it, kw = self.it_shadow, dict(iter_shadow=self.it if last else None, gather=self._next_gather if last else None)
            elif self._handover:
                it, kw = self.it, dict(iter_shadow=self.it_shadow if i == 0 else None)
            else:
                it, kw = self.it, dict(advance_iter=self.it if last else None)
            ops.adaround_step_batch(self._items(opl[i:i + self.STEP_BATCH]), scale, self.weight, self.sched, it, self.round_log, mode=mode,
                                    row_groups=[op.row_groups for op in opl[i:i + self.STEP_BATCH]] if any(op.row_groups for op in opl) else None,
                                    **kw)

    @property
    def _handover(self):
        """The counter hand-over needs the unit's step as batched launches (it is the first of them that fills the shadow)."""
        return self.fold_iter and self._batchable(list(self.ops.values()))

    @property
    def _folded(self):
        """The step launch of iteration i assembles the mini-batch of iteration i + 1.  Counter words then: the loss / tail launch reads
        the real counter `it` and publishes it into `it_shadow` (ops.iter_bind_publish); the step reads `it_shadow` and its first thread
        stores it + 1 into `it` -- nobody reads a word that another thread of the same launch writes (include/rdo_ptq_hip.h)."""
        return self.fold_gather and self._handover and self.rd is None

    def _it_src(self):
        return self.it_shadow if (self._handover and not self._folded) else self.it

    def _it_pub(self):
        return self.it if (self._handover and not self._folded) else None

    def _gather(self, x):
        """The unit's mini-batch for the current iteration: x_q / x_fp rows mixed by the QDrop mask into `x`, as fp32 and / or planes.
        Recorded as the iteration's first kernel -- or, folded, handed to the step launch of the PREVIOUS iteration (`_step_batches`)
        with `_prime` covering iteration 0."""
        x = _act_of(x)
        g = dict(cache_q=self.cq, cache_fp=self.cf, idx_table=self.idx, B=self.B, batch_offset=self.batch_offset,
                 prob=self.input_prob, seed=self.seed, out=x.f32, out_planes=x.planes)
        if self._folded and not self._probing:
            self._next_gather = g
        else:
            self._gather_now(g, self._it_src(), self._it_pub())

    def _gather_now(self, g, it, publish=None):
        if g["out_planes"] is not None:
            ops.gather_qdrop_h2(self.cq, self.cf, self.idx, it, self.B, self.input_prob, self.seed, g["out"], g["out_planes"], self.batch_offset,
                                iter_publish=publish)
        else:
            ops.gather_qdrop(self.cq, self.cf, self.idx, it, self.B, self.input_prob, self.seed, g["out"], self.batch_offset, iter_publish=publish)

    def _prime(self):
        """Folded gather: the mini-batch of the iteration the counter stands at, assembled eagerly (before the first iteration of a
        run and after a restart; every later one comes from the previous iteration's step launch)."""
        if self._next_gather is not None:
            self.it_shadow.copy_(self.it)
            self._gather_now(self._next_gather, self.it)

    def _grad_ops(self, names):
        opl = [self.ops[n] for n in names]
        if self._batchable(opl):
            for i in range(0, len(opl), self.STEP_BATCH):
                ops.adaround_step_batch(self._items(opl[i:i + self.STEP_BATCH]), 1.0, self.weight, self.sched, self.it, self.round_log, mode=1)
            return
        for op in opl:
            ops.adaround_grad(op.desc, op.w, op.alpha, op.delta, op.zp, op.slabs, op.dalpha)

    def _step_ops(self, apply=False):
        """AdaRound step of every op of the unit + iteration counter: one batched launch (+ one for the dgrad layouts) when the
        tensors allow it, else one launch per op.  The bf16 planes of the new weights are written by the same launches -- except for
        ops on an MX grid (`_MxOp`: never batchable), whose step writes no planes: the split kernels follow it.
        apply (data parallel, plan B): the step from the all-reduced gradient bucket instead of from the weight-gradient slabs."""
        opl = list(self.ops.values())
        scale = self.bucket.scale if apply else 1.0
        if self._batchable(opl):
            self._step_batches(opl, scale, 2 if apply else 0)
            self._after_step(lin_done=True)
            return
        for op in opl:
            if apply:
                ops.adaround_apply(op.desc, op.w, op.delta, op.zp, op.dalpha, scale, self.weight, self.sched, self.it,
                                   op.alpha, op.m, op.v, op.wq, op.wd, self.round_log, op.wq_planes, op.wd_planes)
            else:
                op.step(self, scale)
        ops.iter_advance(self.it)
        self._after_step()
        for op in opl:
            if op.is_mx:                       # rdo_mx_round_step writes no planes: the split kernels refresh them
                op.split_planes(("wq_planes", "wd_planes"))

    def _next_plan(self):
        """close the plan being recorded and go on recording into a new one"""
        self._rec_ctx.__exit__(None, None, None)
        plan = Plan()
        self._rec_ctx = plan.record()
        self._rec_ctx.__enter__()
        return plan

    def _split_point(self):
        """Called by the backward pass right before its last weight-gradient kernel.  Data-parallel recording only: the gradients
        of every other op are final here -> chain them into the front of the bucket, close plan A and continue in plan A2, so
        that `run` can start the all-reduce of the front while the last wgrad computes."""
        if self._probing or self._late is None or self.plan_a2 is not None:
            return
        self._grad_ops([n for n in self.ops if n != self._late])
        self.plan_a2 = self._next_plan()

    def _record(self):
        self.plan_a = Plan()
        self.plan_a2 = self.plan_b = self.plan_rd = None
        self._rec_ctx = self.plan_a.record()
        self._rec_ctx.__enter__()
        self._next_gather = None
        try:
            if self._folded:
                ops.iter_bind_publish(self.it_shadow)          # consumed by the iteration's first loss / tail launch
            self._forward_backward()
            if self._folded and (ops.iter_bind_publish(None) or self._next_gather is None):
                raise RuntimeError("calibration engine: the folded gather needs exactly one loss / tail launch and one gather per iteration")
            if not self.split:
                self._step_ops()
            elif self.plan_a2 is not None:
                self._grad_ops([self._late])
            else:
                self._grad_ops(list(self.ops))
        finally:
            ops.iter_bind_publish(None)        # (a recording that raised must not leave its word bound for the next engine's loss launch)
            self._rec_ctx.__exit__(None, None, None)
            self._rec_ctx = None
        if self.split:
            self.plan_b = Plan()
            with self.plan_b.record():
                self._step_ops(apply=True)

    # ------------------------------------------------------------------------------------------------------------------
    def run(self, n_iters=None, idle=None):
        """Enqueue `n_iters` (default: all remaining) calibration iterations on the current stream; `idle()` (optional) is called after
        every enqueued piece, in front of the next poll -- host work that overlaps the GPU's (recon.py draws the next unit's mini-batch
        indices there).  Units on H2 planes read their
        overflow word every `H2_POLL` iterations of a long call (a 4-byte read; calls of at most H2_POLL iterations stay fully
        asynchronous, the word is then read by `logs` / `finish`) and restart themselves when it is set (`_recover`)."""
        done = self._done
        n = self.iters - done if n_iters is None else int(n_iters)
        if n < 0 or done + n > self.iters:
            raise ValueError(f"cannot run {n} iterations: {done} of {self.iters} already done")
        target = done + n
        with ops.h2_flag(self._ovf[0:2]):
            while self._done < target:
                k = target - self._done
                if self.P and self.H2_POLL > 0:
                    k = min(k, self.H2_POLL)
                if not (self.P and self.H2_POLL > 0) and idle is not None:
                    k = min(k, max(64, (target - done) // 16))      # no poll points: still enqueue in pieces so that `idle` gets its turns
                if self.plan_rd is not None:
                    self._run_rd(k)
                elif not self.split:
                    self.plan_a.run(k, graph=self.use_graph)
                else:
                    self._run_dp(k)
                self._done += k
                if idle is not None:
                    idle()                                      # host work while the GPU has the enqueued iterations to do
                if self._done < target and self.P and self.H2_POLL > 0:
                    self.dp_drain()
                if self._done < target and self._overflowed():
                    self._recover()                  # back to iteration 0 with new scales / on fp32 activations
        return n

    def prepare(self, n_iters=None):
        """Capture the graphs a `run(n_iters)` (default: the rest of the unit's iterations) will replay -- set-up work like the recording;
        `run` does it lazily otherwise (inside its first call).  Single-GPU plans only: the data-parallel and `rd` loops capture in
        their own first call (they need an eager iteration in front)."""
        if self.use_graph and not self.split and self.plan_rd is None:
            n = self.iters - self._done if n_iters is None else int(n_iters)
            k = min(n, self.H2_POLL) if (self.P and self.H2_POLL > 0) else n
            self.plan_a.prepare(k)
            if n % k:
                self.plan_a.prepare(n % k)

    def _data_terms(self):
        """(rec, task) per iteration on the device, averaged over the data-parallel ranks."""
        rec, task = self.loss_log.sum(1), self.task_log.sum(1)
        if self._task_is_rec:
            rec = rec * 0.5
            task = rec.clone()
        if self.world > 1:
            both = torch.stack([rec, task])
            torch.distributed.all_reduce(both, group=self.group)
            rec, task = both[0] / self.world, both[1] / self.world
        return rec, task

    def logs(self):
        """(total, rec+task, round) per iteration as CPU tensors (synchronises)."""
        self._check_overflow()
        rec, task = self._data_terms()
        rt = (rec + task).cpu()
        rd = self.round_log.sum(1).cpu()
        return rt + rd, rt, rd

    def logs_terms(self):
        """(rec, task, round, b) per iteration as CPU tensors: the four numbers of the reference's periodic log line
        (layer_opt.py:168-170); b is the temperature of the schedule table (0 while the rounding loss is off)."""
        self._check_overflow()
        rec, task = self._data_terms()
        return rec.cpu(), task.cpu(), self.round_log.sum(1).cpu(), self.sched[:, 0].cpu()

    def alpha_of(self, name):
        """Trained alpha in the logical weight shape (OIHW view of the OHWI storage; [Cin,Cout,KH,KW] for transposed convs)."""
        op = self.ops[name]
        if op.tconv is not None:
            return op.alpha.flip(1, 2).permute(3, 0, 1, 2)
        if op.qm.kind in ("linear", "layernorm"):
            return op.alpha.reshape(op.qm.org_weight.shape)
        return op.alpha.permute(0, 3, 1, 2) if op.alpha.dim() == 4 else op.alpha

    def finish(self):
        """Hand the trained rounding back to the modules: AdaRoundQuantizer with hard targets, `trained` flags
        (layer_opt.py:313-316 / block_opt.py:316-321).  An op on an MX grid writes alpha into the module's own `MXAdaRoundQuantizer`:
        no AdaRoundQuantizer is made for it."""
        self._check_overflow()
        for name, op in self.ops.items():
            qm = op.qm
            rows = op.alpha.flip(1, 2).contiguous() if op.tconv is not None else op.alpha
            if op.is_mx:
                # the module's MXAdaRoundQuantizer takes the rounding itself (alpha in `to_rows` layout: un-flipped for a transposed conv)
                q = qm.weight_quantizer
                q.alpha = rows.detach().clone().reshape(to_rows(qm.org_weight.data, op.tconv is not None).shape)
                q.soft_targets = False
                qm.act_quantizer.is_training = False
                qm.drop_weight_pack()
                continue
            if qm.kind == "linear":
                rows = op.alpha.reshape(op.alpha.shape[0], -1)
            if not op.channel_wise and not op.is_ln:
                # the per-tensor quantiser keeps alpha in the logical (OIHW) element order, flattened to one row
                rows = from_rows(rows, qm.org_weight.data, op.tconv is not None).contiguous().reshape(1, -1)
            ada = AdaRoundQuantizer(uaq=qm.weight_quantizer, round_mode="learned_hard_sigmoid",
                                    weight_tensor=qm.org_weight.data, alpha_rows=rows)
            ada.soft_targets = False
            qm.weight_quantizer = ada
            qm.act_quantizer.is_training = False
            qm.drop_weight_pack()              # packs of the pre-calibration weights (nearest rounding) are stale from here on
        if self.rd is not None:
            self.rd.pop("memo", None)          # per-image outputs of the unit-independent modules (up to RD_CACHE_LIMIT bytes)
