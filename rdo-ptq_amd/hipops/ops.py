"""Thin tensor-level wrappers over the C ABI (include/rdo_ptq_hip.h).

Conventions: every tensor is a contiguous fp32 CUDA tensor; activations are NHWC `[B,H,W,C]`, conv weights OHWI
`[Cout,KH,KW,Cin]` (the memory image of torch's channels_last OIHW weight).  Calls are enqueued on torch's current stream.
When a plan is being recorded (hipops.plan.Plan.record()), the same calls are captured instead of launched.
A wrapper that checks its arguments does so with the functions of `_args` (one tensor check, one whole-number check), and every check
runs before a pointer is taken (`_ptr`, `_ptr64`) or a library call made.  Workspaces a wrapper keeps between calls come from
`_workspace`; the convolutions' split-K scratch has its own rule (`_scratch`)."""
import contextlib
import ctypes as C
import math
import threading

import torch

from . import _args as A
from . import _lib as L


class H2:
    """Planes of an H2 tensor (include/rdo_ptq_hip.h): `.t` int16 [2, ...] holding fp16 bit patterns -- the two-way split of the values
    times `.scale` (a power of two) -- for activations in slice-major order [2, C/16, pixels, 16], for conv weights in fragment order."""
    __slots__ = ("t", "scale", "flag")

    def __init__(self, t, scale, flag=None):
        self.t, self.scale = t, float(scale)
        self.flag = flag          # this tensor's own overflow words (2-element int32 device tensor; see h2_flag) or None: the bound default
        m, e = math.frexp(self.scale)
        if not (self.scale > 0 and m == 0.5):
            raise ValueError(f"H2 scale must be a positive power of two, got {scale}")

    @property
    def device(self):
        return self.t.device


def _ptr(t, dtypes=(torch.float32, torch.int32, torch.int16), names="fp32/int32"):
    if t is None:
        return None
    if isinstance(t, H2):
        t = t.t
    if not t.is_cuda:
        raise RuntimeError(f"librdoptq_hip has no CPU path: tensor is on {t.device}")
    if t.dtype not in dtypes or not t.is_contiguous():
        raise RuntimeError(f"librdoptq_hip needs contiguous {names} tensors, got {t.dtype} contiguous={t.is_contiguous()}")
    return C.c_void_p(t.data_ptr())


def _ptr64(t):
    """`_ptr` for the float64 operands: tap sums, bias shifts, scan errors and scores"""
    return _ptr(t, (torch.float64,), "float64")


def _pscale(planes):
    """plane scale argument of the AdaRound entries: 0 = bf16 three-way planes (or none), > 0 = fp16 two-way planes of w * scale"""
    return planes.scale if isinstance(planes, H2) else 0.0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def conv_desc(x_shape, w_shape, stride, pad, epilogue=L.EPI_NONE, square_input=False, add_residual=False):
    B, H, W, Cin = x_shape
    Cout, KH, KW, Cin2 = w_shape
    if Cin != Cin2:
        raise ValueError(f"conv: input has {Cin} channels, weight expects {Cin2}")
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    return L.ConvDesc(B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, epilogue, int(square_input), int(add_residual))


_SCRATCH = {}       # device -> list of scratch tensors (kept alive: recorded plans hold raw pointers into them)


def _scratch(device, n_floats):
    """Split-K workspace shared by all convolutions of a device (launches are stream-ordered, so one buffer suffices)."""
    pool = _SCRATCH.setdefault(device, [])
    if not pool or pool[-1].numel() < n_floats:
        pool.append(torch.empty(max(n_floats, 1 << 22), device=device, dtype=torch.float32))
    return pool[-1]


_WORKSPACE = {}     # (op, device, *key) -> the workspace a wrapper keeps between its calls


def _workspace(op, device, need, dtype=torch.float32, *key):
    """Workspace of wrapper `op` on `device` (one without an index is the current one) for `key`: at least `need` elements of `dtype`,
    made or replaced by a larger one when there is none that large.  Launches are stream-ordered, so one buffer per key suffices.  Not
    for a wrapper that a plan records: a replaced buffer is let go (`_scratch` keeps its ones)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    ws = _WORKSPACE.get((op, device) + key)
    if ws is None or ws.numel() < need:
        ws = _WORKSPACE[(op, device) + key] = torch.empty(need, device=device, dtype=dtype)
    return ws


def _workspaces(op):
    """the live workspaces of wrapper `op` (for the tests that poison them between two launches)"""
    return [ws for k, ws in _WORKSPACE.items() if k[0] == op]


def uses_bf16x6(x_shape, w_shape, stride, pad):
    d = conv_desc(x_shape, w_shape, stride, pad)
    return bool(L.lib().rdo_conv2d_fwd_uses_bf16x6(C.byref(d)))


def split_bf16x3(w, planes=None):
    """Conv weight in kernel layout [Cout,KH,KW,Cin] (or [C,C] = 1x1) -> int16 tensor of 3 * w.numel() bf16 values: the exact
    split w = p0 + p1 + p2, each plane in the fragment order the bf16x6 kernels read ([Cin/16][KH][KW][Cout][16])."""
    if w.dim() == 2:
        w = w.reshape(w.shape[0], 1, 1, w.shape[1])
    if w.dim() != 4:
        raise ValueError("split_bf16x3: expected a conv weight [Cout,KH,KW,Cin]")
    planes = torch.empty((3,) + tuple(w.shape), device=w.device, dtype=torch.int16) if planes is None else planes
    co, kh, kw, ci = w.shape
    L.check(L.lib().rdo_split_bf16x3_conv(_ptr(w), co, kh, kw, ci, _ptr(planes), _stream()), "rdo_split_bf16x3_conv")
    return planes


def split_bf16x3_linear(w, planes=None):
    """Element order kept: planes[p].view_as(w) is plane p (generic helper, not a conv operand)."""
    planes = torch.empty((3,) + tuple(w.shape), device=w.device, dtype=torch.int16) if planes is None else planes
    L.check(L.lib().rdo_split_bf16x3(_ptr(w), w.numel(), _ptr(planes), _stream()), "rdo_split_bf16x3")
    return planes


def conv2d_fwd(x, w, bias=None, stride=1, pad=0, epilogue=L.EPI_NONE, aux=None, residual=None, square_input=False,
               out=None, pre=None, wplanes=None):
    d = conv_desc(x.shape, w.shape, stride, pad, epilogue, square_input, residual is not None)
    if out is None:
        out = torch.empty((d.B, d.Ho, d.Wo, d.Cout), device=x.device, dtype=torch.float32)
    need = int(L.lib().rdo_conv2d_fwd_workspace(C.byref(d)))
    ws = _scratch(x.device, need) if need else None
    L.check(L.lib().rdo_conv2d_fwd(C.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(aux), _ptr(residual), _ptr(out), _ptr(pre),
                                   _ptr(ws), ws.numel() if ws is not None else 0, _ptr(wplanes), _stream()), "rdo_conv2d_fwd")
    return out


SCRATCH_FLOATS = 1 << 22     # smallest split-K workspace _scratch hands out


def conv_fwd_ksplit(x_shape, w_shape, stride, pad, has_planes, device):
    """Split factor conv2d_fwd uses for this shape with the workspace it would get (1: no split-K pass)."""
    d = conv_desc(x_shape, w_shape, stride, pad)
    need = int(L.lib().rdo_conv2d_fwd_workspace(C.byref(d)))
    return int(L.lib().rdo_conv2d_fwd_ksplit(C.byref(d), int(bool(has_planes)), max(need, SCRATCH_FLOATS))), need


def conv2d_fwd_partials(x, w, stride=1, pad=0, wplanes=None):
    """K-split accumulation only: returns (workspace tensor holding [ksplit][M][Cout] partial sums, ksplit).  The workspace is the
    shared split-K scratch of the device: consume it with the next launch (loss_act_bwd_splitk)."""
    d = conv_desc(x.shape, w.shape, stride, pad)
    ks, need = conv_fwd_ksplit(tuple(x.shape), tuple(w.shape), stride, pad, wplanes is not None, x.device)
    ws = _scratch(x.device, need)
    L.check(L.lib().rdo_conv2d_fwd_partials(C.byref(d), _ptr(x), _ptr(w), _ptr(wplanes), _ptr(ws), ws.numel(), _stream()),
            "rdo_conv2d_fwd_partials")
    return ws, ks


def loss_act_bwd_splitk(partial, ksplit, bias, out_shape, residual, tgt_cache, idx_table, iter_ptr, coef, act, loss_log, out=None, grad_out=None,
                        dpre=None):
    B = out_shape[0]
    per_image = 1
    for v in out_shape[1:]:
        per_image *= int(v)
    L.check(L.lib().rdo_loss_act_bwd_splitk(_ptr(partial), int(ksplit), _ptr(bias), _ptr(residual), _ptr(tgt_cache), _ptr(idx_table),
                                            _ptr(iter_ptr), B, per_image, int(out_shape[-1]), coef, int(act), _ptr(out), _ptr(grad_out),
                                            _ptr(dpre), _ptr(loss_log), _stream()), "rdo_loss_act_bwd_splitk")


def wgrad_nsplit(x_shape, w_shape, stride, pad):
    d = conv_desc(x_shape, w_shape, stride, pad)
    return int(L.lib().rdo_conv2d_wgrad_nsplit(C.byref(d)))


def wgrad_uses_bf16x6(x_shape, w_shape, stride, pad):
    d = conv_desc(x_shape, w_shape, stride, pad)
    return bool(L.lib().rdo_conv2d_wgrad_uses_bf16x6(C.byref(d)))


@contextlib.contextmanager
def forced_wgrad(big=-1, nsplit=-1):
    """Inside the block rdo_conv2d_wgrad and its predicates (wgrad_nsplit, wgrad_uses_bf16x6) take the given tile (0: 64 x 64, 1: 192 x 192;
    this also switches the thin-Cout kernel off) and / or slab count instead of their own choice; -1 leaves a choice to the library.
    Process-wide (rdo_debug_force_wgrad_choice): a tuning and test hook, restored to (-1, -1) on exit."""
    L.lib().rdo_debug_force_wgrad_choice(int(big), int(nsplit))
    try:
        yield
    finally:
        L.lib().rdo_debug_force_wgrad_choice(-1, -1)


def conv2d_wgrad(x, dy, w_shape, stride=1, pad=0, square_input=False, slabs=None):
    d = conv_desc(x.shape, w_shape, stride, pad, square_input=square_input)
    ns = int(L.lib().rdo_conv2d_wgrad_nsplit(C.byref(d))) if slabs is None else slabs.shape[0]
    if slabs is None:
        slabs = torch.empty((ns,) + tuple(w_shape), device=x.device, dtype=torch.float32)
    L.check(L.lib().rdo_conv2d_wgrad(C.byref(d), _ptr(x), _ptr(dy), _ptr(slabs), ns, _stream()), "rdo_conv2d_wgrad")
    return slabs


def reduce_slabs(slabs, out=None):
    ns = slabs.shape[0]
    numel = slabs[0].numel()
    if out is None:
        out = torch.empty(slabs.shape[1:], device=slabs.device, dtype=torch.float32)
    L.check(L.lib().rdo_reduce_slabs(_ptr(slabs), ns, numel, _ptr(out), _stream()), "rdo_reduce_slabs")
    return out


def ada_desc(w, n_levels=256, reparam=None, conv_layout=True):
    """w: OHWI conv weight [Cout,KH,KW,Cin] or a GDN gamma [C,C]."""
    if w.dim() == 4:
        rows, KH, KW, Cin = w.shape
    else:
        rows, Cin = w.shape
        KH = KW = 1
    if not conv_layout:
        KH = KW = Cin = 0
    bound, ped = (reparam if reparam is not None else (0.0, 0.0))
    return L.AdaDesc(w.numel(), rows, n_levels, int(reparam is not None), bound, ped, KH, KW, Cin)


def adaround_init_alpha(d, w, delta, alpha=None):
    alpha = torch.empty_like(w) if alpha is None else alpha
    L.check(L.lib().rdo_adaround_init_alpha(C.byref(d), _ptr(w), _ptr(delta), _ptr(alpha), _stream()), "rdo_adaround_init_alpha")
    return alpha


def adaround_fwd(d, w, alpha, delta, zp, soft, wq=None, wd=None):
    wq = torch.empty_like(w) if wq is None else wq
    L.check(L.lib().rdo_adaround_fwd(C.byref(d), _ptr(w), _ptr(alpha), _ptr(delta), _ptr(zp), int(soft), _ptr(wq), _ptr(wd),
                                     _stream()), "rdo_adaround_fwd")
    return wq


def uaq_fakequant(d, w, delta, zp, wq=None, wd=None):
    wq = torch.empty_like(w) if wq is None else wq
    L.check(L.lib().rdo_uaq_fakequant(C.byref(d), _ptr(w), _ptr(delta), _ptr(zp), _ptr(wq), _ptr(wd), _stream()),
            "rdo_uaq_fakequant")
    return wq


def uaq_init_minmax(w, n_levels):
    rows = w.shape[0]
    delta = torch.empty(rows, device=w.device, dtype=torch.float32)
    zp = torch.empty_like(delta)
    L.check(L.lib().rdo_uaq_init_minmax(_ptr(w), rows, w.numel() // rows, n_levels, _ptr(delta), _ptr(zp), _stream()),
            "rdo_uaq_init_minmax")
    return delta, zp


def adaround_step(d, w, delta, zp, slabs, grad_scale, round_weight, sched, iter_ptr, alpha, m, v, wq, wd, round_log,
                  wq_planes=None, wd_planes=None):
    """`wq_planes` / `wd_planes`: optional planes of the new weights in fragment order -- an int16 [3, numel] tensor receives the bf16
    three-way split, an `H2` object the fp16 two-way split of w * scale."""
    _bind_out(None)            # weight planes raise the enclosing block's word
    L.check(L.lib().rdo_adaround_step(C.byref(d), _ptr(w), _ptr(delta), _ptr(zp), _ptr(slabs), slabs.shape[0], grad_scale,
                                      round_weight, _ptr(sched), _ptr(iter_ptr), _ptr(alpha), _ptr(m), _ptr(v), _ptr(wq),
                                      _ptr(wd), _ptr(round_log), _ptr(wq_planes), _ptr(wd_planes), _pscale(wq_planes), _pscale(wd_planes),
                                      _stream()), "rdo_adaround_step")


def unit1x1_supported(M, K, N):
    return bool(L.lib().rdo_unit1x1_supported(int(M), int(K), int(N)))


def unit1x1_nslab(M, N):
    return int(L.lib().rdo_unit1x1_nslab(int(M), int(N)))


def unit1x1_form(form):
    """1: split-fp16 form of rdo_unit1x1 where Cout is a multiple of 96 (default); 0: always the exact fp32 form.  -> previous setting."""
    return int(L.lib().rdo_unit1x1_form(int(form)))


def unit1x1(x, w, bias, tgt_cache, idx_table, iter_ptr, coef, act, loss_log, slabs):
    """One launch for a 1 x 1 layer unit's data path (include/rdo_ptq_hip.h: rdo_unit1x1): x [B, H, W, K] mini-batch, w [N, 1, 1, K] soft
    weights -> loss into `loss_log`, weight-gradient slabs [nslab, N, 1, 1, K]."""
    K, N = int(x.shape[-1]), int(w.shape[0])
    M = x.numel() // K
    L.check(L.lib().rdo_unit1x1(_ptr(x), M, K, N, _ptr(w), _ptr(bias), _ptr(tgt_cache), _ptr(idx_table), _ptr(iter_ptr), int(x.shape[0]),
                                float(coef), int(act), _ptr(slabs), int(slabs.shape[0]), _ptr(loss_log), _stream()), "rdo_unit1x1")


def iter_bind_publish(word):
    """The next loss / tail launch of this thread leaves the iteration number it read in `word` (a one-element int32 tensor; None clears).
    Returns True when an earlier binding was still pending (include/rdo_ptq_hip.h: rdo_iter_bind_publish)."""
    return bool(L.lib().rdo_iter_bind_publish(_ptr(word)))


def adaround_step_batch(items, grad_scale, round_weight, sched, iter_ptr, round_log, advance_iter=None, mode=0, iter_shadow=None, gather=None,
                        row_groups=None):
    """items: list of dicts(d, w, delta, zp, slabs, alpha, m, v, wq, wd, wq_planes, wd_planes[, dalpha, lin_fwd, lin_bwd]) -- one launch for every
    weight tensor of a unit (<= 8, numel % 4 == 0): mode 0 the fused AdaRound step, 1 the data gradient into `dalpha`, 2 the update
    from an (all-reduced) `dalpha`; `advance_iter`: the device iteration counter to increment afterwards.
    `gather`: dict(cache_q, cache_fp, idx_table, B, batch_offset, prob, seed, out, out_planes) -- the launch also assembles the NEXT
    iteration's mini-batch (rdo_adaround_step_batch_gather).
    `row_groups` (None: the plain entries): one 0 or 4 per item -- 4: the item's slabs are read and its forward planes written with the rows in 4 groups
    (rdo_adaround_step_batch_gather_px, include/rdo_ptq_subpel.h; with or without a gather, not with advance_iter)."""
    _bind_out(None)            # weight planes raise the enclosing block's word
    arr = (L.AdaStepItem * len(items))()
    dp = lambda t: None if t is None else _ptr(t).value
    for k, it in enumerate(items):
        a = arr[k]
        a.d = it["d"]
        a.w, a.delta, a.zp, a.slabs = dp(it["w"]), dp(it["delta"]), dp(it["zp"]), dp(it["slabs"])
        a.nsplit = it["slabs"].shape[0] if it.get("slabs") is not None else 0
        a.alpha, a.adam_m, a.adam_v, a.wq, a.wd = dp(it["alpha"]), dp(it["m"]), dp(it["v"]), dp(it["wq"]), dp(it.get("wd"))
        a.wq_planes, a.wd_planes = dp(it.get("wq_planes")), dp(it.get("wd_planes"))
        a.wq_plane_scale, a.wd_plane_scale = _pscale(it.get("wq_planes")), _pscale(it.get("wd_planes"))
        a.dalpha = dp(it.get("dalpha"))
        lf, lb = it.get("lin_fwd"), it.get("lin_bwd")      # H2 planes in rdo_linear_h2's fragment order, written by the step itself
        a.lin_fwd_planes, a.lin_bwd_planes = dp(lf), dp(lb)
        a.lin_plane_scale = float((lf if lf is not None else lb).scale) if (lf is not None or lb is not None) else 0.0
    px = row_groups is not None
    if px and (advance_iter is not None or len(row_groups) != len(items)):
        raise ValueError("adaround_step_batch: row_groups needs one entry per item and moves the counter by hand-over (iter_shadow), not advance_iter")
    if px and gather is None:
        rg = (C.c_int32 * len(items))(*[int(v) for v in row_groups])
        L.check(L.lib().rdo_adaround_step_batch_gather_px(arr, len(items), int(mode), grad_scale, round_weight, _ptr(sched), _ptr(iter_ptr),
                                                          _ptr(round_log), _ptr(iter_shadow), None, rg, _stream()),
                "rdo_adaround_step_batch_gather_px")
        return
    if gather is not None:
        if advance_iter is not None:
            raise ValueError("adaround_step_batch: the gather form moves the counter by hand-over (iter_shadow), not advance_iter")
        cq, pl = gather["cache_q"], gather.get("out_planes")
        g = L.GatherDesc()
        g.cache_q, g.cache_fp, g.idx_table = dp(cq), dp(gather["cache_fp"]), dp(gather["idx_table"])
        g.n_iters, g.B, g.batch_offset = int(gather["idx_table"].shape[0]), int(gather["B"]), int(gather.get("batch_offset", 0))
        g.per_image, g.C, g.prob, g.seed = cq[0].numel(), int(cq.shape[-1]), float(gather["prob"]), int(gather["seed"])
        g.out, g.out_planes, g.out_scale = dp(gather.get("out")), dp(pl), (float(pl.scale) if pl is not None else 0.0)
        g.overflow_flag = dp(getattr(pl, "flag", None))      # the gathered planes raise their own overflow word
        if px:
            rg = (C.c_int32 * len(items))(*[int(v) for v in row_groups])
            L.check(L.lib().rdo_adaround_step_batch_gather_px(arr, len(items), int(mode), grad_scale, round_weight, _ptr(sched), _ptr(iter_ptr),
                                                              _ptr(round_log), _ptr(iter_shadow), C.byref(g), rg, _stream()),
                    "rdo_adaround_step_batch_gather_px")
            return
        L.check(L.lib().rdo_adaround_step_batch_gather(arr, len(items), int(mode), grad_scale, round_weight, _ptr(sched), _ptr(iter_ptr),
                                                       _ptr(round_log), _ptr(iter_shadow), C.byref(g), _stream()), "rdo_adaround_step_batch_gather")
        return
    L.check(L.lib().rdo_adaround_step_batch(arr, len(items), int(mode), grad_scale, round_weight, _ptr(sched), _ptr(iter_ptr), _ptr(round_log),
                                            _ptr(advance_iter), _ptr(iter_shadow), _stream()), "rdo_adaround_step_batch")


def adaround_grad(d, w, alpha, delta, zp, slabs, dalpha):
    L.check(L.lib().rdo_adaround_grad(C.byref(d), _ptr(w), _ptr(alpha), _ptr(delta), _ptr(zp), _ptr(slabs), slabs.shape[0],
                                      _ptr(dalpha), _stream()), "rdo_adaround_grad")


def adaround_apply(d, w, delta, zp, dalpha, grad_scale, round_weight, sched, iter_ptr, alpha, m, v, wq, wd, round_log,
                   wq_planes=None, wd_planes=None):
    _bind_out(None)            # weight planes raise the enclosing block's word
    L.check(L.lib().rdo_adaround_apply(C.byref(d), _ptr(w), _ptr(delta), _ptr(zp), _ptr(dalpha), grad_scale, round_weight,
                                       _ptr(sched), _ptr(iter_ptr), _ptr(alpha), _ptr(m), _ptr(v), _ptr(wq), _ptr(wd),
                                       _ptr(round_log), _ptr(wq_planes), _ptr(wd_planes), _pscale(wq_planes), _pscale(wd_planes), _stream()),
            "rdo_adaround_apply")


def set_tuning(key, value):
    """Process-wide kernel-variant switch (include/rdo_ptq_hip.h: rdo_set_tuning); returns the previous value."""
    prev = int(L.lib().rdo_get_tuning(key.encode()))
    L.check(L.lib().rdo_set_tuning(key.encode(), int(value)), f"rdo_set_tuning({key})")
    return prev


def actquant_workspace(channels):
    """floats `actquant_perchannel` needs in `ws`; the call leaves the tensor's min[C] | max[C] in the first 2 C of them"""
    return int(L.lib().rdo_actquant_workspace(int(channels)))


def actquant_perchannel(x, out=None, ws=None, n_bits=8):
    """x: [..., C] channels-last; per-channel dynamic quant-dequant (8 bit = the reference's hard-wired width)."""
    Cc = x.shape[-1]
    npix = x.numel() // Cc
    out = torch.empty_like(x) if out is None else out
    need = int(L.lib().rdo_actquant_workspace(Cc))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=x.device, dtype=torch.float32)
    L.check(L.lib().rdo_actquant_perchannel(_ptr(x), npix, Cc, int(n_bits), _ptr(out), _ptr(ws), _stream()), "rdo_actquant_perchannel")
    return out


ACT_SEARCH_CANDIDATES = 10        # kAqsCand of csrc/actquant.hip: range * (1 - 0.05 k), k = 0..9


def _act_range_check(x, rng, what):
    Cc = x.shape[-1]
    if rng.numel() != 2 * Cc:
        raise ValueError(f"{what}: the range holds {rng.numel() // 2} channels, the tensor has {Cc}")
    return Cc, x.numel() // Cc


def act_range_init(channels, device):
    """Empty running range lo | hi = +inf | -inf of `channels` channels."""
    r = torch.empty(2 * int(channels), device=device, dtype=torch.float32)
    r[:channels] = float("inf")
    r[channels:] = float("-inf")
    return r


def actquant_observe(x, rng, out=None, n_bits=8):
    """The dynamic quantiser on x [..., C], whose per-channel min | max is then merged into the running range `rng` [2C] (in place):
    the activation is read by the dynamic kernels only."""
    Cc, npix = _act_range_check(x, rng, "actquant_observe")
    ws = torch.empty(int(L.lib().rdo_actquant_workspace(Cc)), device=x.device, dtype=torch.float32)
    out = actquant_perchannel(x, out=out, ws=ws, n_bits=n_bits)
    L.check(L.lib().rdo_actquant_observe(_ptr(ws), Cc, _ptr(rng), _stream()), "rdo_actquant_observe")
    return out


def actquant_static(x, rng, out=None, n_bits=8):
    """x: [..., C] channels-last; quant-dequant on the frozen per-channel grid rng = lo[C] | hi[C] (one launch; out may be x)."""
    Cc, npix = _act_range_check(x, rng, "actquant_static")
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().rdo_actquant_static(_ptr(x), npix, Cc, int(n_bits), _ptr(rng), _ptr(out), _stream()), "rdo_actquant_static")
    return out


def actquant_search(x, rng, err, n_bits=8, ws=None):
    """err [C, 10] += per-channel squared error of x [..., C] on the ten shrunk grids rng * (1 - 0.05 k)."""
    Cc, npix = _act_range_check(x, rng, "actquant_search")
    if tuple(err.shape) != (Cc, ACT_SEARCH_CANDIDATES):
        raise ValueError(f"actquant_search: err must be [{Cc}, {ACT_SEARCH_CANDIDATES}], got {tuple(err.shape)}")
    need = int(L.lib().rdo_actquant_search_workspace(Cc))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=x.device, dtype=torch.float32)
    L.check(L.lib().rdo_actquant_search(_ptr(x), npix, Cc, int(n_bits), _ptr(rng), _ptr(err), _ptr(ws), _stream()), "rdo_actquant_search")
    return err


ACT_SCORE_MAX = 4                 # RDO_ACT_SCORE_MAX of include/rdo_ptq_hip.h: grids scored in one read of the tensor


def actquant_score(x, cand, err, clip=None, energy=None, n_bits=8, ws=None):
    """The measured squared error of K grids on x [..., C]: cand [K, 2C] = rows lo_k | hi_k; err [C, K] += sum (x - Q_k(x))^2 with Q_k the
    expression of `actquant_static` on row k; clip [C, K, 2] (int32) += the counts of x < lo_k | x > hi_k; energy [C] += sum x^2.  `clip`
    and `energy` may be None (err is the same bits).  Everything is checked on the host before the call."""
    what = "actquant_score"
    A.tensor(what, "x", x, contiguous=True)
    if x.dim() < 1:
        raise ValueError(f"{what}: x must be [..., C], got a scalar")
    Cc = x.shape[-1]
    if not torch.is_tensor(cand) or cand.dim() != 2 or not 1 <= cand.shape[0] <= ACT_SCORE_MAX:      # (K is read off cand: its own check)
        raise ValueError(f"{what}: cand must be [K, 2C] with K in 1..{ACT_SCORE_MAX}, got "
                         f"{tuple(cand.shape) if torch.is_tensor(cand) else type(cand).__name__}")
    K = int(cand.shape[0])
    A.tensor(what, "cand", cand, shape=(K, 2 * Cc), contiguous=True, oneshot=True)
    A.tensor(what, "err", err, shape=(Cc, K), contiguous=True, oneshot=True)
    A.tensor(what, "clip", clip, torch.int32, "int32", shape=(Cc, K, 2), contiguous=True, optional=True, oneshot=True)
    A.tensor(what, "energy", energy, shape=(Cc,), contiguous=True, optional=True, oneshot=True)
    n_bits = A.whole(what, "n_bits", n_bits, 2, 16)
    need = int(L.lib().rdo_actquant_score_workspace(Cc, K))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=x.device, dtype=torch.float32)
    L.check(L.lib().rdo_actquant_score(_ptr(x), x.numel() // Cc, Cc, n_bits, _ptr(cand), K, _ptr(err), _ptr(clip), _ptr(energy), _ptr(ws),
                                       _stream()), "rdo_actquant_score")
    return err


def pair_moments(a, b, out=None):
    """Per-channel moments of two tensors of the same channels-last storage [..., C]: with d = a - b formed in fp32, -> float32 [3, C] =
    sum d | sum d^2 | sum a^2 over the pixels, in one read of both (a fixed summation order: the same input gives the same bits).  `out`:
    a contiguous fp32 [3, C] on the operands' device that is ADDED TO; None makes a zero one.  Everything is checked on the host before
    a pointer is taken."""
    what = "pair_moments"
    for name, t in (("a", a), ("b", b)):
        A.tensor(what, name, t, nonempty=False)
    if a.shape != b.shape:
        raise ValueError(f"{what}: a is {tuple(a.shape)}, b is {tuple(b.shape)}: the shapes differ")
    if a.dim() < 1 or a.numel() == 0:
        raise ValueError(f"{what}: the operands are empty or scalars: {tuple(a.shape)}")
    for name, t in (("a", a), ("b", b)):
        A.tensor(what, name, t, contiguous=True)
    A.tensor(what, "a", a, device=b.device, other="b")
    Cc = int(a.shape[-1])
    A.tensor(what, "out", out, shape=(3, Cc), contiguous=True, device=a.device, optional=True, oneshot=True)
    if not a.is_cuda:
        raise ValueError(f"{what}: the operands are on {a.device}; there is no CPU path")
    if out is None:
        out = torch.zeros(3, Cc, device=a.device, dtype=torch.float32)
    ws = _workspace(what, a.device, int(L.lib().rdo_pair_moments_workspace(Cc)), torch.float32, Cc)
    L.check(L.lib().rdo_pair_moments(_ptr(a), _ptr(b), a.numel() // Cc, Cc, _ptr(out), _ptr(ws), _stream()), "rdo_pair_moments")
    return out


TAP_MAX_SEGMENTS = 48    # kTapMaxSegs of csrc/bias_correct.hip: index runs per axis the kernel arguments hold


def tap_out_size(n, k, stride, pad, transposed=False, output_padding=0):
    """Output size of one axis of `n` inputs: the conv's, or the transposed conv's with `output_padding`."""
    if transposed:
        return (n - 1) * stride - 2 * pad + k + output_padding
    return (n + 2 * pad - k) // stride + 1


def tap_sums(x, k, stride, pad, out_hw, transposed=False, out=None):
    """Tap sums of a layer input (rdo_tap_sums, include/rdo_ptq_bias.h): x channels-last [N, H, W, C] fp32 -> float32 [k * k, C], entry
    (kh * k + kw, c) = the sum of x[:, h, w, c] over the pixels that tap (kh, kw) of a k x k convolution (stride, pad; `transposed`: of a
    transposed convolution) with `out_hw` = (Ho, Wo) outputs reads.  For k = 1 (a Linear layer; stride 1, pad 0) x may be of any rank >=
    2, every leading dimension counted as pixels, and out_hw may be None.  `out`: a contiguous fp32 [k * k, C] on x's device that is
    ADDED TO; None makes a zero one.  One read of x in a fixed summation order: the same input gives the same bits.  Everything is
    checked on the host before a pointer is taken."""
    what = "tap_sums"
    A.tensor(what, "x", x, nonempty=False)
    k = A.whole(what, "k", k, 1)
    if k > L.TAP_MAX_K:
        raise ValueError(f"{what}: k = {k}, at most {L.TAP_MAX_K} is supported")
    stride, pad = A.whole(what, "stride", stride, 1), A.whole(what, "pad", pad, 0)
    if not isinstance(transposed, bool):
        raise ValueError(f"{what}: transposed must be True or False, got {transposed!r}")
    if x.dim() != 4 and not (k == 1 and x.dim() >= 2):
        raise ValueError(f"{what}: x must be channels-last of rank 4 [N, H, W, C] (any rank >= 2 for k = 1), got rank {x.dim()}")
    A.tensor(what, "x", x, contiguous=True)
    Cc = int(x.shape[-1])
    if x.dim() == 4:
        N, H, W = (int(v) for v in x.shape[:3])
    else:
        N, H, W = 1, 1, x.numel() // Cc
    if x.dim() != 4 or (k == 1 and out_hw is None):
        if stride != 1 or pad != 0 or transposed:
            raise ValueError(f"{what}: a token tensor takes k = 1, stride 1, pad 0, not transposed")
        if x.dim() != 4 and out_hw is not None:
            raise ValueError(f"{what}: out_hw must be None for a token tensor of rank {x.dim()}")
        out_hw = (H, W)
    pair = "a pair of positive whole numbers (Ho, Wo)"
    if not isinstance(out_hw, (tuple, list)) or len(out_hw) != 2:
        raise ValueError(f"{what}: out_hw must be {pair}, got {out_hw!r}")
    Ho, Wo = (A.whole(what, "out_hw", v, 1, want=pair) for v in out_hw)
    for name, n_in, n_out in (("Ho", H, Ho), ("Wo", W, Wo)):
        if transposed:
            lo = (n_in - 1) * stride - 2 * pad + k
            if not lo <= n_out < lo + stride:
                raise ValueError(f"{what}: geometry: a transposed conv of {n_in} inputs (k {k}, stride {stride}, pad {pad}) gives {lo} .. "
                                 f"{lo + stride - 1} outputs, {name} = {n_out}")
        elif n_in + 2 * pad - k < 0 or n_out != (n_in + 2 * pad - k) // stride + 1:
            raise ValueError(f"{what}: geometry: a conv of {n_in} inputs (k {k}, stride {stride}, pad {pad}) does not give {name} = {n_out}")
    if N * H * W > 0x7fffffff:
        raise ValueError(f"{what}: geometry: {N * H * W} pixels are beyond 32-bit pixel indices")
    if max(k * k, 4 * k + 4) * Cc > 0x7fffffff:
        raise ValueError(f"{what}: geometry: {Cc} channels are too many for 32-bit entry indices")
    if transposed and 2 * (-(-pad // stride)) > TAP_MAX_SEGMENTS:
        # (a conv has at most 2 (k - 1) border indices, and no axis more than 4 k + 4 distinct tap masks: only this one can happen)
        raise ValueError(f"{what}: geometry: pad {pad} at stride {stride} leaves more than {TAP_MAX_SEGMENTS} border indices on an axis")
    A.tensor(what, "out", out, shape=(k * k, Cc), contiguous=True, device=x.device, optional=True, oneshot=True)
    if not x.is_cuda:
        raise ValueError(f"{what}: x is on {x.device}; there is no CPU path")
    if out is None:
        out = torch.zeros(k * k, Cc, device=x.device, dtype=torch.float32)
    ws = _workspace(what, x.device, int(L.lib().rdo_tap_sums_workspace(Cc, k)), torch.float32, Cc, k)
    L.check(L.lib().rdo_tap_sums(_ptr(x), N, H, W, Cc, k, stride, pad, Ho, Wo, int(transposed), _ptr(out), _ptr(ws), _stream()),
            "rdo_tap_sums")
    return out


def bias_shift(w_ref, w_q, s_ref, s_q, n, org_bias, shift=None, bias_out=None):
    """The bias shift of one layer from float64 tap sums (rdo_bias_shift): w_ref, w_q contiguous fp32 [O, ...] rows in the `to_rows`
    order, K = their row length; s_ref, s_q float64 of K elements (`tap_sums` results added up in float64, flattened [kh][kw][c]); n =
    the number of output pixels; org_bias fp32 [O].  -> (shift float64 [O] = (w_ref . s_ref - w_q . s_q) / n, both products and the
    difference in float64, and bias_out fp32 [O] = float32(org_bias + shift)).  Everything is checked on the host before a pointer is
    taken."""
    what = "bias_shift"
    f32, f64 = (torch.float32, "float32"), (torch.float64, "float64")
    for name, t, dt in (("w_ref", w_ref, f32), ("w_q", w_q, f32), ("org_bias", org_bias, f32), ("s_ref", s_ref, f64), ("s_q", s_q, f64)):
        A.tensor(what, name, t, *dt, contiguous=True, device=None if t is w_ref else w_ref.device, other="w_ref")
    if w_ref.dim() < 2 or w_q.shape != w_ref.shape:
        raise ValueError(f"{what}: w_ref {tuple(w_ref.shape)} and w_q {tuple(w_q.shape)} must be the same rows [O, ...] of rank >= 2")
    O = int(w_ref.shape[0])
    K = w_ref.numel() // O
    for name, t in (("s_ref", s_ref), ("s_q", s_q)):
        if t.numel() != K:
            raise ValueError(f"{what}: {name} holds {t.numel()} elements, the weight rows {K}")
    A.tensor(what, "org_bias", org_bias, *f32, shape=(O,))
    n = A.whole(what, "n", n, 1, want="a positive whole number of output pixels")
    for name, t, dt in (("shift", shift, f64), ("bias_out", bias_out, f32)):
        A.tensor(what, name, t, *dt, shape=(O,), contiguous=True, device=w_ref.device, optional=True, oneshot=True)
    if not w_ref.is_cuda:
        raise ValueError(f"{what}: the operands are on {w_ref.device}; there is no CPU path")
    shift = torch.empty(O, device=w_ref.device, dtype=torch.float64) if shift is None else shift
    bias_out = torch.empty(O, device=w_ref.device, dtype=torch.float32) if bias_out is None else bias_out
    L.check(L.lib().rdo_bias_shift(_ptr(w_ref), _ptr(w_q), _ptr64(s_ref), _ptr64(s_q), 1.0 / n, _ptr(org_bias), O, K, _ptr64(shift),
                                   _ptr(bias_out), _stream()), "rdo_bias_shift")
    return shift, bias_out


def width_list(what, widths, max_bits=L.WIDTH_SCAN_MAX_BITS):
    """`widths` as a list of ints: a non-empty sequence of at most 8 distinct whole numbers in 2 .. max_bits, else ValueError"""
    if isinstance(widths, (str, bytes)) or torch.is_tensor(widths) or not hasattr(widths, "__len__") or not hasattr(widths, "__iter__"):
        raise ValueError(f"{what}: widths must be a sequence of whole numbers, got {widths!r}")
    widths = list(widths)
    if not 1 <= len(widths) <= L.WIDTH_SCAN_MAX_K:
        raise ValueError(f"{what}: widths must hold 1 .. {L.WIDTH_SCAN_MAX_K} entries, got {len(widths)}")
    widths = [A.whole(what, "every width", b, L.WIDTH_SCAN_MIN_BITS, max_bits) for b in widths]
    if len(set(widths)) != len(widths):
        raise ValueError(f"{what}: widths must be distinct, got {widths}")
    return widths


def uaq_width_scan(w_rows, widths, delta=None, zp=None):
    """What round-to-nearest costs a weight at several widths, in one call (rdo_uaq_width_scan, include/rdo_ptq_bits.h): w_rows contiguous
    fp32 [rows, inner] (what `UniformAffineQuantizer._rows` gives, flattened to rank 2), widths: 1 .. 8 distinct whole numbers in 2 .. 16.
    -> (delta, zp fp32 [K, rows]; err float64 [K, rows] = sum (w - wq)^2 per row with wq the expression of `uaq_fakequant` on the grid of
    n_levels = 2^width; energy float64 [rows] = sum w^2).  With delta and zp None the grids are those of `uaq_init_minmax(w_rows, 2^width)`
    bit for bit; with both given (fp32 [K, rows] on w_rows' device) they are copied through and scored.  Float64 sums in a fixed order:
    the same input gives the same bits.  Everything is checked on the host before a pointer is taken."""
    what = "uaq_width_scan"
    A.tensor(what, "w_rows", w_rows, rank=2, layout="of rank 2 [rows, inner]", contiguous=True)
    widths = width_list(what, widths)
    rows, inner, K = int(w_rows.shape[0]), int(w_rows.shape[1]), len(widths)
    if rows > 0x7fffffff:
        raise ValueError(f"{what}: {rows} rows are beyond 32-bit row indices")
    if (delta is None) != (zp is None):
        raise ValueError(f"{what}: delta and zp must be given together or not at all")
    for name, t in (("delta", delta), ("zp", zp)):
        A.tensor(what, name, t, shape=(K, rows), contiguous=True, device=w_rows.device, optional=True, oneshot=True)
    if inner > L.WIDTH_SCAN_LDS_ROW and rows * -(-inner // L.WIDTH_SCAN_CHUNK) > 0x7fffffff:
        raise ValueError(f"{what}: [{rows}, {inner}] splits into more shares than 32-bit workgroup indices hold")
    if not w_rows.is_cuda:
        raise ValueError(f"{what}: w_rows is on {w_rows.device}; there is no CPU path")
    need = int(L.lib().rdo_uaq_width_scan_workspace(rows, inner, K))              # in bytes
    ws = _workspace(what, w_rows.device, -(-need // 8), torch.float64)
    out_d = torch.empty(K, rows, device=w_rows.device, dtype=torch.float32)
    out_z = torch.empty_like(out_d)
    err = torch.empty(K, rows, device=w_rows.device, dtype=torch.float64)
    energy = torch.empty(rows, device=w_rows.device, dtype=torch.float64)
    L.check(L.lib().rdo_uaq_width_scan(_ptr(w_rows), rows, inner, (C.c_int32 * K)(*widths), K, _ptr(delta), _ptr(zp), _ptr(out_d), _ptr(out_z),
                                       _ptr64(err), _ptr64(energy), _ptr64(ws), _stream()), "rdo_uaq_width_scan")
    return out_d, out_z, err, energy


def actquant_width_scan(x, rng, widths):
    """What ONE per-channel grid costs an activation at several widths, in one read of the tensor (rdo_actquant_width_scan,
    include/rdo_ptq_actbits.h): x contiguous fp32 [..., C] channels-last, rng fp32 [2C] = lo | hi on x's device, widths: 1 .. 8 distinct
    whole numbers in 2 .. 16.  -> (err fp32 [C, K] = sum (x - Q_k(x))^2 with Q_k the expression of `actquant_static` on rng at n_bits =
    widths[k]; energy fp32 [C] = sum x^2), both WRITTEN by the call (a caller that adds batches does so itself, in float64).  With rng =
    the tensor's own per-channel min | max, Q_k is `actquant_perchannel` at that width too.  fp32 sums in a fixed order: the same input
    gives the same bits.  Everything is checked on the host before a pointer is taken."""
    what = "actquant_width_scan"
    A.tensor(what, "x", x, contiguous=True)
    if x.dim() < 1:
        raise ValueError(f"{what}: x must be [..., C], got a scalar")
    Cc = int(x.shape[-1])
    npix = x.numel() // Cc
    A.tensor(what, "rng", rng, shape=(2 * Cc,), contiguous=True, device=x.device, oneshot=True)
    widths = width_list(what, widths, L.ACT_WIDTH_SCAN_MAX_BITS)
    K = len(widths)
    if npix > 0x7fffffff:
        raise ValueError(f"{what}: {npix} pixels are beyond 32-bit pixel counts")
    if Cc * (L.ACT_WIDTH_SCAN_MAX_K + 1) > 0x7fffffff:
        raise ValueError(f"{what}: {Cc} channels are too many for 32-bit entry indices")
    if not x.is_cuda:
        raise ValueError(f"{what}: x is on {x.device}; there is no CPU path")
    ws = _workspace(what, x.device, int(L.lib().rdo_actquant_width_scan_workspace(Cc, K)), torch.float32, Cc, K)
    err = torch.empty(Cc, K, device=x.device, dtype=torch.float32)
    energy = torch.empty(Cc, device=x.device, dtype=torch.float32)
    L.check(L.lib().rdo_actquant_width_scan(_ptr(x), npix, Cc, _ptr(rng), (C.c_int32 * K)(*widths), K, _ptr(err), _ptr(energy), _ptr(ws),
                                            _stream()), "rdo_actquant_width_scan")
    return err, energy


MX_OUTPUTS = ("wq", "scales", "codes", "err", "energy")      # what `mx_fakequant` can be asked for, in the order of the C entry


def mx_format(what, fmt):
    """(id, element bits) of the MX format named `fmt`; ValueError listing the table for anything else"""
    if not isinstance(fmt, str) or fmt not in L.MX_FORMATS:
        raise ValueError(f"{what}: unknown MX format {fmt!r}; the formats are {list(L.MX_FORMATS)}")
    return L.MX_FORMATS[fmt]


def _mx_geometry(what, rows, inner):
    nb = -(-inner // L.MX_BLOCK)
    if rows > 0x7fffffff or rows * nb > 2 ** 40:
        raise ValueError(f"{what}: [{rows}, {inner}] is beyond 2^31 - 1 rows or 2^40 blocks")
    return nb


def mx_fakequant(w_rows, fmt, want=("wq",), wq_out=None):
    """Quantise a weight-row matrix to an MX block format (rdo_mx_fakequant; include/rdo_ptq_mx.h states the formats): w_rows contiguous
    fp32 [rows, inner] (what `to_rows` gives, flattened to rank 2), fmt a name of `MX_FORMATS`, want a non-empty sequence of distinct
    names out of `MX_OUTPUTS`.  -> dict of the requested outputs: 'wq' fp32 [rows, inner], 'scales' uint8 [rows, ceil(inner / 32)] (E8M0
    codes, 255 for a block that holds a NaN or an infinity), 'codes' uint8 [rows, inner], 'err' float64 [rows] = sum (w - wq)^2 with
    the difference formed in fp32, 'energy' float64 [rows] = sum w^2.  Float64 sums in a fixed order: the same input gives the same bits.
    `wq_out`: a contiguous fp32 [rows, inner] to write 'wq' into; it may be w_rows itself.  Everything is checked on the host before a
    pointer is taken."""
    what = "mx_fakequant"
    A.tensor(what, "w_rows", w_rows, rank=2, layout="of rank 2 [rows, inner]", contiguous=True)
    fid, _ = mx_format(what, fmt)
    if isinstance(want, (str, bytes)) or not hasattr(want, "__iter__"):
        raise ValueError(f"{what}: want must be a sequence of names out of {list(MX_OUTPUTS)}, got {want!r}")
    want = list(want)
    if not want or any(n not in MX_OUTPUTS for n in want) or len(set(want)) != len(want):
        raise ValueError(f"{what}: want must hold at least one and only distinct names out of {list(MX_OUTPUTS)}, got {want!r}")
    rows, inner, dev = int(w_rows.shape[0]), int(w_rows.shape[1]), w_rows.device
    nb = _mx_geometry(what, rows, inner)
    if wq_out is not None and "wq" not in want:
        raise ValueError(f"{what}: wq_out is given but 'wq' is not wanted")
    A.tensor(what, "wq_out", wq_out, shape=(rows, inner), contiguous=True, device=dev, optional=True, oneshot=True)
    if not w_rows.is_cuda:
        raise ValueError(f"{what}: w_rows is on {dev}; there is no CPU path")
    out = {}
    if "wq" in want:
        out["wq"] = torch.empty(rows, inner, device=dev, dtype=torch.float32) if wq_out is None else wq_out
    if "scales" in want:
        out["scales"] = torch.empty(rows, nb, device=dev, dtype=torch.uint8)
    if "codes" in want:
        out["codes"] = torch.empty(rows, inner, device=dev, dtype=torch.uint8)
    for n in ("err", "energy"):
        if n in want:
            out[n] = torch.empty(rows, device=dev, dtype=torch.float64)
    ws = None
    if "err" in want or "energy" in want:
        ws = _workspace(what, dev, -(-int(L.lib().rdo_mx_fakequant_workspace(rows, inner)) // 8), torch.float64)
    u8 = ((torch.uint8,), "uint8")
    L.check(L.lib().rdo_mx_fakequant(_ptr(w_rows), rows, inner, fid, _ptr(out.get("wq")), _ptr(out.get("scales"), *u8),
                                     _ptr(out.get("codes"), *u8), _ptr64(out.get("err")), _ptr64(out.get("energy")), _ptr64(ws), _stream()),
            "rdo_mx_fakequant")
    return {n: out[n] for n in want}


def mx_dequant(codes, scales, inner, fmt):
    """fp32 [rows, inner] from what `mx_fakequant` gave as 'codes' (contiguous uint8 [rows, inner]) and 'scales' (contiguous uint8 [rows,
    ceil(inner / 32)] on its device): bit for bit the 'wq' of that call (rdo_mx_dequant).  A scale code of 255 gives NaN.  Everything is
    checked on the host before a pointer is taken."""
    what = "mx_dequant"
    A.tensor(what, "codes", codes, torch.uint8, "uint8", rank=2, layout="of rank 2 [rows, inner]", contiguous=True)
    fid, _ = mx_format(what, fmt)
    inner = A.whole(what, "inner", inner, 1)
    rows, dev = int(codes.shape[0]), codes.device
    if codes.shape[1] != inner:
        raise ValueError(f"{what}: codes is {tuple(codes.shape)}; inner is {inner}")
    nb = _mx_geometry(what, rows, inner)
    A.tensor(what, "scales", scales, torch.uint8, "uint8", shape=(rows, nb), contiguous=True, device=dev, oneshot=True)
    if not codes.is_cuda:
        raise ValueError(f"{what}: codes is on {dev}; there is no CPU path")
    w = torch.empty(rows, inner, device=dev, dtype=torch.float32)
    u8 = ((torch.uint8,), "uint8")
    L.check(L.lib().rdo_mx_dequant(_ptr(codes, *u8), _ptr(scales, *u8), rows, inner, fid, _ptr(w), _stream()), "rdo_mx_dequant")
    return w


# ---- learned rounding on the MX grids (include/rdo_ptq_mxround.h) -----------------------------------------------------------------------
_U8 = ((torch.uint8,), "uint8")


def _mx_cuda(what, t, name):
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} is on {t.device}; there is no CPU path")


def mx_neighbours(w_rows, fmt, want_scales=False):
    """The neighbours of every element of a weight-row matrix on the grid of its block (rdo_mx_neighbours; include/rdo_ptq_mxround.h states
    the definitions): w_rows contiguous fp32 [rows, inner] -> (lo, gap) fp32 [rows, inner], lo the largest grid value <= w and gap the
    distance to the next one; gap == 0 marks a pinned element (lo = +-max X) or a block that is not finite (lo = NaN).  want_scales:
    -> (lo, gap, scales), scales uint8 [rows, ceil(inner / 32)], the bytes `mx_fakequant` gives.  Checked on the host before a pointer
    is taken."""
    what = "mx_neighbours"
    A.tensor(what, "w_rows", w_rows, rank=2, layout="of rank 2 [rows, inner]", contiguous=True)
    fid, _ = mx_format(what, fmt)
    rows, inner, dev = int(w_rows.shape[0]), int(w_rows.shape[1]), w_rows.device
    nb = _mx_geometry(what, rows, inner)
    _mx_cuda(what, w_rows, "w_rows")
    lo, gap = torch.empty_like(w_rows), torch.empty_like(w_rows)
    scales = torch.empty(rows, nb, device=dev, dtype=torch.uint8) if want_scales else None
    L.check(L.lib().rdo_mx_neighbours(_ptr(w_rows), rows, inner, fid, _ptr(lo), _ptr(gap), _ptr(scales, *_U8), _stream()), "rdo_mx_neighbours")
    return (lo, gap, scales) if want_scales else (lo, gap)


def _mx_same(what, first, **named):
    """every named tensor: contiguous fp32 with the element count and device of `first` = (name, tensor), itself checked first"""
    A.tensor(what, first[0], first[1], contiguous=True)
    for name, t in named.items():
        A.tensor(what, name, t, numel=first[1].numel(), contiguous=True, device=first[1].device, other=first[0])
    _mx_cuda(what, first[1], first[0])
    return first[1].numel()


def mx_round_init_alpha(w, lo, gap, alpha=None):
    """alpha0 = -log(1.2 / (rest + 0.1) - 1) with rest = (w - lo) / gap in fp32; 0 for a pinned element (rdo_mx_round_init_alpha).
    w, lo, gap (and alpha, made when None): contiguous fp32 of one element count on one device."""
    what = "mx_round_init_alpha"
    alpha = torch.empty_like(w) if (alpha is None and torch.is_tensor(w)) else alpha
    n = _mx_same(what, ("w", w), lo=lo, gap=gap, alpha=alpha)
    L.check(L.lib().rdo_mx_round_init_alpha(_ptr(w), _ptr(lo), _ptr(gap), n, _ptr(alpha), _stream()), "rdo_mx_round_init_alpha")
    return alpha


def _mx_desc(what, d, lo):
    if not isinstance(d, L.AdaDesc) or d.numel != lo.numel() or d.rows < 1 or d.numel % d.rows:
        raise ValueError(f"{what}: d must be an `ada_desc` of the {lo.numel()} elements of lo, got "
                         f"{(d.numel, d.rows) if isinstance(d, L.AdaDesc) else type(d).__name__}")


def mx_round_fwd(d, lo, gap, alpha, soft, fmt, wq=None, wd=None, codes=None, scales=None):
    """Soft (soft=True) or hard weight lo + gap * h on an MX grid into the kernel layouts of `adaround_fwd` (rdo_mx_round_fwd): `wq` in
    the layout of lo (made when None), `wd` (optional) the dgrad layout of the descriptor `d` (`ada_desc`; a gamma's transpose), the GDN
    re-parametrisation of `d` applied.  codes=True (hard only; needs `scales`, uint8 [rows, ceil(inner / 32)] of `mx_neighbours` /
    `mx_fakequant`): -> (wq, codes), codes uint8 [rows, inner] with `mx_dequant(codes, scales)` the hard weight before the reparam bit for
    bit.  Everything is checked on the host before a pointer is taken."""
    what = "mx_round_fwd"
    fid, _ = mx_format(what, fmt)
    wq = torch.empty_like(lo) if (wq is None and torch.is_tensor(lo)) else wq
    _mx_same(what, ("lo", lo), gap=gap, alpha=alpha, wq=wq)
    A.tensor(what, "wd", wd, numel=lo.numel(), contiguous=True, device=lo.device, optional=True, oneshot=True)
    _mx_desc(what, d, lo)
    rows, inner = int(d.rows), int(d.numel // d.rows)
    cd = None
    if codes:
        if soft:
            raise ValueError(f"{what}: codes describe the hard weight: soft must be False")
        A.tensor(what, "scales", scales, torch.uint8, "uint8", shape=(rows, _mx_geometry(what, rows, inner)), contiguous=True, device=lo.device,
                 oneshot=True)
        cd = torch.empty(rows, inner, device=lo.device, dtype=torch.uint8)
    L.check(L.lib().rdo_mx_round_fwd(C.byref(d), _ptr(lo), _ptr(gap), _ptr(alpha), int(bool(soft)), _ptr(wq), _ptr(wd), _ptr(cd, *_U8),
                                     _ptr(scales if codes else None, *_U8), fid, _stream()), "rdo_mx_round_fwd")
    return (wq, cd) if codes else wq


def mx_round_step(d, lo, gap, slabs, grad_scale, round_weight, sched, iter_ptr, alpha, m, v, wq, wd, round_log):
    """One fused AdaRound step on an MX grid (rdo_mx_round_step): `adaround_step` with (lo, gap) in place of (w, delta, zp) and no plane
    outputs.  slabs fp32 [nsplit, ...] of nsplit * numel elements; sched fp32 [iters, 4] (`make_sched`); iter_ptr one int32; round_log
    fp32 [iters, LOG_SLOTS] or None.  Pinned elements (gap == 0) keep alpha, m and v.  Checked on the host before a pointer is taken."""
    what = "mx_round_step"
    n = _mx_same(what, ("lo", lo), gap=gap, alpha=alpha, m=m, v=v, wq=wq)
    dev = lo.device
    A.tensor(what, "wd", wd, numel=n, contiguous=True, device=dev, optional=True, oneshot=True)
    _mx_desc(what, d, lo)
    A.tensor(what, "slabs", slabs, contiguous=True, device=dev, other="lo")
    if slabs.dim() < 1 or slabs.shape[0] < 1 or slabs.numel() != slabs.shape[0] * n:
        raise ValueError(f"{what}: slabs must be [nsplit, ...] with {n} elements a slab, got {tuple(slabs.shape)}")
    A.tensor(what, "sched", sched, rank=2, layout="of rank 2 [iters, 4]", contiguous=True, device=dev, other="lo")
    if sched.shape[1] != 4:
        raise ValueError(f"{what}: sched must be [iters, 4], got {tuple(sched.shape)}")
    A.tensor(what, "iter_ptr", iter_ptr, torch.int32, "int32", numel=1, device=dev, other="lo")
    A.tensor(what, "round_log", round_log, shape=(sched.shape[0], L.LOG_SLOTS), contiguous=True, device=dev, optional=True, oneshot=True)
    L.check(L.lib().rdo_mx_round_step(C.byref(d), _ptr(lo), _ptr(gap), _ptr(slabs), int(slabs.shape[0]), float(grad_scale), float(round_weight),
                                      _ptr(sched), _ptr(iter_ptr), _ptr(alpha), _ptr(m), _ptr(v), _ptr(wq), _ptr(wd), _ptr(round_log), _stream()),
            "rdo_mx_round_step")


# ---- MX codes on the block-scaled matrix instruction (include/rdo_ptq_mxgemm.h) -------------------------------------------------------------
class MXOperand:
    """A packed MX operand of `mx_gemm`: `.packed` uint8 [rows, K / 32 * 4 b] (blocks of 4 b bytes, b the element bits of `.fmt`; the byte
    image is stated in include/rdo_ptq_mxgemm.h), `.scales` uint8 [rows, K / 32] (E8M0 bytes), `.fmt` a name of `MX_FORMATS`, `.rows`, `.K`."""
    __slots__ = ("packed", "scales", "fmt", "rows", "K")

    def __init__(self, packed, scales, fmt, rows, K):
        self.packed, self.scales, self.fmt, self.rows, self.K = packed, scales, fmt, int(rows), int(K)

    @property
    def device(self):
        return self.packed.device

    def __repr__(self):
        return f"MXOperand({self.fmt}, rows={self.rows}, K={self.K}, device={self.packed.device})"


def _mx_k(what, rows, K):
    """blocks a row of a packed operand: K must be a whole number of blocks"""
    if K % L.MX_BLOCK:
        raise ValueError(f"{what}: K = {K} is no multiple of the MX block size {L.MX_BLOCK}")
    return _mx_geometry(what, rows, K)


def _mx_operand(what, name, op, device=None):
    """an `MXOperand` whose tensors have the shapes its fields state; -> (format id, element bits, blocks a row)"""
    if not isinstance(op, MXOperand):
        raise ValueError(f"{what}: {name} must be an MXOperand, got {type(op).__name__}")
    fid, bits = mx_format(what, op.fmt)
    if op.rows < 1 or op.K < 1:
        raise ValueError(f"{what}: {name} states rows {op.rows} and K {op.K}")
    nb = _mx_k(what, op.rows, op.K)
    A.tensor(what, f"{name}.packed", op.packed, torch.uint8, "uint8", shape=(op.rows, nb * 4 * bits), contiguous=True, device=device, oneshot=True)
    A.tensor(what, f"{name}.scales", op.scales, torch.uint8, "uint8", shape=(op.rows, nb), contiguous=True, device=op.packed.device, oneshot=True)
    return fid, bits, nb


def mx_pack_codes(codes, scales, fmt):
    """An `MXOperand` from one-code-per-byte element codes (contiguous uint8 [rows, K], K % 32 == 0: 'codes' of `mx_fakequant`, the codes of
    `mx_round_fwd`) and their scale bytes (contiguous uint8 [rows, K / 32]; kept, not copied) (rdo_mx_pack_codes).  Checked on the host
    before a pointer is taken."""
    what = "mx_pack_codes"
    A.tensor(what, "codes", codes, torch.uint8, "uint8", rank=2, layout="of rank 2 [rows, K]", contiguous=True)
    fid, bits = mx_format(what, fmt)
    rows, K, dev = int(codes.shape[0]), int(codes.shape[1]), codes.device
    nb = _mx_k(what, rows, K)
    A.tensor(what, "scales", scales, torch.uint8, "uint8", shape=(rows, nb), contiguous=True, device=dev, oneshot=True)
    _mx_cuda(what, codes, "codes")
    packed = torch.empty(rows, nb * 4 * bits, device=dev, dtype=torch.uint8)
    L.check(L.lib().rdo_mx_pack_codes(_ptr(codes, *_U8), rows, K, fid, _ptr(packed, *_U8), _stream()), "rdo_mx_pack_codes")
    return MXOperand(packed, scales, fmt, rows, K)


def mx_quant_pack(x2d, fmt, want_xq=False):
    """Quantise activation rows to the MX format `fmt` and pack them in one read (rdo_mx_quant_pack): x2d contiguous fp32 [rows, K], K % 32
    == 0, blocks of 32 along K -> `MXOperand`; want_xq: -> (operand, xq), xq fp32 [rows, K] the decoded values.  Bit for bit `mx_fakequant`
    followed by `mx_pack_codes`.  Checked on the host before a pointer is taken."""
    what = "mx_quant_pack"
    A.tensor(what, "x2d", x2d, rank=2, layout="of rank 2 [rows, K]", contiguous=True)
    fid, bits = mx_format(what, fmt)
    rows, K, dev = int(x2d.shape[0]), int(x2d.shape[1]), x2d.device
    nb = _mx_k(what, rows, K)
    _mx_cuda(what, x2d, "x2d")
    packed = torch.empty(rows, nb * 4 * bits, device=dev, dtype=torch.uint8)
    scales = torch.empty(rows, nb, device=dev, dtype=torch.uint8)
    xq = torch.empty_like(x2d) if want_xq else None
    L.check(L.lib().rdo_mx_quant_pack(_ptr(x2d), rows, K, fid, _ptr(packed, *_U8), _ptr(scales, *_U8), _ptr(xq), _stream()), "rdo_mx_quant_pack")
    op = MXOperand(packed, scales, fmt, rows, K)
    return (op, xq) if want_xq else op


def mx_unpack_codes(op):
    """codes uint8 [rows, K] of an `MXOperand`: the inverse of `mx_pack_codes` (rdo_mx_unpack_codes)"""
    what = "mx_unpack_codes"
    fid, _, _ = _mx_operand(what, "op", op)
    _mx_cuda(what, op.packed, "op.packed")
    codes = torch.empty(op.rows, op.K, device=op.packed.device, dtype=torch.uint8)
    L.check(L.lib().rdo_mx_unpack_codes(_ptr(op.packed, *_U8), op.rows, op.K, fid, _ptr(codes, *_U8), _stream()), "rdo_mx_unpack_codes")
    return codes


# ---- the stored rows of a packed MX checkpoint (include/rdo_ptq_mxfile.h) ----------------------------------------------------------------
MX_UNPACK_OUTPUTS = ("w", "codes")      # what `mx_unpack_dequant` can be asked for


def mx_pack_rows(codes, fmt, out=None):
    """The bytes a packed MX checkpoint stores for a weight (rdo_mx_pack_rows): codes contiguous uint8 [rows, inner] of any inner >= 1,
    one code per byte (upper bits ignored) -> uint8 [rows, ceil(inner / 32) * 4 b]; the missing elements of a short last block are zero
    codes.  For inner % 32 == 0 it is `mx_pack_codes(...).packed` bit for bit.  `out`: a contiguous uint8 tensor of that shape on the
    codes' device, 4-byte aligned, to write into.  Checked on the host before a pointer is taken."""
    what = "mx_pack_rows"
    A.tensor(what, "codes", codes, torch.uint8, "uint8", rank=2, layout="of rank 2 [rows, inner]", contiguous=True)
    fid, bits = mx_format(what, fmt)
    rows, inner, dev = int(codes.shape[0]), int(codes.shape[1]), codes.device
    nb = _mx_geometry(what, rows, inner)
    A.tensor(what, "out", out, torch.uint8, "uint8", shape=(rows, nb * 4 * bits), contiguous=True, device=dev, optional=True, oneshot=True)
    _mx_cuda(what, codes, "codes")
    packed = torch.empty(rows, nb * 4 * bits, device=dev, dtype=torch.uint8) if out is None else out
    L.check(L.lib().rdo_mx_pack_rows(_ptr(codes, *_U8), rows, inner, fid, _ptr(packed, *_U8), _stream()), "rdo_mx_pack_rows")
    return packed


def mx_unpack_dequant(packed, scales, inner, fmt, want=("w",), w_out=None, codes_out=None):
    """From the stored rows back to the weight in one launch (rdo_mx_unpack_dequant): packed contiguous uint8 [rows, ceil(inner / 32) *
    4 b] (what `mx_pack_rows` gives), scales contiguous uint8 [rows, ceil(inner / 32)] on its device, want a non-empty sequence of
    distinct names out of `MX_UNPACK_OUTPUTS` -> dict: 'w' fp32 [rows, inner], bit for bit `mx_dequant` of the codes (a scale code of
    255 gives NaN), 'codes' uint8 [rows, inner] with zero upper bits.  `w_out` / `codes_out`: contiguous tensors of those shapes on
    packed's device to write a wanted output into.  Checked on the host before a pointer is taken."""
    what = "mx_unpack_dequant"
    A.tensor(what, "packed", packed, torch.uint8, "uint8", rank=2, layout="of rank 2 [rows, row bytes]", contiguous=True)
    fid, bits = mx_format(what, fmt)
    inner = A.whole(what, "inner", inner, 1)
    if isinstance(want, (str, bytes)) or not hasattr(want, "__iter__"):
        raise ValueError(f"{what}: want must be a sequence of names out of {list(MX_UNPACK_OUTPUTS)}, got {want!r}")
    want = list(want)
    if not want or any(n not in MX_UNPACK_OUTPUTS for n in want) or len(set(want)) != len(want):
        raise ValueError(f"{what}: want must hold at least one and only distinct names out of {list(MX_UNPACK_OUTPUTS)}, got {want!r}")
    rows, dev = int(packed.shape[0]), packed.device
    nb = _mx_geometry(what, rows, inner)
    if packed.shape[1] != nb * 4 * bits:
        raise ValueError(f"{what}: packed is {tuple(packed.shape)}; a row of inner {inner} in {fmt} has {nb * 4 * bits} bytes")
    A.tensor(what, "scales", scales, torch.uint8, "uint8", shape=(rows, nb), contiguous=True, device=dev, oneshot=True)
    for name, given in (("w", w_out), ("codes", codes_out)):
        if given is not None and name not in want:
            raise ValueError(f"{what}: {name}_out is given but {name!r} is not wanted")
    A.tensor(what, "w_out", w_out, shape=(rows, inner), contiguous=True, device=dev, optional=True, oneshot=True)
    A.tensor(what, "codes_out", codes_out, torch.uint8, "uint8", shape=(rows, inner), contiguous=True, device=dev, optional=True, oneshot=True)
    _mx_cuda(what, packed, "packed")
    out = {}
    if "w" in want:
        out["w"] = torch.empty(rows, inner, device=dev, dtype=torch.float32) if w_out is None else w_out
    if "codes" in want:
        out["codes"] = torch.empty(rows, inner, device=dev, dtype=torch.uint8) if codes_out is None else codes_out
    L.check(L.lib().rdo_mx_unpack_dequant(_ptr(packed, *_U8), _ptr(scales, *_U8), rows, inner, fid, _ptr(out.get("w")),
                                          _ptr(out.get("codes"), *_U8), _stream()), "rdo_mx_unpack_dequant")
    return {n: out[n] for n in want}


def mx_gemm(a, b, bias=None):
    """y fp32 [M, N] = A B^T (+ bias) on the block-scaled matrix instruction (rdo_mx_gemm): a an `MXOperand` [M, K], b an `MXOperand` [N, K]
    of any two formats, bias contiguous fp32 [N] or None.  The products are exact; the sum is the instruction's fp32 accumulation.
    Checked on the host before a pointer is taken."""
    what = "mx_gemm"
    fa, _, _ = _mx_operand(what, "a", a)
    fb, _, _ = _mx_operand(what, "b", b, device=a.packed.device)
    if a.K != b.K:
        raise ValueError(f"{what}: a has K = {a.K}, b has K = {b.K}")
    dev = a.packed.device
    A.tensor(what, "bias", bias, shape=(b.rows,), contiguous=True, device=dev, optional=True, oneshot=True)
    _mx_cuda(what, a.packed, "a.packed")
    y = torch.empty(a.rows, b.rows, device=dev, dtype=torch.float32)
    L.check(L.lib().rdo_mx_gemm(_ptr(a.packed, *_U8), _ptr(a.scales, *_U8), fa, _ptr(b.packed, *_U8), _ptr(b.scales, *_U8), fb, a.rows, b.rows,
                                a.K, _ptr(bias), _ptr(y), _stream()), "rdo_mx_gemm")
    return y


def mx_conv2d(x, w, shape, k, stride=1, pad=0, bias=None):
    """y fp32 [B, Ho, Wo, N] = conv(x, w) (+ bias) on the block-scaled matrix instruction (rdo_mx_conv2d; include/rdo_ptq_mxconv.h): x an
    `MXOperand` [B * H * W, C] -- an NHWC activation, one packed row per pixel, what `mx_quant_pack` makes of the NHWC rows --, shape =
    (B, H, W), w an `MXOperand` [N, k * k * C] whose rows are in (kh, kw, in) order (`to_rows`), of any two formats; square kernel k, one
    stride >= 1, one zero padding >= 0, dilation 1, groups 1; bias contiguous fp32 [N] or None.  Ho = (H + 2 pad - k) // stride + 1, Wo
    likewise.  Bit for bit `mx_gemm` on the im2col matrix of x.  Checked on the host before a pointer is taken."""
    what = "mx_conv2d"
    fx, _, _ = _mx_operand(what, "x", x)
    fw, _, _ = _mx_operand(what, "w", w, device=x.packed.device)
    if isinstance(shape, (str, bytes)) or not hasattr(shape, "__len__") or len(shape) != 3:
        raise ValueError(f"{what}: shape must be (B, H, W), got {shape!r}")
    B, H, W = (A.whole(what, f"shape[{i}]", v, 1) for i, v in enumerate(shape))
    k, stride, pad = A.whole(what, "k", k, 1), A.whole(what, "stride", stride, 1), A.whole(what, "pad", pad, 0)
    if x.rows != B * H * W:
        raise ValueError(f"{what}: x has {x.rows} rows, shape {(B, H, W)} states {B * H * W} pixels")
    if w.K != k * k * x.K:
        raise ValueError(f"{what}: w has K = {w.K}, a {k} x {k} kernel over x's {x.K} channels needs K = {k * k * x.K}")
    if H + 2 * pad < k or W + 2 * pad < k:
        raise ValueError(f"{what}: a {k} x {k} kernel does not fit the {H} x {W} input under padding {pad}")
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if B * Ho * Wo > 0x7fffffff or max(k, stride, pad, x.K) > 0x7fffffff:
        raise ValueError(f"{what}: {B} x {Ho} x {Wo} output pixels, {x.K} channels, k {k}, stride {stride} or pad {pad} is beyond 2^31 - 1")
    dev = x.packed.device
    A.tensor(what, "bias", bias, shape=(w.rows,), contiguous=True, device=dev, optional=True, oneshot=True)
    _mx_cuda(what, x.packed, "x.packed")
    y = torch.empty(B, Ho, Wo, w.rows, device=dev, dtype=torch.float32)
    L.check(L.lib().rdo_mx_conv2d(_ptr(x.packed, *_U8), _ptr(x.scales, *_U8), fx, _ptr(w.packed, *_U8), _ptr(w.scales, *_U8), fw, B, H, W, x.K,
                                  w.rows, k, stride, pad, _ptr(bias), _ptr(y), _stream()), "rdo_mx_conv2d")
    return y


def mx_conv_transpose2d(x, w, shape, k, stride=1, pad=0, output_padding=0, bias=None):
    """y fp32 [B, Ho, Wo, N] = conv_transpose(x, w) (+ bias) on the block-scaled matrix instruction (rdo_mx_conv_transpose2d;
    include/rdo_ptq_mxtconv.h): x an `MXOperand` [B * H * W, C] -- an NHWC activation, one packed row per pixel, what `mx_quant_pack`
    makes of the NHWC rows --, shape = (B, H, W), w an `MXOperand` [N, k * k * C] whose rows are those of `to_rows(W, tconv=True)`
    ((kh, kw, in) order, taps un-flipped), of any two formats; square kernel k, one stride >= 1, one padding >= 0, one output padding
    in 0 .. stride - 1, dilation 1, groups 1; bias contiguous fp32 [N] or None.  Ho = (H - 1) stride - 2 pad + k + output_padding, Wo
    likewise.  Phase by phase bit for bit `mx_gemm` on the gathered operands.  Checked on the host before a pointer is taken."""
    what = "mx_conv_transpose2d"
    fx, _, _ = _mx_operand(what, "x", x)
    fw, _, _ = _mx_operand(what, "w", w, device=x.packed.device)
    if isinstance(shape, (str, bytes)) or not hasattr(shape, "__len__") or len(shape) != 3:
        raise ValueError(f"{what}: shape must be (B, H, W), got {shape!r}")
    B, H, W = (A.whole(what, f"shape[{i}]", v, 1) for i, v in enumerate(shape))
    k, stride, pad = A.whole(what, "k", k, 1), A.whole(what, "stride", stride, 1), A.whole(what, "pad", pad, 0)
    opad = A.whole(what, "output_padding", output_padding, 0)
    if opad >= stride:
        raise ValueError(f"{what}: output_padding {opad} must be below the stride {stride}")
    if x.rows != B * H * W:
        raise ValueError(f"{what}: x has {x.rows} rows, shape {(B, H, W)} states {B * H * W} pixels")
    if w.K != k * k * x.K:
        raise ValueError(f"{what}: w has K = {w.K}, a {k} x {k} kernel over x's {x.K} channels needs K = {k * k * x.K}")
    Ho, Wo = (H - 1) * stride - 2 * pad + k + opad, (W - 1) * stride - 2 * pad + k + opad
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f"{what}: a {k} x {k} kernel at stride {stride}, padding {pad} and output padding {opad} leaves no output of the "
                         f"{H} x {W} input")
    if B * Ho * Wo > 0x7fffffff or max(k, stride, pad, x.K) > 0x7fffffff:
        raise ValueError(f"{what}: {B} x {Ho} x {Wo} output pixels, {x.K} channels, k {k}, stride {stride} or pad {pad} is beyond 2^31 - 1")
    dev = x.packed.device
    A.tensor(what, "bias", bias, shape=(w.rows,), contiguous=True, device=dev, optional=True, oneshot=True)
    _mx_cuda(what, x.packed, "x.packed")
    y = torch.empty(B, Ho, Wo, w.rows, device=dev, dtype=torch.float32)
    L.check(L.lib().rdo_mx_conv_transpose2d(_ptr(x.packed, *_U8), _ptr(x.scales, *_U8), fx, _ptr(w.packed, *_U8), _ptr(w.scales, *_U8), fw, B, H,
                                            W, x.K, w.rows, k, stride, pad, opad, _ptr(bias), _ptr(y), _stream()), "rdo_mx_conv_transpose2d")
    return y


def pack_row_words(inner, bits):
    """W = ceil(inner * bits / 32): the 32-bit words one row of `inner` codes of `bits` bits occupies (rdo_pack_row_words on the host)"""
    return -(-int(inner) * int(bits) // 32)


def _pack_geometry(what, rows, inner, bits):
    W = pack_row_words(inner, bits)
    if rows > 0x7fffffff or W > 0x7fffffff or rows * W > 2 ** 40:
        raise ValueError(f"{what}: [{rows}, {inner}] at {bits} bits is beyond 2^31 - 1 rows, 2^31 - 1 words a row or 2^40 words")
    return W


def weight_pack(w_rows, delta, zp, bits, alpha_rows=None, out=None):
    """Quantise a weight-row matrix to integer levels and pack them at their own width (rdo_weight_pack; include/rdo_ptq_pack.h states
    the bit layout): w_rows contiguous fp32 [rows, inner] (what `UniformAffineQuantizer._rows` gives, flattened to rank 2), delta and zp
    fp32 [rows] on its device, bits a whole number in 2 .. 16.  alpha_rows None: round to nearest, the level inside `uaq_fakequant`;
    given (fp32 [rows, inner]): down, plus one where alpha >= 0, the level inside `adaround_fwd(..., soft=False)`.
    -> int32 [rows, W] holding raw bits, W = ceil(inner * bits / 32); every word is written, the padding bits are zero.  `out`: a
    contiguous int32 [rows, W] to write into.  Everything is checked on the host before a pointer is taken."""
    what = "weight_pack"
    A.tensor(what, "w_rows", w_rows, rank=2, layout="of rank 2 [rows, inner]", contiguous=True)
    bits = A.whole(what, "bits", bits, L.PACK_MIN_BITS, L.PACK_MAX_BITS)
    rows, inner, dev = int(w_rows.shape[0]), int(w_rows.shape[1]), w_rows.device
    fits = dict(contiguous=True, device=dev, oneshot=True)
    A.tensor(what, "delta", delta, shape=(rows,), **fits)
    A.tensor(what, "zp", zp, shape=(rows,), **fits)
    A.tensor(what, "alpha_rows", alpha_rows, shape=(rows, inner), optional=True, **fits)
    W = _pack_geometry(what, rows, inner, bits)
    A.tensor(what, "out", out, torch.int32, "int32", shape=(rows, W), optional=True, **fits)
    if not w_rows.is_cuda:
        raise ValueError(f"{what}: w_rows is on {dev}; there is no CPU path")
    out = torch.empty(rows, W, device=dev, dtype=torch.int32) if out is None else out
    L.check(L.lib().rdo_weight_pack(_ptr(w_rows), _ptr(alpha_rows), _ptr(delta), _ptr(zp), rows, inner, bits, _ptr(out), _stream()),
            "rdo_weight_pack")
    return out


def weight_unpack(packed, delta, zp, inner, bits, levels=True, dequant=True, levels_out=None, wq_out=None):
    """Unpack what `weight_pack` made (rdo_weight_unpack): packed contiguous int32 [rows, W] with W = ceil(inner * bits / 32), delta and zp
    fp32 [rows] on its device (both may be None when `dequant` is False).  -> (levels, wq): int32 [rows, inner] when `levels`, else None;
    fp32 [rows, inner] = (level - zp) * delta, the tail expression of the fake-quantisation kernels, when `dequant`, else None.  At
    least one of the two must be asked for.  `levels_out`, `wq_out`: contiguous tensors to write into.  Everything is checked on the
    host before a pointer is taken."""
    what = "weight_unpack"
    A.tensor(what, "packed", packed, torch.int32, "int32", rank=2, layout="of rank 2 [rows, W]", contiguous=True)
    bits = A.whole(what, "bits", bits, L.PACK_MIN_BITS, L.PACK_MAX_BITS)
    inner = A.whole(what, "inner", inner, 1)
    if not (isinstance(levels, bool) and isinstance(dequant, bool) and (levels or dequant)):
        raise ValueError(f"{what}: levels and dequant must be True or False, and one of them True; got {levels!r}, {dequant!r}")
    rows, dev = int(packed.shape[0]), packed.device
    fits = dict(contiguous=True, device=dev, oneshot=True)
    W = _pack_geometry(what, rows, inner, bits)
    if packed.shape[1] != W:
        raise ValueError(f"{what}: packed is {tuple(packed.shape)}; {inner} codes of {bits} bits make W = {W} words a row")
    if dequant or delta is not None or zp is not None:
        A.tensor(what, "delta", delta, shape=(rows,), **fits)
        A.tensor(what, "zp", zp, shape=(rows,), **fits)
    if levels_out is not None and not levels:
        raise ValueError(f"{what}: levels_out is given but levels is False")
    A.tensor(what, "levels_out", levels_out, torch.int32, "int32", shape=(rows, inner), optional=True, **fits)
    if wq_out is not None and not dequant:
        raise ValueError(f"{what}: wq_out is given but dequant is False")
    A.tensor(what, "wq_out", wq_out, shape=(rows, inner), optional=True, **fits)
    if not packed.is_cuda:
        raise ValueError(f"{what}: packed is on {dev}; there is no CPU path")
    lv = wq = None
    if levels:
        lv = torch.empty(rows, inner, device=dev, dtype=torch.int32) if levels_out is None else levels_out
    if dequant:
        wq = torch.empty(rows, inner, device=dev, dtype=torch.float32) if wq_out is None else wq_out
    L.check(L.lib().rdo_weight_unpack(_ptr(packed), _ptr(delta) if dequant else None, _ptr(zp) if dequant else None, rows, inner, bits,
                                      _ptr(lv), _ptr(wq), _stream()), "rdo_weight_unpack")
    return lv, wq


def actquant_static_bwd(x, g, rng, drange, dx=None, n_bits=8, ws=None):
    """Backward of `actquant_static` with a straight-through round: returns dx (= g inside the range, 0 outside; `dx` may be g) and
    accumulates the per-channel range gradient into drange [2C] = dlo | dhi.  x, g: [..., C] channels-last, contiguous."""
    Cc, npix = _act_range_check(x, rng, "actquant_static_bwd")
    if g.shape != x.shape or drange.numel() != 2 * Cc:
        raise ValueError(f"actquant_static_bwd: g {tuple(g.shape)} / drange [{drange.numel()}] do not match x {tuple(x.shape)}")
    dx = torch.empty_like(x) if dx is None else dx
    need = int(L.lib().rdo_actquant_static_bwd_workspace(Cc))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=x.device, dtype=torch.float32)
    L.check(L.lib().rdo_actquant_static_bwd(_ptr(x), _ptr(g), npix, Cc, int(n_bits), _ptr(rng), _ptr(dx), _ptr(drange), _ptr(ws), _stream()),
            "rdo_actquant_static_bwd")
    return dx


def act_range_step(rng, grad, obs, m, v, step, lr):
    """One projected Adam step on a site's range [2C] (in place; m, v [2C] are its moments, `step` counts from 1, `obs` [2C] is the
    observed max range the step size is relative to and the range stays inside)."""
    n = rng.numel()
    if n % 2 or any(t.numel() != n for t in (grad, obs, m, v)):
        raise ValueError(f"act_range_step: range, grad, obs, m and v must all hold 2C = {n} floats")
    L.check(L.lib().rdo_act_range_step(_ptr(rng), _ptr(grad), _ptr(obs), _ptr(m), _ptr(v), n // 2, int(step), float(lr), _stream()),
            "rdo_act_range_step")
    return rng


ACT_HIST_BINS = 1024              # kAqhBins of csrc/actquant.hip (rdo_actquant_hist_bins)


def act_hist_init(channels, device):
    """Empty per-channel histogram [C, 1024] (int32)."""
    return torch.zeros(int(channels), ACT_HIST_BINS, device=device, dtype=torch.int32)


def actquant_hist(x, rng, hist):
    """hist [C, 1024] (int32) += the per-channel counts of x [..., C] on the observed range rng = lo[C] | hi[C] (the bin rule of
    include/rdo_ptq_hip.h).  The caller keeps a channel's total below 2^31."""
    Cc, npix = _act_range_check(x, rng, "actquant_hist")
    A.tensor("actquant_hist", "hist", hist, torch.int32, "int32", shape=(Cc, ACT_HIST_BINS), contiguous=True, oneshot=True)
    L.check(L.lib().rdo_actquant_hist(_ptr(x), npix, Cc, _ptr(rng), _ptr(hist), _stream()), "rdo_actquant_hist")
    return hist


def _hist_operands(what, hist, rng):
    """-> C of a contiguous int32 histogram [C, 1024] whose range holds 2C floats"""
    Cc = hist.shape[0]
    A.tensor(what, "hist", hist, torch.int32, "int32", shape=(Cc, ACT_HIST_BINS), contiguous=True, oneshot=True)
    if rng.numel() != 2 * Cc:
        raise ValueError(f"{what}: the range holds {rng.numel()} floats, the histogram has {Cc} channels: not [2C]")
    return Cc


def act_percentile_select(hist, rng, tail):
    """-> a new range [2C]: every channel's observed range rng with whole bins dropped from each end while the dropped count stays within
    floor(tail * n) (tail = 1 - p / 100; 0 returns rng bit for bit)."""
    Cc = _hist_operands("act_percentile_select", hist, rng)
    out = torch.empty_like(rng)
    L.check(L.lib().rdo_act_percentile_select(_ptr(hist), Cc, _ptr(rng), float(tail), _ptr(out), _stream()), "rdo_act_percentile_select")
    return out


def act_hist_mse_select(hist, rng, n_bits, score=False):
    """-> a new range [2C]: every channel's observed range rng with the whole bins dropped from each end that minimise the modelled
    squared quantisation error on a grid of n_bits (exhaustive search over all clip pairs: the rule of include/rdo_ptq_hip.h).
    `score`: -> (range, float64 [C, 2] = S of the choice | S(0, 0); 0 | 0 for a channel that kept its range)."""
    Cc = _hist_operands("act_hist_mse_select", hist, rng)
    n_bits = A.whole("act_hist_mse_select", "n_bits", n_bits, 2, 16)
    out = torch.empty_like(rng)
    hp, rp, op = _ptr(hist), _ptr(rng), _ptr(out)
    sc = torch.empty(Cc, 2, device=rng.device, dtype=torch.float64) if score else None     # (made on rng's device once _ptr has accepted the others)
    L.check(L.lib().rdo_act_hist_mse_select(hp, Cc, rp, n_bits, op, _ptr64(sc), _stream()), "rdo_act_hist_mse_select")
    return (out, sc) if score else out


def gather_qdrop(cache_q, cache_fp, idx_table, iter_ptr, B, prob, seed, out, batch_offset=0, iter_publish=None):
    """`batch_offset`: row of the global mini-batch this (data-parallel) rank's first row is -- the QDrop counter runs over the
    global batch, so N ranks with one seed draw the mask a single process would."""
    per_image = cache_q[0].numel()
    L.check(L.lib().rdo_gather_qdrop(_ptr(cache_q), _ptr(cache_fp), _ptr(idx_table), _ptr(iter_ptr), B, int(batch_offset), per_image,
                                     prob, seed,
                                     _ptr(out), _ptr(iter_publish), _stream()), "rdo_gather_qdrop")
    return out


def lp2_loss_grad(pred, tgt_cache, idx_table, iter_ptr, coef, grad, loss_log):
    B = pred.shape[0]
    per_image = pred[0].numel()
    L.check(L.lib().rdo_lp2_loss_grad(_ptr(pred), _ptr(tgt_cache), _ptr(idx_table), _ptr(iter_ptr), B, per_image,
                                      pred.shape[-1], coef, _ptr(grad), _ptr(loss_log), _stream()), "rdo_lp2_loss_grad")
    return grad


def lp_loss_grad(pred, tgt_cache, idx_table, iter_ptr, coef2, coefp, p, grad, loss_log, loss_log_p=None):
    """coef2 * lp_loss(., p=2) + coefp * lp_loss(., p=p) of the same (pred, tgt) pair, and its gradient.  With `loss_log_p`
    the |d|^p term is logged there and only the p = 2 term in `loss_log`."""
    B = pred.shape[0]
    per_image = pred[0].numel()
    L.check(L.lib().rdo_lp_loss_grad(_ptr(pred), _ptr(tgt_cache), _ptr(idx_table), _ptr(iter_ptr), B, per_image,
                                     pred.shape[-1], coef2, coefp, p, _ptr(grad), _ptr(loss_log), _ptr(loss_log_p), _stream()),
            "rdo_lp_loss_grad")
    return grad


def lrelu(x, out=None):
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().rdo_lrelu_fwd(_ptr(x), x.numel(), _ptr(out), _stream()), "rdo_lrelu_fwd")
    return out


def lrelu_bwd(g, y, out=None):
    out = torch.empty_like(g) if out is None else out
    L.check(L.lib().rdo_lrelu_bwd(_ptr(g), _ptr(y), g.numel(), _ptr(out), _stream()), "rdo_lrelu_bwd")
    return out


def relu(x, out=None):
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().rdo_relu_fwd(_ptr(x), x.numel(), _ptr(out), _stream()), "rdo_relu_fwd")
    return out


def relu_bwd(g, y, out=None):
    out = torch.empty_like(g) if out is None else out
    L.check(L.lib().rdo_relu_bwd(_ptr(g), _ptr(y), g.numel(), _ptr(out), _stream()), "rdo_relu_bwd")
    return out


def add(a, b, out=None):
    out = torch.empty_like(a) if out is None else out
    L.check(L.lib().rdo_add(_ptr(a), _ptr(b), a.numel(), _ptr(out), _stream()), "rdo_add")
    return out


def pixel_shuffle(x, r, out=None):
    """[B,H,W,C*r*r] -> [B,H*r,W*r,C]"""
    B, H, W, CC = x.shape
    Cc = CC // (r * r)
    out = torch.empty((B, H * r, W * r, Cc), device=x.device, dtype=torch.float32) if out is None else out
    L.check(L.lib().rdo_pixel_shuffle(_ptr(x), B, H, W, Cc, r, 0, _ptr(out), _stream()), "rdo_pixel_shuffle")
    return out


def pixel_unshuffle(x, r, out=None):
    """[B,H*r,W*r,C] -> [B,H,W,C*r*r]  (gradient of pixel_shuffle)"""
    B, Hr, Wr, Cc = x.shape
    H, W = Hr // r, Wr // r
    out = torch.empty((B, H, W, Cc * r * r), device=x.device, dtype=torch.float32) if out is None else out
    L.check(L.lib().rdo_pixel_shuffle(_ptr(x), B, H, W, Cc, r, 1, _ptr(out), _stream()), "rdo_pixel_shuffle(inverse)")
    return out


def gdn_bwd_t(g, x, norm, inverse, out=None):
    out = torch.empty_like(g) if out is None else out
    L.check(L.lib().rdo_gdn_bwd_t(_ptr(g), _ptr(x), _ptr(norm), g.numel(), int(inverse), _ptr(out), _stream()), "rdo_gdn_bwd_t")
    return out


def gdn_bwd_dx(g, x, norm, acc, inverse, out=None):
    out = torch.empty_like(g) if out is None else out
    L.check(L.lib().rdo_gdn_bwd_dx(_ptr(g), _ptr(x), _ptr(norm), _ptr(acc), g.numel(), int(inverse), _ptr(out), _stream()),
            "rdo_gdn_bwd_dx")
    return out


def nchw_to_nhwc(x, out=None):
    B, Cc, H, W = x.shape
    out = torch.empty((B, H, W, Cc), device=x.device, dtype=torch.float32) if out is None else out
    L.check(L.lib().rdo_nchw_to_nhwc(_ptr(x), B, Cc, H, W, 0, _ptr(out), _stream()), "rdo_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x, out=None):
    B, H, W, Cc = x.shape
    out = torch.empty((B, Cc, H, W), device=x.device, dtype=torch.float32) if out is None else out
    L.check(L.lib().rdo_nchw_to_nhwc(_ptr(x), B, Cc, H, W, 1, _ptr(out), _stream()), "rdo_nchw_to_nhwc(inverse)")
    return out


def zero_insert(x, stride, pad_top, pad_left, Ho, Wo, out=None):
    """[B,H,W,C] -> [B,Ho,Wo,C] with x placed at (pad + h*stride, pad + w*stride) and zeros elsewhere."""
    B, H, W, Cc = x.shape
    out = torch.empty((B, Ho, Wo, Cc), device=x.device, dtype=torch.float32) if out is None else out
    L.check(L.lib().rdo_zero_insert(_ptr(x), B, H, W, Cc, stride, pad_top, pad_left, Ho, Wo, _ptr(out), _stream()), "rdo_zero_insert")
    return out


class TconvPhase:
    """Sub-pixel form of ConvTranspose2d(K, stride, pad) with output = stride x input (include/rdo_ptq_hip.h, rdo_tconv_expand): the
    window size / padding of the equivalent stride-1 conv and the device index tables between the kernel-layout weight
    [Cout][K][K][Cin] (`flipped`: taps stored as [K-1-kh][K-1-kw], the engine's layout; else as they lie in the module's weight) and
    the phase weight [Cout * s^2][Kp][Kp][Cin]."""
    _cache = {}

    def __init__(self, K, stride, pad, flipped, device):
        s = stride
        win = []                                   # per phase a: [(d, kh)] input offset d and tap kh
        for a in range(s):
            r, q = (a + pad) % s, (a + pad) // s
            win.append([(q - t, r + s * t) for t in range((K - r + s - 1) // s) if r + s * t < K])
        dmax = max(max(d for d, _ in w) for w in win if w)
        dmin = min(min(d for d, _ in w) for w in win if w)
        self.pad = max(dmax, -dmin, 0)
        self.Kp = 2 * self.pad + 1
        self.S2, self.K, self.stride = s * s, K, s
        fl = (lambda k: K - 1 - k) if flipped else (lambda k: k)
        mp = [[-1] * (self.Kp * self.Kp) for _ in range(self.S2)]
        inv = [-1] * (K * K)
        for a in range(s):
            for b in range(s):
                for dh, kh in win[a]:
                    for dw, kw in win[b]:
                        u, v = dh + self.pad, dw + self.pad
                        tap = fl(kh) * K + fl(kw)
                        mp[a * s + b][u * self.Kp + v] = tap
                        inv[tap] = (a * s + b) * self.Kp * self.Kp + u * self.Kp + v
        assert all(i >= 0 for i in inv)
        self.map = torch.tensor(mp, dtype=torch.int32, device=device).contiguous()
        self.inv = torch.tensor(inv, dtype=torch.int32, device=device).contiguous()

    @classmethod
    def get(cls, K, stride, pad, output_padding, flipped, device):
        """The phase form, or None when the geometry has none (output must be exactly stride x input)."""
        if output_padding != stride + 2 * pad - K or stride < 2:
            return None
        key = (K, stride, pad, bool(flipped), str(device))
        if key not in cls._cache:
            cls._cache[key] = cls(K, stride, pad, flipped, device)
        return cls._cache[key]

    def w_shape(self, Cout, Cin):
        return (Cout * self.S2, self.Kp, self.Kp, Cin)


def tconv_expand(w_rows, ph, out=None):
    """kernel-layout weight [Cout][K][K][Cin] -> phase weight [Cout * s^2][Kp][Kp][Cin] (structural zeros included)."""
    Cout, K, _, Cin = w_rows.shape
    out = torch.empty(ph.w_shape(Cout, Cin), device=w_rows.device, dtype=torch.float32) if out is None else out
    L.check(L.lib().rdo_tconv_expand(_ptr(w_rows), _ptr(ph.map), Cout, K * K, Cin, ph.S2, ph.Kp * ph.Kp, _ptr(out), _stream()), "rdo_tconv_expand")
    return out


def tconv_fold(slabs_phase, ph, Cout, Cin, out=None):
    """gradient slabs [ns][Cout * s^2][Kp][Kp][Cin] of the phase weight -> slabs [ns][Cout][K][K][Cin] of the kernel weight"""
    ns = slabs_phase.shape[0]
    out = torch.empty((ns, Cout, ph.K, ph.K, Cin), device=slabs_phase.device, dtype=torch.float32) if out is None else out
    L.check(L.lib().rdo_tconv_fold(_ptr(slabs_phase), _ptr(ph.inv), ns, Cout, ph.K * ph.K, Cin, ph.S2, ph.Kp * ph.Kp, _ptr(out), _stream()),
            "rdo_tconv_fold")
    return out


class WeightPack:
    """Constant tensors derived from ONE weight in kernel layout (`w` = [Cout,KH,KW,Cin] rows), each built on first use and kept:
    the bf16x3 planes the split-precision MFMA forward reads, the flipped / transposed forms the input-gradient convolutions read
    (with their planes), the phase weight of a transposed conv.  The callers that hold a pack (QuantModule, hipops.autograd) own
    its validity: a pack is made for one value of the weight and dropped when that value changes."""

    def __init__(self, w_rows, bias=None):
        self.w = w_rows.detach().contiguous()
        self.bias = None if bias is None else bias.detach().contiguous()
        self._d = {}

    def get(self, key, make):
        v = self._d.get(key)
        if v is None:
            v = self._d[key] = make()
        return v

    def planes(self, x_shape, stride, pad):
        """bf16x3 planes of `w` when rdo_conv2d_fwd takes the split-precision path for this problem, else None."""
        if not uses_bf16x6(tuple(x_shape), tuple(self.w.shape), stride, pad):
            return None
        return self.get("planes", lambda: split_bf16x3(self.w))

    def flipped(self):
        """Pack of the stride-1 input-gradient weight [Cin][KH'][KW'][Cout] (taps flipped)."""
        return self.get("flipped", lambda: WeightPack(self.w.flip(1, 2).permute(3, 1, 2, 0)))

    def transposed(self):
        """Pack of `w` read with input and output channels exchanged, [Cin][KH][KW][Cout] (taps as they lie)."""
        return self.get("transposed", lambda: WeightPack(self.w.permute(3, 1, 2, 0)))

    def lin_planes(self, transposed=False):
        """Fragment-ordered fp16 planes of a Linear's weight [N, 1, 1, K] (or of its transpose: the input-gradient Linear) for
        rdo_linear_h2; the power-of-two scale comes from the weight's own magnitude (a synchronising reduction, once per pack)."""
        def make():
            w2 = self.w.reshape(self.w.shape[0], -1)
            return split_h2_linear(w2.t().contiguous() if transposed else w2)
        return self.get(("lin", bool(transposed)), make)

    def phase(self, ph):
        """(pack of the phase weight, phase bias) of the transposed conv with this weight as `to_rows(W, tconv=True)`."""
        def make():
            wp = tconv_expand(self.w, ph)
            return WeightPack(wp, None if self.bias is None else self.bias.repeat_interleave(ph.S2))
        return self.get(("phase", id(ph)), make)


def conv2d_fwd_pack(x, pack, stride=1, pad=0, bias=True, **kw):
    """conv2d_fwd with the weight, bias and (where the split-precision path applies) the weight planes of a WeightPack."""
    return conv2d_fwd(x, pack.w, pack.bias if bias else None, stride, pad, wplanes=pack.planes(x.shape, stride, pad), **kw)


def conv_transpose2d(x, w_iohw_rows, bias, stride, pad, output_padding, epilogue=L.EPI_NONE, pack=None):
    """x [B,H,W,Cin]; w_iohw_rows = to_rows(W, tconv=True) = [Cout,KH,KW,Cin] (un-flipped taps of the [Cin,Cout,KH,KW] weight), or
    `pack` = a WeightPack of it (weight-derived tensors are then built once).  Output = stride x input (the deconv of the LIC
    decoders): stride-1 conv with the phase weight + pixel shuffle, no zero insertion; other geometries: zero insertion + dense conv.
    `output_padding`: one int for both axes or an (h, w) pair (the input gradient of a strided conv whose height and width leave
    different remainders); the phase form needs output = stride x input on both."""
    if pack is None:
        pack = WeightPack(w_iohw_rows, bias)
    Cout, KH, KW, Cin = pack.w.shape
    B, H, W, _ = x.shape
    oph, opw = (int(v) for v in output_padding) if isinstance(output_padding, (tuple, list)) else (int(output_padding),) * 2
    ph = TconvPhase.get(KH, stride, pad, oph, False, x.device) if KH == KW and oph == opw else None
    if ph is not None:
        # LeakyReLU / ReLU commute with the pixel shuffle; large problems on the split-precision path
        yp = conv2d_fwd_pack(x, pack.phase(ph), 1, ph.pad, epilogue=epilogue)
        return pixel_shuffle(yp, stride)
    q = KH - 1 - pad
    if q < 0:
        raise ValueError("conv_transpose2d: padding larger than kernel_size - 1 is not supported")
    Hup, Wup = (H - 1) * stride + 1 + 2 * q + oph, (W - 1) * stride + 1 + 2 * q + opw
    xu = zero_insert(x, stride, q, q, Hup, Wup)
    return conv2d_fwd_pack(xu, pack.get("zi", lambda: WeightPack(pack.w.flip(1, 2), pack.bias)), 1, 0, epilogue=epilogue)


def _ln_operands(what, x, weight, bias=None, same=(), slabs=None, max_c=None, vec=False):
    """-> (rows, C, nslabs) of a LayerNorm call on x [..., C]: weight / bias [C] (or None), every tensor of `same` of x's shape (or None),
    `slabs` [n >= 1, C]; all of them non-empty fp32 tensors on x's device"""
    A.tensor(what, "x", x)
    if x.dim() < 1:
        raise ValueError(f"{what}: x must be [..., C], got a scalar")
    Cc = x.shape[-1]
    if max_c is not None and Cc > max_c:
        raise ValueError(f"{what}: C = {Cc} channels, at most {max_c} are supported")
    if vec and Cc % 4:
        raise ValueError(f"{what}: C = {Cc} must be a multiple of 4")
    A.tensor(what, "weight", weight, device=x.device, shape=(Cc,), optional=True)
    A.tensor(what, "bias", bias, device=x.device, shape=(Cc,), optional=True)
    for name, t in same:
        A.tensor(what, name, t, device=x.device, shape=x.shape, optional=True)
    ns = 0
    if slabs is not None:
        A.tensor(what, "dgamma_slabs", slabs, device=x.device)
        if slabs.dim() != 2 or slabs.shape[1] != Cc:
            raise ValueError(f"{what}: dgamma_slabs must be [n >= 1, {Cc}], got {tuple(slabs.shape)}")
        ns = slabs.shape[0]
    return x.numel() // Cc, Cc, ns


def layer_norm(x, weight, bias, eps=1e-5, out=None):
    rows, Cc, _ = _ln_operands("layer_norm", x, weight, bias, same=(("out", out),))
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().rdo_layer_norm(_ptr(x), _ptr(weight), _ptr(bias), rows, Cc, eps, _ptr(out), _stream()),
            "rdo_layer_norm")
    return out


def linear_h2_supported(rows, cin, cout):
    return bool(L.lib().rdo_linear_h2_supported(int(rows), int(cin), int(cout)))


def split_h2_linear(w, scale=None, planes=None):
    """W [N][K] (any shape whose first dim is N, rest flattened to K) -> H2 planes in the fragment order of rdo_linear_h2; the scale
    defaults to a power of two that puts max |W| at 2^7 (a device synchronisation: set-up only -- pass `scale` inside recorded plans)."""
    N = w.shape[0]
    K = w.numel() // N
    if scale is None:
        scale = pow2_scale(w.abs().max())
    if planes is None:
        planes = H2(torch.empty((2, K // 32, N // 16, 64, 8), device=w.device, dtype=torch.int16), scale)
    L.check(L.lib().rdo_split_h2_linear(_ptr(w), N, K, float(planes.scale), _ptr(planes), _stream()), "rdo_split_h2_linear")
    return planes


def linear_h2(x, planes, bias=None, out=None, square_input=False, epilogue=L.EPI_NONE, pre=None, aux=None):
    """out [rows, N] = x [rows, K] W^T + bias (x^2 instead of x with `square_input`: the GDN norm pool) on the per-token-scaled
    fp16-split kernel; `planes` from split_h2_linear.  epilogue: EPI_GELU (out = gelu(y), `pre` receives y) or EPI_GELU_BWD
    (out = y * gelu'(aux))."""
    K = x.shape[-1]
    rows = x.numel() // K
    N = planes.t.shape[2] * 16
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (N,), device=x.device, dtype=torch.float32)
    if epilogue == L.EPI_NONE:
        L.check(L.lib().rdo_linear_h2(_ptr(x), rows, K, N, _ptr(planes), float(planes.scale), _ptr(bias), int(bool(square_input)), _ptr(out), _stream()),
                "rdo_linear_h2")
    else:
        L.check(L.lib().rdo_linear_h2_epi(_ptr(x), rows, K, N, _ptr(planes), float(planes.scale), _ptr(bias), int(bool(square_input)), int(epilogue),
                                          _ptr(pre), _ptr(aux), _ptr(out), _stream()), "rdo_linear_h2_epi")
    return out


def add_layer_norm(a, b, weight, bias, eps=1e-5, sum_out=None, out=None):
    """s = a + b (b may be None) -> `sum_out` (written when given), LayerNorm(s) -> out: the residual add of a Swin block and the
    LayerNorm that reads it, in one pass."""
    rows, Cc, _ = _ln_operands("add_layer_norm", a, weight, bias, same=(("b", b), ("sum_out", sum_out), ("out", out)), max_c=512, vec=True)
    if sum_out is not None and b is None:
        raise ValueError("add_layer_norm: sum_out without a second addend b")
    out = torch.empty_like(a) if out is None else out
    L.check(L.lib().rdo_add_layer_norm(_ptr(a), _ptr(b), _ptr(weight), _ptr(bias), rows, Cc, eps, _ptr(sum_out), _ptr(out),
                                       _stream()), "rdo_add_layer_norm")
    return out


def layer_norm_bwd_add(x, weight, dy, add1=None, add2=None, eps=1e-5, dx=None, dgamma_slabs=None):
    """dx = (add1) (+ add2) + LayerNorm-backward(dy); dgamma partial sums as in `layer_norm_bwd`."""
    what = "layer_norm_bwd_add"
    A.tensor(what, "dy", dy)
    rows, Cc, ns = _ln_operands(what, x, weight, same=(("dy", dy), ("add1", add1), ("add2", add2), ("dx", dx)), slabs=dgamma_slabs,
                                max_c=512, vec=True)
    if add2 is not None and add1 is None:
        raise ValueError(f"{what}: add2 without add1")
    if add1 is not None and dx is None:
        raise ValueError(f"{what}: an addend without dx")
    if dx is None and dgamma_slabs is None:
        raise ValueError(f"{what}: nothing to compute (neither dx nor dgamma_slabs)")
    L.check(L.lib().rdo_layer_norm_bwd_add(_ptr(x), _ptr(weight), _ptr(dy), _ptr(add1), _ptr(add2), rows, Cc, eps, _ptr(dx),
                                           _ptr(dgamma_slabs), ns, _stream()), "rdo_layer_norm_bwd_add")
    return dx


def add3(a, b, c, out=None):
    """(a + b) + c"""
    A.tensor("add3", "a", a)
    for name, t in (("b", b), ("c", c)):
        A.tensor("add3", name, t, device=a.device, numel=a.numel())
    A.tensor("add3", "out", out, device=a.device, numel=a.numel(), optional=True)
    if a.numel() % 4:
        raise ValueError(f"add3: {a.numel()} elements, the count must be a multiple of 4")
    out = torch.empty_like(a) if out is None else out
    L.check(L.lib().rdo_add3(_ptr(a), _ptr(b), _ptr(c), a.numel(), _ptr(out), _stream()), "rdo_add3")
    return out


def layer_norm_bwd(x, weight, dy, eps=1e-5, dx=None, dgamma_slabs=None):
    """dx (returned) and, when `dgamma_slabs` [nslabs, C] is given, the partial sums of dy * xhat."""
    what = "layer_norm_bwd"
    A.tensor(what, "dy", dy)
    rows, Cc, ns = _ln_operands(what, x, weight, same=(("dy", dy), ("dx", dx)), slabs=dgamma_slabs, max_c=512)
    if dx is None and dgamma_slabs is None:
        raise ValueError(f"{what}: nothing to compute (neither dx nor dgamma_slabs)")
    L.check(L.lib().rdo_layer_norm_bwd(_ptr(x), _ptr(weight), _ptr(dy), rows, Cc, eps, _ptr(dx), _ptr(dgamma_slabs), ns,
                                       _stream()), "rdo_layer_norm_bwd")
    return dx


def attn_desc(B, H, W, Cc, heads, window, shift, scale=None):
    return L.AttnDesc(B, H, W, Cc, heads, window, shift, float((Cc // heads) ** -0.5 if scale is None else scale))


def _attn_geometry(what, d):
    """-> (pixels, N, windows) of a descriptor the attention kernels accept (make_geom of csrc/swin.hip), ValueError otherwise"""
    if not isinstance(d, L.AttnDesc):
        raise ValueError(f"{what}: expected an attn_desc, got {type(d).__name__}")
    if min(d.B, d.H, d.W, d.C, d.heads, d.window) <= 0:
        raise ValueError(f"{what}: bad geometry B={d.B} H={d.H} W={d.W} C={d.C} heads={d.heads} window={d.window}")
    if d.C % d.heads:
        raise ValueError(f"{what}: C={d.C} is not divisible by heads={d.heads}")
    if d.H % d.window or d.W % d.window:
        raise ValueError(f"{what}: {d.H}x{d.W} is not divisible by window {d.window}")
    if d.window * d.window > 64:
        raise ValueError(f"{what}: windows of more than 64 tokens are not supported (window={d.window})")
    if d.C // d.heads > 64:
        raise ValueError(f"{what}: head dims above 64 are not supported (C={d.C}, heads={d.heads})")
    if not 0 <= d.shift < d.window:
        raise ValueError(f"{what}: shift={d.shift} must be in [0, window={d.window})")
    N = d.window * d.window
    return d.B * d.H * d.W, N, d.B * (d.H // d.window) * (d.W // d.window)


def window_attention(d, qkv, bias, out=None, probs=None, compute_out=True):
    """Fused (S)W-MSA core on [B, H, W, 3C] -> [B, H, W, C]; `probs` [windows, N, N, heads] is filled when given."""
    what = "window_attention"
    pixels, N, windows = _attn_geometry(what, d)
    A.tensor(what, "qkv", qkv, numel=pixels * 3 * d.C)
    A.tensor(what, "bias", bias, device=qkv.device, numel=d.heads * N * N)
    A.tensor(what, "probs", probs, device=qkv.device, numel=windows * N * N * d.heads, optional=True)
    if not compute_out and probs is None:
        raise ValueError(f"{what}: compute_out=False without probs leaves nothing to compute")
    if compute_out:
        A.tensor(what, "out", out, device=qkv.device, numel=pixels * d.C, optional=True)
        if out is None:
            out = torch.empty((d.B, d.H, d.W, d.C), device=qkv.device, dtype=torch.float32)
    L.check(L.lib().rdo_window_attention_fwd(C.byref(d), _ptr(qkv), _ptr(bias), _ptr(out) if compute_out else None, _ptr(probs),
                                             _stream()), "rdo_window_attention_fwd")
    return out


def window_attention_pv(d, qkv, probs, out=None):
    what = "window_attention_pv"
    pixels, N, windows = _attn_geometry(what, d)
    A.tensor(what, "qkv", qkv, numel=pixels * 3 * d.C)
    A.tensor(what, "probs", probs, device=qkv.device, numel=windows * N * N * d.heads)
    A.tensor(what, "out", out, device=qkv.device, numel=pixels * d.C, optional=True)
    out = torch.empty((d.B, d.H, d.W, d.C), device=qkv.device, dtype=torch.float32) if out is None else out
    L.check(L.lib().rdo_window_attention_pv(C.byref(d), _ptr(qkv), _ptr(probs), _ptr(out), _stream()), "rdo_window_attention_pv")
    return out


def window_attention_bwd(d, qkv, bias, dout, dqkv=None):
    what = "window_attention_bwd"
    pixels, N, windows = _attn_geometry(what, d)
    A.tensor(what, "qkv", qkv, numel=pixels * 3 * d.C)
    A.tensor(what, "bias", bias, device=qkv.device, numel=d.heads * N * N)
    A.tensor(what, "dout", dout, device=qkv.device, numel=pixels * d.C)
    A.tensor(what, "dqkv", dqkv, device=qkv.device, numel=qkv.numel(), optional=True)
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    L.check(L.lib().rdo_window_attention_bwd(C.byref(d), _ptr(qkv), _ptr(bias), _ptr(dout), _ptr(dqkv), _stream()),
            "rdo_window_attention_bwd")
    return dqkv


def window_attention_pv_bwd(d, qkv, probs_q, dout, dprobs=None, dqkv=None):
    """Backward of `window_attention_pv` from the probabilities it was given -> (dprobs [windows, N, N, heads], dqkv [B, H, W, 3C] with
    dV in its last third and zeros in the other two); every element of both is written."""
    what = "window_attention_pv_bwd"
    pixels, N, windows = _attn_geometry(what, d)
    A.tensor(what, "qkv", qkv, numel=pixels * 3 * d.C)
    A.tensor(what, "probs_q", probs_q, device=qkv.device, numel=windows * N * N * d.heads)
    A.tensor(what, "dout", dout, device=qkv.device, numel=pixels * d.C)
    A.tensor(what, "dprobs", dprobs, device=qkv.device, numel=probs_q.numel(), optional=True)
    A.tensor(what, "dqkv", dqkv, device=qkv.device, numel=qkv.numel(), optional=True)
    dprobs = torch.empty((windows, N, N, d.heads), device=qkv.device, dtype=torch.float32) if dprobs is None else dprobs
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    L.check(L.lib().rdo_window_attention_pv_bwd(C.byref(d), _ptr(qkv), _ptr(probs_q), _ptr(dout), _ptr(dprobs), _ptr(dqkv), _stream()),
            "rdo_window_attention_pv_bwd")
    return dprobs, dqkv


def window_attention_probs_bwd(d, qkv, probs, dprobs, dqkv=None):
    """Backward of the probabilities `window_attention(..., compute_out=False)` wrote, from those float32 values and their gradient ->
    dqkv [B, H, W, 3C] with dQ | dK in its first two thirds and zeros in the last; every element is written."""
    what = "window_attention_probs_bwd"
    pixels, N, windows = _attn_geometry(what, d)
    A.tensor(what, "qkv", qkv, numel=pixels * 3 * d.C)
    A.tensor(what, "probs", probs, device=qkv.device, numel=windows * N * N * d.heads)
    A.tensor(what, "dprobs", dprobs, device=qkv.device, numel=probs.numel())
    A.tensor(what, "dqkv", dqkv, device=qkv.device, numel=qkv.numel(), optional=True)
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    L.check(L.lib().rdo_window_attention_probs_bwd(C.byref(d), _ptr(qkv), _ptr(probs), _ptr(dprobs), _ptr(dqkv), _stream()),
            "rdo_window_attention_probs_bwd")
    return dqkv


def gelu(x, out=None):
    A.tensor("gelu", "x", x)
    A.tensor("gelu", "out", out, device=x.device, numel=x.numel(), optional=True)
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().rdo_gelu_fwd(_ptr(x), x.numel(), _ptr(out), _stream()), "rdo_gelu_fwd")
    return out


def gelu_bwd(dy, x, dx=None):
    A.tensor("gelu_bwd", "x", x)
    A.tensor("gelu_bwd", "dy", dy, device=x.device, numel=x.numel())
    A.tensor("gelu_bwd", "dx", dx, device=x.device, numel=x.numel(), optional=True)
    dx = torch.empty_like(x) if dx is None else dx
    L.check(L.lib().rdo_gelu_bwd(_ptr(dy), _ptr(x), x.numel(), _ptr(dx), _stream()), "rdo_gelu_bwd")
    return dx


def round_(x, out=None):
    A.tensor("round_", "x", x)
    A.tensor("round_", "out", out, device=x.device, numel=x.numel(), optional=True)
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().rdo_round(_ptr(x), x.numel(), _ptr(out), _stream()), "rdo_round")
    return out


def ssim_level(x, y, window, c1, c2):
    """x, y: [planes, H, W]; window: 11 Python floats -> (ssim_mean[planes], cs_mean[planes])."""
    planes, H, W = x.shape
    ssim = torch.empty(planes, device=x.device, dtype=torch.float32)
    cs = torch.empty(planes, device=x.device, dtype=torch.float32)
    win = (C.c_float * 11)(*[float(v) for v in window])
    L.check(L.lib().rdo_ssim_level(_ptr(x), _ptr(y), planes, H, W, win, c1, c2, _ptr(ssim), _ptr(cs), _stream()), "rdo_ssim_level")
    return ssim, cs


def avg_pool2(x):
    planes, H, W = x.shape
    ph, pw = H % 2, W % 2
    out = torch.empty((planes, (H + 2 * ph - 2) // 2 + 1, (W + 2 * pw - 2) // 2 + 1), device=x.device, dtype=torch.float32)
    L.check(L.lib().rdo_avg_pool2(_ptr(x), planes, H, W, _ptr(out), _stream()), "rdo_avg_pool2")
    return out


def ssim_level_bwd(x, y, window, c1, c2, g_ssim, g_cs, dx=None):
    """Gradient with respect to x of sum(g_ssim * ssim_mean + g_cs * cs_mean) of `ssim_level(x, y, window, c1, c2)`; g_ssim, g_cs: [planes]
    on the device -> dx [planes, H, W]."""
    planes, H, W = x.shape
    if y.shape != x.shape or g_ssim.numel() != planes or g_cs.numel() != planes or (dx is not None and dx.shape != x.shape):
        raise ValueError("ssim_level_bwd: x, y (and dx) must share one [planes, H, W] shape, g_ssim / g_cs hold one value per plane")
    dx = torch.empty_like(x) if dx is None else dx
    win = (C.c_float * 11)(*[float(v) for v in window])
    L.check(L.lib().rdo_ssim_level_bwd(_ptr(x), _ptr(y), planes, H, W, win, c1, c2, _ptr(g_ssim), _ptr(g_cs), _ptr(dx), _stream()),
            "rdo_ssim_level_bwd")
    return dx


def avg_pool2_bwd(g_out, H, W):
    """Adjoint of `avg_pool2` on a [planes, H, W] input: g_out [planes, Ho, Wo] -> dx [planes, H, W]."""
    planes = g_out.shape[0]
    ph, pw = H % 2, W % 2
    if tuple(g_out.shape[1:]) != ((H + 2 * ph - 2) // 2 + 1, (W + 2 * pw - 2) // 2 + 1):
        raise ValueError(f"avg_pool2_bwd: gradient {tuple(g_out.shape)} does not match a {H}x{W} input")
    dx = torch.empty((planes, H, W), device=g_out.device, dtype=torch.float32)
    L.check(L.lib().rdo_avg_pool2_bwd(_ptr(g_out), planes, H, W, _ptr(dx), _stream()), "rdo_avg_pool2_bwd")
    return dx


def iter_advance(iter_ptr):
    L.check(L.lib().rdo_iter_advance(_ptr(iter_ptr), _stream()), "rdo_iter_advance")


def _fp32_operands(what, optional=(), **named):
    """The entropy / rate kernels index every operand by the first one's element count: refuse, before any pointer is taken, an operand
    that is not a non-empty fp32 tensor of that count on the same device (the operands named in `optional` may be None).  -> the count"""
    first = None
    for name, t in named.items():
        if first is None:
            A.tensor(what, name, t, optional=name in optional)
            first = None if t is None else (name, t)
        else:
            A.tensor(what, name, t, device=first[1].device, other=first[0], numel=first[1].numel(), optional=name in optional)
    return first[1].numel()


def _eb_operands(what, z, params, medians=False):
    """-> C of a channels-last z [..., C] whose params are [C, 58] (and medians [C]) fp32 on z's device"""
    _fp32_operands(what, z=z)
    if z.dim() < 1:
        raise ValueError(f"{what}: z must be channels-last [..., C], got a scalar")
    Cc = z.shape[-1]
    A.tensor(what, "params", params, shape=(Cc, 58), device=z.device, oneshot=True)
    if medians is not False:
        A.tensor(what, "medians", medians, shape=(Cc,), device=z.device, oneshot=True)
    return Cc


def _sum_out(what, ref, out):
    """the accumulator of a rate / distortion sum: one fp32 element on the operands' device (made zero when None)"""
    A.tensor(what, "out", out, numel=1, device=ref.device, optional=True, oneshot=True)
    return torch.zeros(1, device=ref.device, dtype=torch.float32) if out is None else out


def factorized_likelihood(z_cl, params, medians):
    """z_cl: [..., C] channels-last.  -> (z_hat, likelihood)"""
    Cc = _eb_operands("factorized_likelihood", z_cl, params, medians)
    zhat, lik = torch.empty_like(z_cl), torch.empty_like(z_cl)
    L.check(L.lib().rdo_factorized_likelihood_fwd(_ptr(z_cl), _ptr(params), _ptr(medians), z_cl.numel(), Cc, _ptr(zhat),
                                                  _ptr(lik), _stream()), "rdo_factorized_likelihood_fwd")
    return zhat, lik


def factorized_likelihood_bwd(zhat_cl, params, grad_scale=1.0):
    """d(grad_scale * sum(-log2 p)) / dz^ of the factorised prior, element-wise (z^ channels-last)"""
    Cc = _eb_operands("factorized_likelihood_bwd", zhat_cl, params)
    dz = torch.empty_like(zhat_cl)
    L.check(L.lib().rdo_factorized_likelihood_bwd(_ptr(zhat_cl), _ptr(params), zhat_cl.numel(), Cc, grad_scale, _ptr(dz), _stream()),
            "rdo_factorized_likelihood_bwd")
    return dz


def gaussian_likelihood(y, scales, means=None, scale_bound=0.11):
    n = _fp32_operands("gaussian_likelihood", ("means",), y=y, scales=scales, means=means)
    yhat, lik = torch.empty_like(y), torch.empty_like(y)
    L.check(L.lib().rdo_gaussian_likelihood_fwd(_ptr(y), _ptr(scales), _ptr(means), n, scale_bound, _ptr(yhat), _ptr(lik),
                                                _stream()), "rdo_gaussian_likelihood_fwd")
    return yhat, lik


def gaussian_likelihood_bwd(yhat, scales, means, grad_scale=1.0, scale_bound=0.11):
    n = _fp32_operands("gaussian_likelihood_bwd", ("means",), yhat=yhat, scales=scales, means=means)
    ds, dm = torch.empty_like(scales), torch.empty_like(scales)
    L.check(L.lib().rdo_gaussian_likelihood_bwd(_ptr(yhat), _ptr(scales), _ptr(means), n, scale_bound, grad_scale,
                                                _ptr(ds), _ptr(dm), _stream()), "rdo_gaussian_likelihood_bwd")
    return ds, dm


def neg_log2_sum(lik, scale=1.0, out=None):
    n = _fp32_operands("neg_log2_sum", lik=lik)
    out = _sum_out("neg_log2_sum", lik, out)
    L.check(L.lib().rdo_neg_log2_sum(_ptr(lik), n, scale, _ptr(out), _stream()), "rdo_neg_log2_sum")
    return out


def sq_diff_sum(a, b, scale=1.0, clamp01=False, out=None):
    n = _fp32_operands("sq_diff_sum", a=a, b=b)
    out = _sum_out("sq_diff_sum", a, out)
    L.check(L.lib().rdo_sq_diff_sum(_ptr(a), _ptr(b), n, scale, int(clamp01), _ptr(out), _stream()), "rdo_sq_diff_sum")
    return out


def _ordered_ws(device):
    """the workspace the two ordered sums share"""
    return _workspace("ordered_sum", device, int(L.lib().rdo_ordered_sum_workspace()))


def neg_log2_sum_ordered(lik, scale=1.0, out=None):
    """`neg_log2_sum` summed in a fixed order: the same bits on every run (evaluation)."""
    n = _fp32_operands("neg_log2_sum_ordered", lik=lik)
    out = _sum_out("neg_log2_sum_ordered", lik, out)
    L.check(L.lib().rdo_neg_log2_sum_ordered(_ptr(lik), n, scale, _ptr(out), _ptr(_ordered_ws(lik.device)), _stream()),
            "rdo_neg_log2_sum_ordered")
    return out


def sq_diff_sum_ordered(a, b, scale=1.0, clamp01=False, out=None):
    """`sq_diff_sum` summed in a fixed order: the same bits on every run (evaluation)."""
    n = _fp32_operands("sq_diff_sum_ordered", a=a, b=b)
    out = _sum_out("sq_diff_sum_ordered", a, out)
    L.check(L.lib().rdo_sq_diff_sum_ordered(_ptr(a), _ptr(b), n, scale, int(clamp01), _ptr(out), _ptr(_ordered_ws(a.device)),
                                            _stream()), "rdo_sq_diff_sum_ordered")
    return out


def neg_log2_channel_sums(lik, out=None):
    """Per-channel rate of a 4-D fp32 likelihood tensor [B, C, H, W] on the GPU: -> float32 [C], out[c] = sum over b, h, w of -log2 lik,
    in one read and a fixed summation order (the same input gives the same bits; a NaN stays in its channel).  NCHW-contiguous and
    channels-last-contiguous storage are read as they are (outer, inner = B, H W or B H W, 1); anything else is made contiguous first.
    `out`: a contiguous fp32 [C] on lik's device that is OVERWRITTEN.  Everything is checked on the host before a pointer is taken."""
    what = "neg_log2_channel_sums"
    A.tensor(what, "lik", lik, rank=4, layout="4-D [B, C, H, W]")
    B, Cc, H, W = (int(v) for v in lik.shape)
    A.tensor(what, "out", out, shape=(Cc,), contiguous=True, device=lik.device, optional=True, oneshot=True)
    if not lik.is_cuda:
        raise ValueError(f"{what}: lik is on {lik.device}; there is no CPU path")
    if lik.is_contiguous():
        outer, inner = B, H * W
    elif lik.is_contiguous(memory_format=torch.channels_last):
        lik, outer, inner = lik.permute(0, 2, 3, 1), B * H * W, 1       # the same storage as a contiguous [B, H, W, C] view
    else:
        lik, outer, inner = lik.contiguous(), B, H * W
    if out is None:
        out = torch.empty(Cc, device=lik.device, dtype=torch.float32)
    n_ws = int(L.lib().rdo_neg_log2_channel_sums_workspace(outer, Cc, inner))
    if n_ws <= 0:
        raise ValueError(f"{what}: {tuple(lik.shape)} is beyond the kernel's index arithmetic (C <= 65535, B H W < 2^31)")
    ws = _workspace(what, lik.device, n_ws, torch.float32, n_ws)
    L.check(L.lib().rdo_neg_log2_channel_sums(_ptr(lik), outer, Cc, inner, _ptr(out), _ptr(ws), _stream()), "rdo_neg_log2_channel_sums")
    return out


_SCHED_MEMO = {}


def make_sched(iters, warmup, b_range, lr=1e-3, device="cuda"):
    """Per-iteration schedule table (rdo_sched_row): LinearTempDecay (utils.py:37-54), round-loss gate
    (layer_opt.py:159-161), Adam bias corrections.  Computed on the host in double precision, once per distinct schedule: every unit
    of a calibration run shares one (the Python loop over 20 000 iterations took 0.135 s per unit, 2.8 % of the full schedule)."""
    key = (int(iters), float(warmup), float(b_range[0]), float(b_range[1]), float(lr))
    rows = _SCHED_MEMO.get(key)
    if rows is None:
        if len(_SCHED_MEMO) >= 8:
            _SCHED_MEMO.clear()
        rows = _SCHED_MEMO[key] = _make_sched_rows(iters, warmup, b_range, lr)
    return rows.to(device)


def _make_sched_rows(iters, warmup, b_range, lr):
    import math
    rows = torch.empty((iters, 4), dtype=torch.float32)
    t_max, start = iters, warmup * iters
    loss_start = iters * warmup
    for i in range(iters):
        count = i + 1
        if count < start:
            b = float(b_range[0])
        else:
            rel_t = (count - start) / (t_max - start)
            b = b_range[1] + (b_range[0] - b_range[1]) * max(0.0, 1 - rel_t)
        on = 0.0 if count < loss_start else 1.0
        if not on:
            b = 0.0
        rows[i, 0] = b
        rows[i, 1] = on
        rows[i, 2] = lr / (1 - 0.9 ** count)
        rows[i, 3] = math.sqrt(1 - 0.999 ** count)
    return rows


# ----------------------------------------------------------------------------- H2 tensors and fused unit tails
H2_TARGET = 128.0      # a tensor's scale puts its largest magnitude (as probed) near 2^7: x512 head-room to fp16's 65504, fp32-chain
                       # accuracy down to max |x s| = 2^-2 (tools/f16_probe.hip)


def pow2_scale(amax, target=H2_TARGET):
    """The power of two s with target / 2 < amax * s <= target (1.0 for an all-zero tensor)."""
    amax = float(amax)
    if not math.isfinite(amax):
        raise ValueError("pow2_scale: non-finite magnitude")
    if amax <= 0.0:
        return 1.0
    return 2.0 ** min(60, max(-60, math.floor(math.log2(target / amax))))


def h2_empty(shape, device, scale=1.0, flag=None):
    """Planes of an H2 tensor for an fp32 NHWC tensor of `shape` [..., C] (C % 16 == 0): int16 [2, C/16, pixels, 16] -- slice-major
    planes, include/rdo_ptq_hip.h."""
    Cc = shape[-1]
    if Cc % 16:
        raise ValueError(f"H2 tensors need a channel count that is a multiple of 16, got {Cc}")
    npix = 1
    for d in shape[:-1]:
        npix *= int(d)
    return H2(torch.empty((2, Cc // 16, npix, 16), device=device, dtype=torch.int16), scale, flag)


def h2_to_float(planes, shape):
    """(h1 + h2) / scale as an fp32 tensor of `shape` (the original values to 2^-24 relative)."""
    x = (planes.t[0].view(torch.float16).float() + planes.t[1].view(torch.float16).float()) / planes.scale      # [C/16, pixels, 16]
    return x.permute(1, 0, 2).reshape(shape).contiguous()


def h2_overflow(reset=True):
    """True when a producer of H2 planes raised the per-device default flag -- met a value outside fp16's range with no word of its own
    bound -- since the last reset (synchronises the device).  Words bound with `h2_flag` or carried by an output `H2` are the caller's to
    read: this neither reads nor resets them."""
    rc = int(L.lib().rdo_h2_overflow(int(bool(reset))))
    if rc < 0:
        raise RuntimeError("rdo_h2_overflow failed")
    return bool(rc)


class h2_flag:
    """with h2_flag(word): the H2 producers launched -- or recorded into a plan -- by this thread inside the block raise `word` (a
    zero-initialised int32 device tensor the caller keeps alive as long as the recorded plans) instead of the per-device default flag
    (rdo_h2_bind_flag).  An output `H2` that carries its own `.flag` raises that one instead (`_bind_out`).  A raised word holds the
    fp32 bit pattern of the largest FINITE |x * scale| that did not fit in word 0 (`overflow_magnitude`) and a non-finite mark in word 1.  Blocks nest; leaving restores the previous
    binding."""
    _tls = threading.local()          # rdo_h2_bind_flag is thread_local in the library (csrc/runtime.hip): so is this cache of it

    def __init__(self, word):
        if word is not None and not (word.is_cuda and word.dtype == torch.int32 and word.numel() >= 2):
            raise ValueError("h2_flag: expected an int32 CUDA tensor of two words (finite magnitude, non-finite mark)")
        self.word = word

    @staticmethod
    def _state():
        st = h2_flag._tls
        if not hasattr(st, "stack"):
            st.stack, st.bound = [], None
        return st

    @staticmethod
    def bind(word):
        st = h2_flag._state()
        if word is not st.bound:
            L.check(L.lib().rdo_h2_bind_flag(None if word is None else _ptr(word)), "rdo_h2_bind_flag")
            st.bound = word

    def __enter__(self):
        h2_flag._state().stack.append(self.word)
        h2_flag.bind(self.word)
        return self.word

    def __exit__(self, *exc):
        st = h2_flag._state()
        st.stack.pop()
        h2_flag.bind(st.stack[-1] if st.stack else None)
        return False


def _bind_out(planes):
    """the overflow word the next producer raises: the output tensor's own, else the enclosing h2_flag block's, else the default"""
    own = getattr(planes, "flag", None)
    st = h2_flag._state()
    h2_flag.bind(own if own is not None else (st.stack[-1] if st.stack else None))


def overflow_magnitude(word_value):
    """Largest |x * scale| a raised overflow word recorded (its int32 value is the fp32 bit pattern; inf for NaN / inf inputs)."""
    import struct
    v = struct.unpack("<f", struct.pack("<i", int(word_value)))[0]
    return float("inf") if not math.isfinite(v) else v


def split_h2(x, planes=None, scale=None):
    """fp32 NHWC tensor -> H2 planes; without `planes` / `scale` the scale comes from the tensor's own largest magnitude (a device
    synchronisation: set-up and tests only)."""
    if planes is None:
        planes = h2_empty(x.shape, x.device, pow2_scale(x.abs().max()) if scale is None else scale)
    Cc = x.shape[-1]
    _bind_out(planes)
    L.check(L.lib().rdo_split_h2(_ptr(x), x.numel() // Cc, Cc, planes.scale, _ptr(planes), _stream()), "rdo_split_h2")
    return planes


def split_h2_conv(w, planes=None, scale=None, row_groups=0):
    """Conv weight in kernel layout [Cout,KH,KW,Cin] (or [C,C] = 1x1) -> H2 weight planes int16 [2, Cout,KH,KW,Cin] in the fragment
    order the split-precision kernels read ([Cin/16][KH][KW][Cout][16]).  row_groups = 4: with the rows in 4 groups (logical row r at
    row (r & 3) Cout / 4 + (r >> 2): rdo_split_h2_conv_px, include/rdo_ptq_subpel.h)."""
    if w.dim() == 2:
        w = w.reshape(w.shape[0], 1, 1, w.shape[1])
    if w.dim() != 4:
        raise ValueError("split_h2_conv: expected a conv weight [Cout,KH,KW,Cin]")
    if planes is None:
        planes = H2(torch.empty((2,) + tuple(w.shape), device=w.device, dtype=torch.int16), pow2_scale(w.abs().max()) if scale is None else scale)
    co, kh, kw, ci = w.shape
    _bind_out(planes)
    if row_groups:
        L.check(L.lib().rdo_split_h2_conv_px(_ptr(w), co, kh, kw, ci, planes.scale, _ptr(planes), int(row_groups), _stream()), "rdo_split_h2_conv_px")
    else:
        L.check(L.lib().rdo_split_h2_conv(_ptr(w), co, kh, kw, ci, planes.scale, _ptr(planes), _stream()), "rdo_split_h2_conv")
    return planes


def conv_h2_supported(x_shape, w_shape, stride, pad, square_input=False):
    d = conv_desc(x_shape, w_shape, stride, pad, square_input=square_input)
    return bool(L.lib().rdo_conv2d_fwd_h2_supported(C.byref(d)))


def _oscale(p):
    return p.scale if p is not None else 1.0


def conv2d_fwd_h2(xp, x_shape, w_shape, wplanes, bias=None, stride=1, pad=0, epilogue=L.EPI_NONE, aux=None, residual=None, out=None, pre=None,
                  out_planes=None, aux_planes=None):
    """Conv on an H2 input (`xp` = planes of the NHWC tensor of shape `x_shape`) with fragment-ordered H2 weight planes; writes whichever
    of out / pre / out_planes is given."""
    d = conv_desc(x_shape, w_shape, stride, pad, epilogue, False, residual is not None)
    need = int(L.lib().rdo_conv2d_fwd_h2_workspace(C.byref(d)))
    ws = _scratch(xp.device, need) if need else None
    _bind_out(out_planes)
    L.check(L.lib().rdo_conv2d_fwd_h2(C.byref(d), _ptr(xp), xp.scale, _ptr(wplanes), wplanes.scale, _ptr(bias), _ptr(aux), _ptr(aux_planes),
                                      _ptr(residual), _ptr(out), _ptr(pre), _ptr(out_planes), _oscale(out_planes), _ptr(ws),
                                      ws.numel() if ws is not None else 0, _stream()), "rdo_conv2d_fwd_h2")
    return out


def conv_h2_px_supported(x_shape, w_shape, stride, pad, store_mode):
    """rdo_conv2d_fwd_h2_px takes this shape with this store mode (L.STORE_SHUFFLE / L.STORE_UNSHUFFLE)"""
    d = conv_desc(x_shape, w_shape, stride, pad)
    return bool(L.lib().rdo_conv2d_fwd_h2_px_supported(C.byref(d), int(store_mode)))


def conv2d_fwd_h2_px(xp, x_shape, w_shape, wplanes, store_mode, bias=None, stride=1, pad=0, epilogue=L.EPI_NONE, aux=None, residual=None, out=None,
                     out_planes=None, aux_planes=None):
    """conv2d_fwd_h2 whose stores carry the r = 2 pixel shuffle (store_mode 1: `wplanes` and `bias` with the rows in 4 groups, out /
    out_planes [B,2Ho,2Wo,Cout/4]) or its inverse (2: out / out_planes [B,Ho/2,Wo/2,4 Cout], channels in group order)."""
    d = conv_desc(x_shape, w_shape, stride, pad, epilogue, False, residual is not None)
    need = int(L.lib().rdo_conv2d_fwd_h2_workspace(C.byref(d)))
    ws = _scratch(xp.device, need) if need else None
    _bind_out(out_planes)
    L.check(L.lib().rdo_conv2d_fwd_h2_px(C.byref(d), _ptr(xp), xp.scale, _ptr(wplanes), wplanes.scale, _ptr(bias), _ptr(aux), _ptr(aux_planes),
                                         _ptr(residual), _ptr(out), None, _ptr(out_planes), _oscale(out_planes), _ptr(ws),
                                         ws.numel() if ws is not None else 0, int(store_mode), _stream()), "rdo_conv2d_fwd_h2_px")
    return out


def group_rows(rows):
    """index tensor p with p[g * C + c] = 4 c + g (C = rows / 4): t[p] is t with its rows in 4 groups (include/rdo_ptq_subpel.h)"""
    if rows % 4:
        raise ValueError("group_rows: the row count must be a multiple of 4")
    return torch.arange(rows).view(rows // 4, 4).t().reshape(-1)


def conv_h2_tail_supported(x_shape, w_shape, stride, pad):
    d = conv_desc(x_shape, w_shape, stride, pad)
    return bool(L.lib().rdo_conv2d_fwd_h2_tail_supported(C.byref(d)))


def conv2d_fwd_h2_tail(xp, x_shape, w_shape, wplanes, bias, stride, pad, residual_planes, tgt_cache, idx_table, iter_ptr, coef, act, dpre_planes,
                       loss_log):
    """Plane-input conv + unit tail in one launch: dpre_planes <- dL/dpre of out = act(conv + bias) + residual against tgt_cache[idx]."""
    d = conv_desc(x_shape, w_shape, stride, pad)
    _bind_out(dpre_planes)
    L.check(L.lib().rdo_conv2d_fwd_h2_tail(C.byref(d), _ptr(xp), xp.scale, _ptr(wplanes), wplanes.scale, _ptr(bias), _ptr(residual_planes),
                                           _oscale(residual_planes), _ptr(tgt_cache), _ptr(idx_table), _ptr(iter_ptr), x_shape[0], coef, int(act),
                                           _ptr(dpre_planes), dpre_planes.scale, _ptr(loss_log), _stream()), "rdo_conv2d_fwd_h2_tail")


def gather_qdrop_h2(cache_q, cache_fp, idx_table, iter_ptr, B, prob, seed, out, out_planes, batch_offset=0, iter_publish=None):
    per_image = cache_q[0].numel()
    _bind_out(out_planes)
    L.check(L.lib().rdo_gather_qdrop_h2(_ptr(cache_q), _ptr(cache_fp), _ptr(idx_table), _ptr(iter_ptr), B, int(batch_offset), per_image,
                                        cache_q.shape[-1], prob, seed, _ptr(out), _ptr(out_planes), out_planes.scale, _ptr(iter_publish),
                                        _stream()), "rdo_gather_qdrop_h2")


ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2


def loss_act_bwd(pre, residual, tgt_cache, idx_table, iter_ptr, coef, act, loss_log, out=None, grad_out=None, dpre=None, dpre_planes=None,
                 residual_planes=None):
    B, per_image = pre.shape[0], pre[0].numel()
    _bind_out(dpre_planes)
    L.check(L.lib().rdo_loss_act_bwd(_ptr(pre), _ptr(residual), _ptr(residual_planes), _oscale(residual_planes), _ptr(tgt_cache), _ptr(idx_table),
                                     _ptr(iter_ptr), B, per_image, pre.shape[-1], coef, int(act), _ptr(out), _ptr(grad_out), _ptr(dpre),
                                     _ptr(dpre_planes), _oscale(dpre_planes), _ptr(loss_log), _stream()), "rdo_loss_act_bwd")


def loss_gdn_bwd(x, norm, residual, tgt_cache, idx_table, iter_ptr, coef, inverse, loss_log, grad_out, t=None, t_planes=None, out=None):
    B, per_image = x.shape[0], x[0].numel()
    _bind_out(t_planes)
    L.check(L.lib().rdo_loss_gdn_bwd(_ptr(x), _ptr(norm), _ptr(residual), _ptr(tgt_cache), _ptr(idx_table), _ptr(iter_ptr), B, per_image,
                                     x.shape[-1], coef, int(inverse), _ptr(out), _ptr(grad_out), _ptr(t), _ptr(t_planes), _oscale(t_planes),
                                     _ptr(loss_log), _stream()), "rdo_loss_gdn_bwd")


def gdn_bwd_dx_h2(g, x, norm, acc, inverse, dx=None, dx_planes=None):
    _bind_out(dx_planes)
    L.check(L.lib().rdo_gdn_bwd_dx_h2(_ptr(g), _ptr(x), _ptr(norm), _ptr(acc), g.numel(), g.shape[-1], int(inverse), _ptr(dx),
                                      _ptr(dx_planes), _oscale(dx_planes), _stream()), "rdo_gdn_bwd_dx_h2")


def gdn_fwd_bwd_supported(rows, channels):
    return bool(L.lib().rdo_gdn_fwd_bwd_supported(int(rows), int(channels)))


def gdn_fwd_bwd(c, fwd_planes, bwd_planes, beta, residual, tgt_cache, idx_table, iter_ptr, coef, inverse, loss_log, t, grad_out=None, out=None,
                dx=None, dx_planes=None):
    """The GDN / IGDN block of a unit in one launch: linear_h2(square_input) + loss_gdn_bwd + linear_h2 (gamma'^T) + gdn_bwd_dx_h2, bit for
    bit; `fwd_planes` / `bwd_planes` from split_h2_linear of gamma' and of its transpose (one scale)."""
    if fwd_planes.scale != bwd_planes.scale:
        raise ValueError("gdn_fwd_bwd: the planes of gamma' and of its transpose must share one scale")
    B, per_image = c.shape[0], c[0].numel()
    _bind_out(dx_planes)
    L.check(L.lib().rdo_gdn_fwd_bwd(_ptr(c), _ptr(fwd_planes), _ptr(bwd_planes), float(fwd_planes.scale), _ptr(beta), _ptr(residual),
                                    _ptr(tgt_cache), _ptr(idx_table), _ptr(iter_ptr), B, per_image, c.shape[-1], coef, int(inverse), _ptr(out),
                                    _ptr(grad_out), _ptr(t), _ptr(dx), _ptr(dx_planes), _oscale(dx_planes), _ptr(loss_log), _stream()),
            "rdo_gdn_fwd_bwd")


def gdn_fwd_bwd_px_supported(shape):
    """rdo_gdn_fwd_bwd_px takes the block over an NHWC tensor of `shape`"""
    B, H, W, Cc = shape
    return bool(L.lib().rdo_gdn_fwd_bwd_px_supported(int(B) * int(H) * int(W), int(Cc), int(H), int(W)))


def gdn_fwd_bwd_px(c, fwd_planes, bwd_planes, beta, residual, tgt_cache, idx_table, iter_ptr, coef, inverse, loss_log, t, dup_planes, out=None,
                   dx=None, dx_planes=None):
    """gdn_fwd_bwd whose dL/dout leaves as `dup_planes`: the planes of pixel_unshuffle2(dL/dout) [B,H/2,W/2,4C] with the channels in group
    order (the dY operand of the weight gradient of a sub-pixel conv whose rows are in 4 groups).  `dup_planes` raise their own overflow
    words where they have some."""
    if fwd_planes.scale != bwd_planes.scale:
        raise ValueError("gdn_fwd_bwd_px: the planes of gamma' and of its transpose must share one scale")
    B, H, W, Cc = c.shape
    _bind_out(dx_planes)
    L.check(L.lib().rdo_gdn_fwd_bwd_px(_ptr(c), _ptr(fwd_planes), _ptr(bwd_planes), float(fwd_planes.scale), _ptr(beta), _ptr(residual),
                                       _ptr(tgt_cache), _ptr(idx_table), _ptr(iter_ptr), B, H, W, Cc, coef, int(inverse), _ptr(out),
                                       _ptr(dup_planes), dup_planes.scale, _ptr(getattr(dup_planes, "flag", None)), _ptr(t), _ptr(dx),
                                       _ptr(dx_planes), _oscale(dx_planes), _ptr(loss_log), _stream()), "rdo_gdn_fwd_bwd_px")


def pixel_shuffle_h2(x, out=None, out_planes=None):
    """[B,H,W,4C] -> [B,2H,2W,C] (r = 2) as fp32 and / or planes."""
    B, H, W, CC = x.shape
    _bind_out(out_planes)
    L.check(L.lib().rdo_pixel_shuffle_h2(_ptr(x), B, H, W, CC // 4, _ptr(out), _ptr(out_planes), _oscale(out_planes), _stream()),
            "rdo_pixel_shuffle_h2")


def pixel_unshuffle2(x, out=None, out_planes=None):
    """[B,2H,2W,C] -> [B,H,W,4C]: gradient of the r = 2 pixel shuffle (16-byte accesses on both sides), as fp32 and / or H2 planes."""
    B, Hr, Wr, Cc = x.shape
    if Hr % 2 or Wr % 2:
        raise ValueError(f"pixel_unshuffle2: r = 2 needs an even height and width, got {Hr} x {Wr} (the odd last row / column would be dropped)")
    if out is None and out_planes is None:
        out = torch.empty((B, Hr // 2, Wr // 2, 4 * Cc), device=x.device, dtype=torch.float32)
    _bind_out(out_planes)
    L.check(L.lib().rdo_pixel_unshuffle2(_ptr(x), B, Hr // 2, Wr // 2, Cc, _ptr(out), _ptr(out_planes), _oscale(out_planes), _stream()),
            "rdo_pixel_unshuffle2")
    return out


def wgrad_h2_supported(x_shape, w_shape, stride, pad):
    d = conv_desc(x_shape, w_shape, stride, pad)
    return bool(L.lib().rdo_conv2d_wgrad_h2_supported(C.byref(d)))


def wgrad_h2_layer_supported(x_shape, w_shape, stride, pad):
    """rdo_conv2d_wgrad_h2 takes this shape when it is the weight gradient of a layer unit on planes (narrower channel counts than the
    block units' 192: the general plane kernel masks its 192 x 192 tile)."""
    d = conv_desc(x_shape, w_shape, stride, pad)
    return bool(L.lib().rdo_conv2d_wgrad_h2_layer_supported(C.byref(d)))


def conv2d_wgrad_h2(xp, x_shape, dyp, w_shape, stride=1, pad=0, slabs=None):
    """Weight-gradient slabs from H2 operands (planes of x [B,H,W,Cin] and of dy [B,Ho,Wo,Cout])."""
    d = conv_desc(x_shape, w_shape, stride, pad)
    ns = int(L.lib().rdo_conv2d_wgrad_nsplit(C.byref(d))) if slabs is None else slabs.shape[0]
    if slabs is None:
        slabs = torch.empty((ns,) + tuple(w_shape), device=xp.device, dtype=torch.float32)
    L.check(L.lib().rdo_conv2d_wgrad_h2(C.byref(d), _ptr(xp), xp.scale, _ptr(dyp), dyp.scale, _ptr(slabs), ns, _stream()), "rdo_conv2d_wgrad_h2")
    return slabs
