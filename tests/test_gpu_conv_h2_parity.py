"""Every launch behind rdo_conv2d_fwd_h2 -- conv_fwd_h2_kernel with and without its K split + h2_splitk_epilogue, conv_fwd_h2h_kernel
<4,2,2,3> / <8,1,1,2> (csrc/conv_fwd_h2.hip), conv_fwd_h2k_kernel in its 256 x 192 / 64 / 48 tiles and its K-split form
(conv_fwd_h2k.hip) -- against tests/conv_h2_reference.py (pinned by tests/test_conv_h2_reference.py) at the smallest shapes that reach
them.  The `_px` store modes stay with test_gpu_subpel.py, the `_tail` entry with test_gpu_tail_parity.py.

Every case (conv_h2_reference.CASES; two input families each)
  * selects its launch with the tuning keys of its row (restored in `finally`; the defaults are asserted at the end), asserts
    ops.conv_h2_supported, records the call in a hipops.plan.Plan and asserts the dispatch tag of op_info() and the workspace size
    against the restated dispatcher (expected_launch / workspace_floats): a dispatch change cannot silently move a case;
  * builds the operands with ops.split_h2 / ops.split_h2_conv at the reference's scales and asserts their planes torch.equal to the
    CPU-restated ones: the float64 operands of the reference are what the kernel reads;
  * writes out / pre / the output planes into NaN-filled buffers (0x7E00 in the int16 planes) followed by 64 sentinel elements that must
    survive; before a K-split launch the shared scratch is filled with NaN, so that a partial tile no workgroup wrote shows up;
  * 'exact': out and pre torch.equal to the float32 of the reference, planes bit-equal to the split of it;
    'randn': per element |out - ref| <= (2 q + 4) u S + 2 u |ref| outside the kink mask, either branch's value inside it; `pre` against
    the pre-activation bound; no NaN; the planes torch.equal to the restated split of the fp32 `out` the same launch wrote (both epilogue
    styles split with rdo::h2_split_pk, the formula of the reference: no launch needs _close_planes' looser figure);
  * output forms on the LRELU + residual + pre run: planes only and fp32 only give the bits of the combined run; a second run of the
    recorded plan gives torch.equal outputs;
  * epilogues: NONE and LRELU + residual + pre everywhere; on one per-tap split, one k16 halo, one K32 and one K32 K-split case also
    NONE + residual, RELU, LRELU_BWD with aux, RELU_BWD with aux + residual, and the two `_BWD` forms again from aux_planes (bit-equal);
  * the overflow word stays clear; test_overflow_word raises it with one element and clears it.

Each figure is printed before it is asserted (pytest -s) and kept in FIGURES: the largest err / (u S) per launch; WORST keeps the largest
err / bound with its case.  MEASURED holds the figures of one full run on an MI355X: recorded, not asserted against."""
import ctypes as C
import math

import pytest
import torch

import conv_h2_reference as R

pytestmark = pytest.mark.gpu

U = R.U
NAN = float("nan")
SENT = 777.25
NAN16, SENT16 = 0x7E00, 0x5A5A
FIGURES = {}          # launch -> largest err / (u S) seen in this session
WORST = {}            # launch -> (largest err / bound, case)
REACHED = {}          # launch -> dispatch tag, as seen
# One run on an MI355X, as test_zz_figures prints FIGURES: launch -> (largest err / (u S), largest err / bound).
MEASURED = {"pertap": (79.3, 0.826), "pertap_split": (9.55, 0.217), "k16_192": (79.3, 0.283), "k16_64": (9.71, 0.201), "k32_192": (11.9, 0.276),
            "k32_64": (11.0, 0.249), "k32_48": (11.5, 0.267), "k32_64_split": (10.7, 0.179), "k32_48_split": (10.7, 0.091)}
# The allowance is 2 q + 4 with q between 2.8 (1x1_cout208) and 56 (k32_split48): the sequential chain of the reference pays for the
# channel scaled by 1e3 in every later addition.  Closest to its bound: 1x1_m49062 'randn' NONE at 0.826 (nine stages, q = 2.9).  The
# 'exact' family was bit-equal on every launch.


def _lib():
    from hipops import _lib as L
    from hipops import ops
    from hipops import plan
    return L, ops, plan


def _guarded(shape, dtype=torch.float32):
    n = math.prod(shape)
    fill, sent = (NAN, SENT) if dtype == torch.float32 else (NAN16, SENT16)
    buf = torch.full((n + 64,), fill, device="cuda", dtype=dtype)
    buf[n:] = sent
    return buf, buf[:n].view(shape)


def _intact(buf, n):
    sent = SENT if buf.dtype == torch.float32 else SENT16
    assert bool((buf[n:] == sent).all()), "a launch wrote past its output"


class _Run:
    """one recorded launch of a case: the operands on the device, guarded outputs, the plan"""

    def __init__(self, env, key, forms=("out", "pre", "planes"), aux_planes=False, res=None, out_scale=None):
        L, ops, plan = _lib()
        epi, use_aux, use_res, want_pre = R.EPILOGUES[key]
        xs, ws = env["xs"], env["ws"]
        os_ = (xs[0],) + R.out_hw(xs[1], xs[2], ws[1], env["s"], env["p"]) + (ws[0],)
        self.env, self.bufs = env, []
        self.out = self._buf(os_) if "out" in forms else None
        self.pre = self._buf(os_) if "pre" in forms and want_pre else None
        self.planes = None
        if "planes" in forms:
            t = self._buf((2, ws[0] // 16, math.prod(os_[:3]), 16), torch.int16)
            self.planes = ops.H2(t, env["oscale"][key] if out_scale is None else out_scale)
        aux = env["aux"] if use_aux and not aux_planes else None
        auxp = env["auxp"] if use_aux and aux_planes else None
        residual = (env["res"] if res is None else res) if use_res else None
        self.plan = plan.Plan()
        with self.plan.record():
            ops.conv2d_fwd_h2(env["xp"], xs, ws, env["wp"], env["bias"], env["s"], env["p"], epilogue=epi, aux=aux, residual=residual, out=self.out,
                              pre=self.pre, out_planes=self.planes, aux_planes=auxp)
        self.plan.keep(residual, aux)
        tags = [t for t, _, _ in self.plan.op_info()]
        assert tags == [env["expect"]["tag"]], (env["name"], key, tags, env["expect"])

    def _buf(self, shape, dtype=torch.float32):
        buf, view = _guarded(shape, dtype)
        self.bufs.append((buf, view.numel()))
        return view

    def outputs(self):
        return [t for t in (self.out, self.pre, None if self.planes is None else self.planes.t) if t is not None]

    def run(self):
        """two runs from refilled buffers (and a NaN-filled scratch): -> the outputs of the first, asserted equal to the second's"""
        _, ops, _ = _lib()
        first = None
        for _ in range(2):
            for t in self.outputs():
                t.fill_(NAN if t.dtype == torch.float32 else NAN16)
            if self.env["need"]:
                ops._scratch(self.env["xp"].device, self.env["need"]).fill_(NAN)
            self.plan.run(1, graph=False)
            torch.cuda.synchronize()
            for buf, n in self.bufs:
                _intact(buf, n)
            got = [t.clone() for t in self.outputs()]
            if first is None:
                first = got
            else:
                assert all(torch.equal(a, b) for a, b in zip(first, got)), (self.env["name"], "second run differs")
        return first


def _planes_of(t, scale):
    """the restated split of an fp32 tensor (on its own device) in the activation layout"""
    p0, p1, _ = R.split(t, scale)
    return R.act_planes(p0, p1)


def _hold(launch, label, got, ref, S, bnd, mask=None, alt=None, alt_bnd=None):
    """per element |got - ref| <= bnd (inside the mask: or |got - alt| <= alt_bnd); FIGURES and WORST"""
    assert bool(torch.isfinite(got).all()), (label, "NaN left")
    got = got.double()
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300))
    if mask is not None:
        err_a = (got - alt).abs()
        ratio_a = torch.where(err_a == 0, torch.zeros_like(err_a), err_a / alt_bnd.clamp_min(1e-300))
        took_alt = mask & (ratio_a < ratio)
        ratio = torch.where(took_alt, ratio_a, ratio)
        err = torch.where(took_alt, err_a, err)
    worst = float(ratio.max())
    live = S > 0
    fig = float((err[live] / (U * S[live])).max()) if bool(live.any()) else 0.0
    FIGURES[launch] = max(FIGURES.get(launch, 0.0), fig)
    if worst > WORST.get(launch, (0.0, ""))[0]:
        WORST[launch] = (worst, label)
    print(f"  [{label}] err / (u S) {fig:.3g}   err / bound {worst:.3f}")
    assert worst <= 1.0, (label, launch, worst, int((ratio > 1.0).sum()))


def _env(name, family, ops, L):
    """the operands of a case on the device, checked against the restated planes"""
    c = R.CASES[name]
    B, H, W, Cin, Cout, K, s, p = c[:8]
    cs = R.case(name, family)
    ref = cs["ref"]
    dev = lambda t: t.cuda().contiguous()
    xs, ws = (B, H, W, Cin), (Cout, K, K, Cin)
    assert ops.conv_h2_supported(xs, ws, s, p), name
    tuning = dict(R.TUNING_DEFAULTS, **c[9])
    expect = R.expected_launch(name)
    assert R.launch_name(expect) == c[8]
    need = int(L.lib().rdo_conv2d_fwd_h2_workspace(C.byref(ops.conv_desc(xs, ws, s, p))))
    Ho, Wo = R.out_hw(H, W, K, s, p)
    assert need == R.workspace_floats(c[:8], tuning), (name, need)
    assert (expect["ksplit"] == 1 or need >= expect["ksplit"] * B * Ho * Wo * Cout) and (need > 0 or expect["ksplit"] == 1), (name, need, expect)
    xp, wp = ops.split_h2(dev(cs["x"]), scale=ref.sx), ops.split_h2_conv(dev(cs["w"]), scale=ref.sw)
    assert torch.equal(xp.t.cpu(), ref.xplanes), (name, family, "activation planes differ from the restated split")
    assert torch.equal(wp.t.cpu(), ref.wplanes), (name, family, "weight planes differ from the restated split")
    aux = dev(cs["aux"])
    env = {"name": name, "xs": xs, "ws": ws, "s": s, "p": p, "xp": xp, "wp": wp, "bias": dev(cs["bias"]), "res": dev(cs["res"]), "aux": aux,
           "auxp": ops.split_h2(aux), "expect": expect, "need": need,
           "oscale": {k: R.pow2_scale(float(ref.out(k).ref.abs().max())) for k in R.epilogues_of(name)}}
    return env, ref


@pytest.mark.parametrize("name", list(R.CASES))
def test_conv_h2_launch(name):
    L, ops, _ = _lib()
    c = R.CASES[name]
    launch = c[8]
    saved = {k: ops.set_tuning(k, v) for k, v in c[9].items()}
    try:
        ops.h2_overflow(reset=True)
        for family in R.FAMILIES:
            env, ref = _env(name, family, ops, L)
            print(f"\n{name} {c[:8]} {family} -> {launch} {env['expect']}, workspace {env['need']}")
            REACHED[launch] = env["expect"]["tag"]
            for key in R.epilogues_of(name):
                epi, use_aux, use_res, want_pre = R.EPILOGUES[key]
                o = ref.out(key)
                label = f"{name} {family} {key}"
                run = _Run(env, key)
                got = run.run()
                out, planes = got[0], got[-1]
                pre = got[1] if want_pre else None
                assert torch.equal(planes, _planes_of(out, run.planes.scale)), (label, "planes are not the split of the fp32 out")
                if family == "exact":
                    out32, pre32 = ref.expected32(key)
                    assert torch.equal(out.cpu(), out32), (label, float((out.cpu().double() - out32.double()).abs().max()))
                    if want_pre:
                        assert torch.equal(pre.cpu(), pre32), (label, "pre")
                    assert torch.equal(planes.cpu(), _planes_of(out32, run.planes.scale)), (label, "planes")
                else:
                    g = lambda t: None if t is None else t.cuda()
                    _hold(launch, label, out, g(o.ref), g(o.S), g(o.bnd), g(o.mask), g(o.alt), g(o.alt_bnd))
                    if want_pre:
                        _hold(launch, label + " pre", pre, g(ref.pre), g(ref.S_pre), g(ref.bound_pre))
                if want_pre:                                                           # the output forms, on the run that has all three
                    only_planes = _Run(env, key, forms=("planes",)).run()
                    assert len(only_planes) == 1 and torch.equal(only_planes[0], planes), (label, "planes only")
                    only_out = _Run(env, key, forms=("out",)).run()
                    assert len(only_out) == 1 and torch.equal(only_out[0], out), (label, "fp32 only")
                if use_aux:                                                            # the mask from plane 0 of the aux tensor: the same bits
                    again = _Run(env, key, aux_planes=True).run()
                    assert torch.equal(again[0], out) and torch.equal(again[-1], planes), (label, "aux_planes")
            assert not ops.h2_overflow(reset=True), (name, family, "overflow word raised")
    finally:
        for k, v in saved.items():
            ops.set_tuning(k, v)
    for k, v in R.TUNING_DEFAULTS.items():
        assert int(L.lib().rdo_get_tuning(k.encode())) == v, (k, v)


def test_overflow_word():
    """'exact' family, NONE + residual with ONE output of 2^(16 - j) and out_scale 2^j: 65536 does not fit fp16, every other element does"""
    L, ops, _ = _lib()
    name = next(n for n, c in R.CASES.items() if "ovf" in c[10])
    env, _ = _env(name, "exact", ops, L)
    res, scale, want = R.overflow_setup(name)
    ops.h2_overflow(reset=True)
    quiet = _Run(env, "none_res", out_scale=scale / 2.0).run()                          # one binade of head-room: nothing overflows
    assert not ops.h2_overflow(reset=True)
    got = _Run(env, "none_res", res=res.cuda(), out_scale=scale).run()
    assert ops.h2_overflow(reset=True), "65536 in the planes did not raise the overflow word"
    assert not ops.h2_overflow(reset=True), "reset did not clear the overflow word"
    assert torch.equal(got[0].cpu(), want)
    assert torch.equal(got[-1], _planes_of(got[0], scale))                             # +inf / -inf in that one record, as the split gives
    assert int((got[-1][0] == 0x7C00).sum()) == 1 and int((quiet[-1][0] == 0x7C00).sum()) == 0


def test_zz_figures():
    """prints what the session measured (pytest -s)"""
    print("\nFIGURES = {" + ", ".join(f'"{k}": {v:.3g}' for k, v in sorted(FIGURES.items())) + "}")
    print("WORST err / bound: " + ", ".join(f"{k}: {v[0]:.3f} ({v[1]})" for k, v in sorted(WORST.items())))
    print("launches reached: " + ", ".join(f"{k} -> {v}" for k, v in sorted(REACHED.items())))
    assert set(REACHED.values()) <= set(R.TAGS)
    if len(REACHED) == len(R.TABLE):                                                    # a full session: every row of the table was run
        assert set(REACHED.values()) == set(R.TAGS)
