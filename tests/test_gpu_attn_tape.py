"""The two kernels of csrc/attn_tape.hip (the backward of probs @ v and of the probabilities, both from GIVEN probabilities) against the
float64 reference of tests/attn_tape_reference.py, per element; their determinism and their 4-byte alignment contract; the tape forms
built on them (`WindowAttentionProbsFn`, `WindowAttentionPVFn`) composed with `ActQuantStaticFn` against the four kernels called by hand
and against the fused backward; and the module level: a trained, activation-quantised RSTB unit under torch's tape, `learn_act_ranges`
on it, and what stays refused.

Every launch writes into NaN-filled outputs, which must come back finite everywhere.  Every element obeys
|got - ref| <= c * unit + floor with the units and the floor of attn_tape_reference's docstring and c = 4 x the worst err / (unit + floor)
of its float32 restatement ON THE SAME INPUTS -- the rule of tests/test_gpu_attention.py; no bound comes from a kernel's output.  Each
figure is printed before it is asserted (pytest -s)."""
import types

import pytest
import torch

import attention_cases as AC
import attn_tape_reference as R
from oracle import attention_oracle as A

pytestmark = pytest.mark.gpu

KERNEL_CASES = ["vec_it2_model_head_hd32", "vec_it4_hs65_hd64", "vec_n16_hyper_hd12", "vec_n36_ndb_hd48", "vec_n4_ndb_hd64", "scalar_n64_hd5",
                "scalar_n16_hd33", "scalar_n1_hd5", "single_token_region_shift7", "windows_not_multiple_of_8_b3_hd16"]
TAPE_CASES = ["vec_n16_hyper_hd12", "one_window_per_axis_shift4"]
SENTINEL = -7.25


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


class Case:
    """operands of one geometry on both devices, the float64 references and the restatement's ratios, computed once per name"""
    _memo = {}

    @classmethod
    def get(cls, name):
        if name not in cls._memo:
            cls._memo[name] = cls(name)
        return cls._memo[name]

    def __init__(self, name):
        from hipops import ops
        geom = AC.PATH_CASES[name]
        self.g = g = A.Geom(*geom)
        self.inp = R.inputs(g, seed=len(name) + geom[3])
        self.pv, self.pb, self.r32 = R.restatement_ratios(g, self.inp)
        assert all(v < float("inf") for v in self.r32.values()), self.r32
        self.d = ops.attn_desc(g.B, g.H, g.W, g.C, g.heads, g.ws, g.shift, g.scale)
        self.dev = {k: v.cuda() for k, v in self.inp.items()}
        self.q3 = {"dq": slice(0, g.C), "dk": slice(g.C, 2 * g.C), "dv": slice(2 * g.C, 3 * g.C)}

    def hold(self, what, got, ref, unit, floor):
        assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not finite (never written?)"
        ratio = A.worst_ratio(got, ref, unit, floor)
        r32 = self.r32[what]
        print(f"  {what}: err / (unit + floor)  restatement {r32:.3f}  kernel {ratio:.3f}  allowed {4 * r32:.3f}")
        assert ratio <= 4 * r32, (what, ratio, 4 * r32)

    def run_pv_bwd(self, qkv=None, probs_q=None, dout=None, dprobs=None, dqkv=None):
        from hipops import ops
        g, dev = self.g, self.dev
        dprobs = _nan(g.windows, g.N, g.N, g.heads) if dprobs is None else dprobs
        dqkv = _nan(g.B, g.H, g.W, 3 * g.C) if dqkv is None else dqkv
        got = ops.window_attention_pv_bwd(self.d, dev["qkv"] if qkv is None else qkv, dev["probs_q"] if probs_q is None else probs_q,
                                          dev["dout"] if dout is None else dout, dprobs=dprobs, dqkv=dqkv)
        assert got[0] is dprobs and got[1] is dqkv
        return dprobs, dqkv

    def run_probs_bwd(self, qkv=None, probs=None, dprobs=None, dqkv=None):
        from hipops import ops
        g, dev = self.g, self.dev
        dqkv = _nan(g.B, g.H, g.W, 3 * g.C) if dqkv is None else dqkv
        assert ops.window_attention_probs_bwd(self.d, dev["qkv"] if qkv is None else qkv, dev["probs"] if probs is None else probs,
                                              dev["dprobs"] if dprobs is None else dprobs, dqkv=dqkv) is dqkv
        return dqkv


# ----------------------------------------------------------------------------- 1. per element against float64
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_both_kernels_match_float64_per_element(name):
    print(f"\n{name} {AC.PATH_CASES[name]}")
    c = Case.get(name)
    q3, pv, pb = c.q3, c.pv, c.pb
    dprobs, dqkv = c.run_pv_bwd()
    assert bool(torch.isfinite(dqkv).all()), "pv_bwd dqkv: elements not finite (never written?)"
    c.hold("dprobs", dprobs, pv["dprobs"], pv["u_dprobs"], pv["floor"])
    c.hold("dv", dqkv[..., q3["dv"]], pv["dv"], pv["u_dv"], pv["floor"])
    assert bool((dqkv[..., :2 * c.g.C] == 0).all()), "pv_bwd: the q and k thirds must be exactly 0"
    dqkv = c.run_probs_bwd()
    assert bool(torch.isfinite(dqkv).all()), "probs_bwd dqkv: elements not finite (never written?)"
    c.hold("dq", dqkv[..., q3["dq"]], pb["dq"], pb["u_dq"], pb["floor"])
    c.hold("dk", dqkv[..., q3["dk"]], pb["dk"], pb["u_dk"], pb["floor"])
    assert bool((dqkv[..., q3["dv"]] == 0).all()), "probs_bwd: the v third must be exactly 0"


# ----------------------------------------------------------------------------- 2. determinism, views one float into a buffer
def _off_by_one_float(t):
    """-> (a contiguous view of t's shape that starts one float past a 16-byte boundary, its buffer, the view's offset): 65 sentinel
    floats in front (64 + the one), 64 behind"""
    front = 65
    buf = torch.full((front + t.numel() + 64,), SENTINEL, device="cuda", dtype=torch.float32)
    view = buf[front:front + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and buf.data_ptr() % 16 == 0
    return view, buf, front


def _guards_untouched(buf, front, n):
    return bool((buf[:front] == SENTINEL).all()) and bool((buf[front + n:] == SENTINEL).all())


@pytest.mark.parametrize("name", ["vec_it2_model_head_hd32", "vec_n16_hyper_hd12"])
def test_repeated_launches_and_misaligned_views_give_the_same_bits(name):
    c = Case.get(name)
    g, dev = c.g, c.dev
    dprobs0, dv0 = c.run_pv_bwd()
    dqk0 = c.run_probs_bwd()
    dprobs1, dv1 = c.run_pv_bwd()
    dqk1 = c.run_probs_bwd()
    assert torch.equal(dprobs1, dprobs0) and torch.equal(dv1, dv0) and torch.equal(dqk1, dqk0)
    views = {k: _off_by_one_float(dev[k]) for k in ("qkv", "probs", "probs_q", "dout", "dprobs")}
    out_p, out_v, out_qk = (_off_by_one_float(t) for t in (_nan(*dprobs0.shape), _nan(*dv0.shape), _nan(*dqk0.shape)))
    c.run_pv_bwd(views["qkv"][0], views["probs_q"][0], views["dout"][0], dprobs=out_p[0], dqkv=out_v[0])
    c.run_probs_bwd(views["qkv"][0], views["probs"][0], views["dprobs"][0], dqkv=out_qk[0])
    assert torch.equal(out_p[0], dprobs0) and torch.equal(out_v[0], dv0) and torch.equal(out_qk[0], dqk0)
    for view, buf, front in list(views.values()) + [out_p, out_v, out_qk]:
        assert _guards_untouched(buf, front, view.numel())
    assert all(torch.equal(views[k][0], dev[k]) for k in views)                      # the inputs themselves


# ----------------------------------------------------------------------------- 3. / 4. the tape forms
def _quantiles(x, lo_q, hi_q, floor=0.0):
    """per channel (last dim) of x, on the CPU -> float32 [2C] = the lo_q | hi_q quantiles of the channel's values of magnitude >= floor"""
    rows = x.detach().cpu().double().reshape(-1, x.shape[-1])
    lo, hi = [], []
    for ch in range(rows.shape[1]):
        v = rows[:, ch]
        v = v[v.abs() >= floor]
        lo.append(torch.quantile(v, lo_q))
        hi.append(torch.quantile(v, hi_q))
    return torch.stack(lo + hi).to(torch.float32).cuda()


def _shares(x, rng):
    """elements of x [..., C] below, inside and above the range [2C]"""
    Cc = x.shape[-1]
    lo, hi = rng[:Cc], rng[Cc:]
    below, above = int((x < lo).sum()), int((x > hi).sum())
    return below, x.numel() - below - above, above


def _raw_forward(c, bits, ranges):
    """the quantised attention in raw launches -> probs, probs_q, out, rng0, rng1; `ranges(x, site)` gives a site's range from its input"""
    from hipops import ops
    g, dev = c.g, c.dev
    probs = _nan(g.windows, g.N, g.N, g.heads)
    ops.window_attention(c.d, dev["qkv"], dev["bias"], probs=probs, compute_out=False)
    rng0 = ranges(probs, 0)
    probs_q = ops.actquant_static(probs, rng0, n_bits=bits)
    out = ops.window_attention_pv(c.d, dev["qkv"], probs_q)
    rng1 = ranges(out, 1)
    return probs, probs_q, out, rng0, rng1


def _tape_grads(c, bits, rng0, rng1):
    """autograd through ProbsFn -> ActQuantStaticFn (site 0) -> PVFn -> ActQuantStaticFn (site 1) of sum(out * dout) -> dqkv, drng0, drng1"""
    from hipops.autograd import ActQuantStaticFn, WindowAttentionProbsFn, WindowAttentionPVFn
    dev = c.dev
    qkv = dev["qkv"].clone().requires_grad_(True)
    r0, r1 = rng0.clone().requires_grad_(True), rng1.clone().requires_grad_(True)
    probs = WindowAttentionProbsFn.apply(qkv, c.d, dev["bias"])
    pq = ActQuantStaticFn.apply(probs, r0, bits, True)
    out = ActQuantStaticFn.apply(WindowAttentionPVFn.apply(qkv, pq, c.d), r1, bits, True)
    assert r0.is_leaf and r1.is_leaf
    return torch.autograd.grad((out * dev["dout"]).sum(), [qkv, r0, r1]), out.detach()


@pytest.mark.parametrize("name", TAPE_CASES)
def test_the_tape_is_the_four_kernels_called_by_hand(name):
    from hipops import ops
    c = Case.get(name)
    dev, bits = c.dev, 8

    def clipping(x, site):
        # (masked pairs are a point mass at 0 that no range end can split: the 5 % are of the other probabilities)
        return _quantiles(x, 0.05, 0.95, floor=1e-30 if site == 0 else 0.0)
    probs, probs_q, out, rng0, rng1 = _raw_forward(c, bits, clipping)
    for site, x, rng in ((0, probs, rng0), (1, out, rng1)):
        shares = _shares(x, rng)
        print(f"  {name} site {site}: below / inside / above the range {shares} of {x.numel()}")
        assert min(shares) >= 10, (site, shares)
    (g_qkv, g_r0, g_r1), out_tape = _tape_grads(c, bits, rng0, rng1)
    assert torch.equal(out_tape, ops.actquant_static(out, rng1, n_bits=bits))
    d1, d0 = torch.zeros_like(rng1), torch.zeros_like(rng0)
    dx1 = ops.actquant_static_bwd(out, dev["dout"], rng1, d1, n_bits=bits)
    dpq, dqkv_v = ops.window_attention_pv_bwd(c.d, dev["qkv"], probs_q, dx1)
    dprobs = ops.actquant_static_bwd(probs, dpq, rng0, d0, n_bits=bits)
    dqkv_qk = ops.window_attention_probs_bwd(c.d, dev["qkv"], probs, dprobs)
    assert torch.equal(g_qkv, dqkv_v + dqkv_qk) and torch.equal(g_r1, d1) and torch.equal(g_r0, d0)
    assert bool(torch.isfinite(g_qkv).all()) and float(g_qkv.abs().max()) > 0 and float(d0.abs().max()) > 0 and float(d1.abs().max()) > 0


@pytest.mark.parametrize("name", TAPE_CASES)
def test_at_16_bits_with_open_ranges_the_tape_agrees_with_the_fused_backward(name):
    c = Case.get(name)
    g, inp, bits = c.g, c.inp, 16
    probs, probs_q, out, rng0, rng1 = _raw_forward(c, bits, lambda x, site: _quantiles(x, 0.0, 1.0))
    for site, x, rng in ((0, probs, rng0), (1, out, rng1)):
        below, inside, above = _shares(x, rng)
        assert below == 0 and above == 0, (site, below, above)                       # nothing is clipped
    (g_qkv, _, _), _ = _tape_grads(c, bits, rng0, rng1)
    ref = A.reference(g, inp["qkv"], inp["bias"], inp["dout"])
    r32 = A.restate32(g, inp["qkv"], inp["bias"], inp["dout"])["dqkv"]
    got = g_qkv.cpu().double()
    for k in ("dq", "dk"):
        sl = c.q3[k]
        allowed = 4 * A.worst_ratio(r32[..., sl], ref["dqkv"][..., sl], ref["u_dqkv"][..., sl])
        ratio = A.worst_ratio(got[..., sl], ref["dqkv"][..., sl], ref["u_dqkv"][..., sl])
        print(f"  {name} {k}: err / unit  tape {ratio:.3f}  allowed {allowed:.3f}")
        assert ratio <= allowed, (k, ratio, allowed)
    # the v third: the rule's bound plus what 16-bit rounding of the probabilities can move P^T dO, (r_h / (2 (2^16 - 1))) sum_i |dO_id|
    sl = c.q3["dv"]
    c_dv = 4 * A.worst_ratio(r32[..., sl], ref["dqkv"][..., sl], ref["u_dqkv"][..., sl])
    width = (rng0[g.heads:].cpu().double() - rng0[:g.heads].cpu().double()).view(1, g.heads, 1, 1)
    (dO,) = A.gather(g, inp["dout"].double(), 1)                                     # [windows, heads, N, hd]
    moved = A.scatter(g, [(width / (2 * (2 ** 16 - 1)) * dO.abs().sum(2, keepdim=True)).expand_as(dO)], A.F64)
    err = (got[..., sl] - ref["dqkv"][..., sl]).abs()
    bound = c_dv * ref["u_dqkv"][..., sl] + moved
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"  {name} dv: worst err / (c u + rounding allowance) {worst:.3f}  (c = {c_dv:.3f})")
    assert bool((err <= bound).all()), worst


# ----------------------------------------------------------------------------- 5. module level
def _holders(unit):
    from quantization import BaseQuantBlock, QuantModule
    return [m for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]


def _flags(unit):
    return [(m.use_weight_quant, m.use_act_quant, m.trained) for m in _holders(unit)]


def _unit(mode="static"):
    """a trained RSTB unit on 6 inputs; static: `max` ranges frozen, as in test_attention_wrapper_keeps_two_ranges"""
    import lic
    from helpers import AQ, WQ
    from quantization.quant_block import QuantRSTB
    from quantization.recon import calibrate_act_ranges
    torch.manual_seed(4)
    unit = QuantRSTB(lic.RSTB(dim=16, input_resolution=(8, 8), depth=2, num_heads=2, window_size=4, mlp_ratio=2.0), WQ, AQ).cuda().eval()
    for m in _holders(unit):
        m.trained = True
        m.act_quantizer.set_act_mode(mode)
    x = torch.randn(6, 16, 8, 8).cuda()
    unit.set_quant_state(False, False)
    with torch.no_grad():
        out_fp = unit(x, (8, 8)).clone()
    unit.set_quant_state(True, False)
    if mode == "static":
        calibrate_act_ranges(unit, x, "max", batch=2)
    return unit, x, out_fp


def _quant_on(unit):
    for m in _holders(unit):
        m.use_weight_quant = m.use_act_quant = True


def _attn_ranges(unit):
    from quantization.quant_block import QuantWindowAttention
    attns = [m for m in unit.modules() if isinstance(m, QuantWindowAttention)]
    assert len(attns) == 2
    return {(i, s): a.act_quantizer.act_range[s].detach().clone() for i, a in enumerate(attns) for s in (0, 1)}


def test_a_trained_quantised_rstb_unit_runs_under_the_tape():
    from hipops.autograd import SqDiffSumFn
    unit, x, out_fp = _unit()
    _quant_on(unit)
    quants = {id(m.act_quantizer): m.act_quantizer for m in _holders(unit)}.values()
    for q in quants:
        q.act_ste = True

    def run():
        xt = x.clone().requires_grad_(True)
        out = unit(xt, (8, 8))
        loss = SqDiffSumFn.apply(out, out_fp, float(out.shape[1]) / out.numel())
        (gx,) = torch.autograd.grad(loss, [xt])
        return out.detach(), gx
    out1, g1 = run()
    out2, g2 = run()
    print(f"  |dx| max {float(g1.abs().max()):.3e}")
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    assert torch.equal(g1, g2) and torch.equal(out1, out2)
    with torch.no_grad():
        plain = unit(x, (8, 8))
    assert torch.equal(plain, out1)


@pytest.mark.parametrize("mode", ["dynamic", "static"])
def test_quantisers_that_stay_off_the_tape_still_refuse_it(mode):
    """dynamic quantisers, and frozen static ones without `act_ste`: both hand back detached tensors.  With every quantiser of the unit
    applied the first one (behind norm1) already cuts the tape and the attention sees an untracked qkv; the refusal is for a tracked
    one, so only the attention wrappers apply theirs here."""
    from quantization.quant_block import QuantWindowAttention
    unit, x, _ = _unit(mode)
    _quant_on(unit)
    with torch.no_grad():
        assert bool(torch.isfinite(unit(x, (8, 8))).all())                          # the untracked path is as before
    for m in _holders(unit):
        m.use_act_quant = isinstance(m, QuantWindowAttention)
    with pytest.raises(NotImplementedError, match="static ranges"):
        unit(x.clone().requires_grad_(True), (8, 8))


def test_learn_act_ranges_on_an_rstb_unit_with_the_switch():
    from quantization.recon import learn_act_ranges
    unit, x, out_fp = _unit()
    start = {id(m): {k: r.detach().clone() for k, r in m.act_quantizer.act_range.items()} for m in _holders(unit)}
    frozen = _attn_ranges(unit)
    flags = _flags(unit)
    gen = torch.Generator().manual_seed(11)
    idx_table = torch.stack([torch.randperm(6, generator=gen)[:2] for _ in range(20)])

    def learn():
        for m in _holders(unit):
            m.act_quantizer.act_range = {k: r.clone() for k, r in start[id(m)].items()}
        learn_act_ranges(unit, x, out_fp, 20, 1e-3, 2, idx_table=idx_table, swin=True)
        return _attn_ranges(unit)
    first = learn()
    assert _flags(unit) == flags
    for m in _holders(unit):
        q = m.act_quantizer
        assert (q.act_frozen() or not q.act_range) and not any(r.requires_grad for r in q.act_range.values()) and q.act_obs == {}
    for key, r in first.items():
        n = r.numel() // 2
        moved = float((r - frozen[key]).abs().max())
        print(f"  attention {key[0]} site {key[1]}: largest move of an end {moved:.3e}")
        assert not torch.equal(r, frozen[key]), key
        assert bool((r[:n] >= frozen[key][:n]).all()) and bool((r[n:] <= frozen[key][n:]).all()), key     # inside the observed (max) range
    second = learn()
    assert all(torch.equal(first[k], second[k]) for k in first)


def test_block_reconstruction_still_refuses_learned_ranges_without_the_switch():
    from quantization import block_reconstruction
    unit, x, _ = _unit()
    args = types.SimpleNamespace(task_loss=2.0, act_mode="static", act_range="learned")
    with pytest.raises(NotImplementedError, match="RSTB"):
        block_reconstruction(None, unit, "g_a1", torch.zeros(2, 3, 64, 64), batch_size=2, iters=1, act_quant=True, args=args)
