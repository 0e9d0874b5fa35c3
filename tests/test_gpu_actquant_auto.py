"""The measured range choice on the GPU: `ops.actquant_score` against a restatement (the quantiser's arithmetic step by step in fp32, the
sums in float64, the counts as integers), the per-channel choice of act_range='auto' against the same restatement, and the calibration
flow with 'auto' and with `act_report` on the toy models of the other activation-quantiser tests."""
import io
import math
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SHAPES = [(16384, 192), (35, 1280), (561, 3), (1, 6), (300000, 1)]
BITS = [4, 8, 16]
# what a 1e-4 relative bound on both of two sums allows between their ratio and the exact one
FACTOR = (1 + 1e-4) / (1 - 1e-4)


# ----------------------------------------------------------------------------- the restatement
def _score_ref(x, cand, n_bits):
    """x [npix, C], cand [K, 2C] (fp32, any device) -> err float64 [C, K], clip int64 [C, K, 2], energy float64 [C] on the CPU: aq_quant
    of csrc/actquant.hip one fp32 operation at a time (torch rounds each on its own), the residual and its square in fp32 as the kernel
    forms them, only the sums in float64; the clipped counts from fp32 comparisons with the ends"""
    C, K = x.shape[1], cand.shape[0]
    R = torch.tensor(float(2 ** n_bits - 1), dtype=torch.float32, device=x.device)
    err = torch.zeros(C, K, dtype=torch.float64)
    clip = torch.zeros(C, K, 2, dtype=torch.int64)
    for k in range(K):
        lo, hi = cand[k, :C], cand[k, C:]
        rng = torch.clamp(hi - lo, min=1e-6)
        q = torch.round(torch.clamp((x - lo) / rng, 0, 1) * R)
        d = x - ((q / R) * rng + lo)
        err[:, k] = (d * d).double().sum(0).cpu()
        clip[:, k, 0] = (x < lo).sum(0).cpu()
        clip[:, k, 1] = (x > hi).sum(0).cpu()
    return err, clip, (x * x).double().sum(0).cpu()


def _rel_err(got, ref):
    nz = ref != 0
    assert bool((got[~nz] == 0).all())
    return float(((got[nz] - ref[nz]).abs() / ref[nz]).max()) if bool(nz.any()) else 0.0


def _unaligned(x):
    """the same values behind a data pointer that is 4 bytes past a 16-byte boundary"""
    buf = torch.empty(x.numel() + 1, device=x.device, dtype=x.dtype)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _heavy(npix, C):
    """cubed normal values (heavy tails), the negative side squeezed, one constant channel"""
    g = torch.Generator().manual_seed(npix + C)
    z = torch.randn(npix, C, generator=g)
    x = z ** 3 * (0.25 + torch.arange(C) % 7) * 0.3
    x = torch.where(x < 0, x * 0.01, x)
    if C > 1:
        x[:, 1] = 0.75
    return x.float().contiguous()


def _clipping_cands(x):
    """four grids per channel: the observed range, both ends shrunk towards zero, and two that cut different shares off the two ends"""
    lo, hi = x.amin(0), x.amax(0)
    w = hi - lo
    return torch.stack([torch.cat([lo, hi]), torch.cat([lo * 0.7, hi * 0.7]), torch.cat([lo + 0.1 * w, hi - 0.3 * w]),
                        torch.cat([lo + 0.25 * w, hi - 0.05 * w])]).float().contiguous()


def _score(ops, x, cand, n_bits, clip=True, energy=True):
    C, K = x.shape[-1], cand.shape[0]
    err = torch.zeros(C, K, device="cuda")
    cl = torch.zeros(C, K, 2, dtype=torch.int32, device="cuda") if clip else None
    en = torch.zeros(C, device="cuda") if energy else None
    ops.actquant_score(x, cand, err, cl, en, n_bits=n_bits)
    return err, cl, en


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("n_bits", BITS)
@pytest.mark.parametrize("npix,C", SHAPES)
def test_score_matches_the_restatement(npix, C, n_bits, K):
    """err and energy within 1e-4 relative of the restatement (non-negative terms, serial chains of at most 1024 of them plus the tree:
    (1024 + 20) * 2^-24 = 6.2e-5), the counts exactly; the same bits from a second launch and without the nullable outputs; two calls on
    two parts of the tensor (an uneven split, the second part behind an unaligned pointer) against one call on the whole; with K = 1
    the error of `ops.actquant_static` itself."""
    from hipops import ops
    x = _heavy(npix, C)
    cand = _clipping_cands(x)
    cand = cand[2:3].contiguous() if K == 1 else cand
    ref_err, ref_clip, ref_energy = _score_ref(x, cand, n_bits)
    xc, cc = x.cuda(), cand.cuda()
    err, clip, energy = _score(ops, xc, cc, n_bits)
    worst = max(_rel_err(err.cpu().double(), ref_err), _rel_err(energy.cpu().double(), ref_energy))
    print(f"score npix={npix} C={C} n_bits={n_bits} K={K}: largest relative error {worst:.3e}, clipped {int(ref_clip.sum())} of {npix * C * K}")
    assert worst <= 1e-4
    assert torch.equal(clip.cpu().long(), ref_clip)
    if npix > 1:
        assert int(ref_clip.sum()) > 0                                    # (the candidates do clip)
    err2, clip2, energy2 = _score(ops, xc, cc, n_bits)                    # fixed reduction order: the same bits from launch to launch
    assert torch.equal(err, err2) and torch.equal(clip, clip2) and torch.equal(energy, energy2)
    err3, _, _ = _score(ops, xc, cc, n_bits, clip=False, energy=False)    # the nullable outputs do not change err
    assert torch.equal(err, err3)
    if npix > 1:
        cut = (npix * 3) // 8 + 1
        e2 = torch.zeros_like(err)
        c2 = torch.zeros_like(clip)
        n2 = torch.zeros_like(energy)
        ops.actquant_score(xc[:cut].contiguous(), cc, e2, c2, n2, n_bits=n_bits)
        ops.actquant_score(_unaligned(xc[cut:].contiguous()), cc, e2, c2, n2, n_bits=n_bits)
        assert torch.equal(c2, clip)
        assert _rel_err(e2.cpu().double(), ref_err) <= 1e-4 and _rel_err(n2.cpu().double(), ref_energy) <= 1e-4
        assert _rel_err(e2.cpu().double(), err.cpu().double()) <= 1e-4
    if K == 1:
        y = ops.actquant_static(xc, cc[0].contiguous(), n_bits=n_bits)
        same = ((xc - y).double() ** 2).sum(0).cpu()
        assert _rel_err(err[:, 0].cpu().double(), same) <= 1e-4


@pytest.mark.parametrize("npix,C", [(4099, 8), (2050, 3)])
def test_counts_on_a_lattice_are_exact_at_the_ends(npix, C):
    """values on multiples of 2^-8 and candidate ends on the same lattice: a value EQUAL to an end is inside (x < lo and x > hi are plain
    fp32 comparisons), and every channel has such values"""
    from hipops import ops
    g = torch.Generator().manual_seed(npix)
    shift = (torch.arange(C) % 3) / 256.0                                 # steps of 2^-5, each channel 0, 1 or 2 steps of 2^-8 off zero
    x = (torch.randint(-40, 41, (npix, C), generator=g).float() / 32.0 + shift).contiguous()
    lo = torch.tensor([-1.0, -0.5, -0.25, 0.0]).repeat(C, 1).t().contiguous() + shift
    hi = torch.tensor([1.0, 0.75, 0.5, 0.125]).repeat(C, 1).t().contiguous() + shift
    cand = torch.cat([lo, hi], dim=1).float().contiguous()
    for k in range(4):
        assert bool(((x == cand[k, :C]).sum(0) > 0).all()) and bool(((x == cand[k, C:]).sum(0) > 0).all())
    ref_err, ref_clip, ref_energy = _score_ref(x, cand, 8)
    err, clip, energy = _score(ops, x.cuda(), cand.cuda(), 8)
    assert torch.equal(clip.cpu().long(), ref_clip) and int(ref_clip.min()) > 0
    for k in range(4):                                                    # the counts, once more, from integers
        xi, li, hi_i = (x * 256).long(), (cand[k, :C] * 256).long(), (cand[k, C:] * 256).long()
        assert torch.equal(clip[:, k, 0].cpu().long(), (xi < li).sum(0)) and torch.equal(clip[:, k, 1].cpu().long(), (xi > hi_i).sum(0))
    assert _rel_err(err.cpu().double(), ref_err) <= 1e-4 and _rel_err(energy.cpu().double(), ref_energy) <= 1e-4


def test_long_chains_and_counts_beyond_the_float_integers():
    """More than 1024 pixels per thread (one channel: all 256 lanes of all 256 workgroups walk the pixels, 1100 each): the running sums
    are closed every 1024 terms.  The same tensor has 72 M values, and the candidates clip more than 2^24 of them at an end: a count
    carried in ONE fp32 number would stop counting there.  The restatement is evaluated by torch on the device (288 MB in fp32 and its
    temporaries, as in test_search_closes_long_chains)."""
    from hipops import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    npix = 256 * 256 * 1100
    x = (torch.rand(npix, 1, generator=g, device="cuda") ** 2).contiguous()
    lo, hi = float(x.min()), float(x.max())
    cand = torch.tensor([[lo, hi], [0.09, 0.81], [0.0, 0.49], [0.25, 1.0]], device="cuda")
    ref_err, ref_clip, ref_energy = _score_ref(x, cand, 8)
    err, clip, energy = _score(ops, x, cand, 8)
    assert int(ref_clip[0, 1, 0]) > 2 ** 24 and int(ref_clip[0, 2, 1]) > 2 ** 24 and int(ref_clip[0, 3, 0]) > 2 ** 24
    assert torch.equal(clip.cpu().long(), ref_clip)
    worst = max(_rel_err(err.cpu().double(), ref_err), _rel_err(energy.cpu().double(), ref_energy))
    print(f"score {npix} x 1: largest relative error {worst:.3e}, counts {ref_clip.reshape(-1).tolist()}")
    assert worst <= 1e-4


# ----------------------------------------------------------------------------- the choice
def _channels(C):
    return 0.25 + (torch.arange(C) % 7) * 0.5, (torch.arange(C) % 5 - 2.0) * 1.5


def _laplace(npix, C, seed):
    u = torch.rand(npix, C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5
    s, o = _channels(C)
    return ((-torch.sign(u) * torch.log1p(-2 * u.abs())) * s + o).float().contiguous()


def _student_t3(npix, C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(npix, C, generator=g)
    chi2 = (torch.randn(3, npix, C, generator=g) ** 2).sum(0)
    s, o = _channels(C)
    return ((z / torch.sqrt(chi2 / 3.0)) * s + o).float().contiguous()


def _one_sided(npix, C, seed):
    """0.5 + an Exponential(1) value, each channel with its own scale"""
    u = torch.rand(npix, C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return ((0.5 - torch.log1p(-u)) * _channels(C)[0]).float().contiguous()


DISTS = {"laplace": _laplace, "student_t3": _student_t3, "one_sided": _one_sided}


def _quantiser(bits):
    from quantization.quantizer import UniformAffineQuantizer
    return UniformAffineQuantizer(n_bits=8, channel_wise=True, scale_method="max", act=True, act_mode="static", dynamic_bits=bits)


def _auto_on_one_tensor(x, bits):
    """observe -> search + histogram -> score -> freeze on one tensor -> (candidates [4, 2C], frozen range [2C]) on the CPU"""
    q = _quantiser(bits)
    q.act_observe()
    q(x, True)
    obs = q.act_range[0].clone()
    q.act_histogram(rule="mse", search=True)
    y = q(x, True)
    cands = q.act_candidates()
    assert torch.equal(cands[0][0], obs)
    q.act_score(cands)
    assert torch.equal(q(x, True), y)                                     # the max-range output goes downstream in both phases
    assert q.act_score_n == {0: x.shape[0]}
    q.act_freeze()
    assert q.act_frozen() and q.act_err == {} and q.act_hist == {} and q.act_cand == {} and q.act_obs == {}
    return cands[0].cpu(), q.act_range[0].cpu()


def _choice_ref(x, cands, frozen, bits):
    """-> (float64 sums [C, 4], first arg-min, channels whose best and second-best DISTINCT sums are more than 1e-4 relative apart,
    float64 sum of the frozen range [C])"""
    ref = _score_ref(x, cands, bits)[0]
    best = ref.min(dim=1).values
    above = torch.where(ref > best[:, None], ref, torch.full_like(ref, float("inf")))
    second = above.min(dim=1).values
    clear = torch.isinf(second) | ((second - best) > 1e-4 * second)      # (no second distinct sum: clear)
    win = torch.from_numpy(np.argmin(ref.numpy(), axis=1))                # numpy returns the FIRST minimum
    mine = _score_ref(x, frozen[None], bits)[0][:, 0]
    return ref, win, clear, mine


@pytest.mark.parametrize("dist", sorted(DISTS))
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("npix,C", SHAPES)
def test_auto_freezes_the_candidate_of_least_float64_error(npix, C, bits, dist):
    x = DISTS[dist](npix, C, 1000 + npix % 997 + C)
    cands, frozen = _auto_on_one_tensor(x.cuda(), bits)
    ref, win, clear, mine = _choice_ref(x, cands, frozen, bits)
    want = torch.cat([cands[:, :C].gather(0, win[None]).reshape(-1), cands[:, C:].gather(0, win[None]).reshape(-1)])
    sel = torch.cat([clear, clear])
    share = float((~clear).float().mean())
    wins = [int((win == k).sum()) for k in range(4)]
    print(f"auto {dist} npix={npix} C={C} bits={bits}: float64 winners max/l2/percentile/hist_mse {wins}, tie band {int((~clear).sum())} "
          f"channels ({share:.4f}), worst frozen / least {float((mine / ref.min(1).values.clamp(min=1e-300)).max()):.6f}")
    assert torch.equal(frozen[sel], want[sel])
    assert bool((mine <= FACTOR * ref.min(dim=1).values).all())
    assert share <= 0.05
    obs = cands[0]
    assert bool((frozen[:C] >= obs[:C]).all()) and bool((frozen[C:] <= obs[C:]).all())


def test_one_sided_channels_at_4_bits_exercise_the_choice():
    """Over the one-sided case at 4 bits (all five shapes), at least two different candidates each win a channel: otherwise nothing above
    exercises a choice.  The frozen range is matched against the candidate rows (first match).  The condition is on the case as a
    whole: a shape with one channel has one winner, the single-pixel shape freezes the max range everywhere (all four sums are zero),
    and with 16 384 values per channel the histogram-MSE range wins all 192 channels (measured on an MI355X; on 35 x 1280 it was 410 max,
    89 l2, 781 hist_mse).  The widest shape must show the choice on its own."""
    total = [0, 0, 0, 0]
    for npix, C in SHAPES:
        x = _one_sided(npix, C, 1000 + npix % 997 + C)
        cands, frozen = _auto_on_one_tensor(x.cuda(), 4)
        rows = torch.cat([cands[:, :C, None], cands[:, C:, None]], dim=2)                  # [4, C, 2]
        mine = torch.stack([frozen[:C], frozen[C:]], dim=1)
        match = (rows == mine[None]).all(dim=2)                                            # [4, C]
        assert bool(match.any(dim=0).all())                                                # every channel froze one of its candidates
        first = torch.from_numpy(np.argmax(match.numpy(), axis=0))
        wins = [int((first == k).sum()) for k in range(4)]
        print(f"one-sided npix={npix} C={C}, 4 bits: channels won by max/l2/percentile/hist_mse {wins}")
        total = [a + b for a, b in zip(total, wins)]
        if (npix, C) == (35, 1280):
            assert sum(1 for w in wins if w > 0) >= 2
    assert sum(1 for w in total if w > 0) >= 2


# ----------------------------------------------------------------------------- calibration flow (toy Cheng2020, toy Lu2022)
def _toy(bits=None, **extra):
    """`_toy` of test_gpu_actquant_static.py, restated; `bits`: the activation grid width (`dynamic_bits`)"""
    import lic
    from quantization import QuantModel
    torch.manual_seed(1005)
    N, n_img, B, iters = 8, 4, 2, 6
    model = lic.Cheng2020Anchor(N=N).cuda().eval()
    g = torch.Generator().manual_seed(13)
    cali = torch.rand(n_img, 3, 64, 64, generator=g).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    if bits is not None:
        aq["dynamic_bits"] = bits
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq, is_cheng=True).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:B])
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Cheng2020", **extra)
    kwargs = dict(cali_data=cali, batch_size=B, iters=iters, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2),
                  warmup=0.2, act_quant=True, opt_mode="mse", config=None, args=args)
    qnn.set_quant_state(True, True)
    qnn.model.g_s[-1][0].set_quant_state(True, False)
    return qnn, cali, list(qnn.model.g_a.named_children()), kwargs, g, N


def _unit_quants(unit):
    from quantization import BaseQuantBlock, QuantModule
    mods = [m for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    return mods, list({id(m.act_quantizer): m.act_quantizer for m in mods}.values())


def _run_w8a8(unit, inp_q, batch, prepare=None, seen=None):
    """the unit in its W8A8 state over its cached inputs, as `calibrate_act_ranges` runs it; `prepare(quants)` is called once the state
    is set; `seen`: a dict that receives (quantiser index, site) -> the list of channels-last tensors the site was handed.  Every quant
    state flag is left as it was found."""
    from quantization.quant_block import QuantRSTB
    from quantization.quantizer import _act_rows
    mods, quants = _unit_quants(unit)
    states = [(m, m.use_weight_quant, m.use_act_quant) for m in mods]
    hooks = []
    if seen is not None:
        for i, q in enumerate(quants):
            def hook(mod, a, kw, i=i):
                if len(a) > 1 and a[1]:
                    seen.setdefault((i, kw.get("site", 0)), []).append(_act_rows(a[0], kw.get("channels_last", False))[0].clone())
            hooks.append(q.register_forward_pre_hook(hook, with_kwargs=True))
    try:
        for m in mods:
            m.use_weight_quant = m.use_act_quant = True
        if prepare is not None:
            prepare(quants)
        with torch.no_grad():
            for i in range(0, inp_q.shape[0], batch):
                h = inp_q[i:i + batch]
                unit(h, (h.shape[2], h.shape[3])) if isinstance(unit, QuantRSTB) else unit(h)
    finally:
        for h in hooks:
            h.remove()
        for m, w, a_ in states:
            m.use_weight_quant, m.use_act_quant = w, a_
    return quants


def _candidates_by_hand(unit, inp_q, batch):
    """What `calibrate_act_ranges(..., 'auto')` does up to the scoring, by hand: observing, then the search + histogram pass, during which
    every site's input (behind max-range upstream quantisers: what the scoring pass sees) is kept -> {(quantiser index, site): (the
    site's values [npix, C], candidates [4, 2C])}.  The quantisers are left as they were found."""
    _, quants = _unit_quants(unit)
    names = ("act_phase", "act_range", "act_err", "act_obs", "act_hist", "act_hist_n", "act_tail", "act_hist_rule", "act_stats")
    found = [{n: (dict(getattr(q, n)) if isinstance(getattr(q, n), dict) else getattr(q, n)) for n in names} for q in quants]
    seen = {}
    try:
        _run_w8a8(unit, inp_q, batch, prepare=lambda qs: [q.act_observe() for q in qs])
        _run_w8a8(unit, inp_q, batch, prepare=lambda qs: [q.act_histogram(rule="mse", search=True) for q in qs if q.act_range], seen=seen)
        out = {}
        for i, q in enumerate(quants):
            if q.act_range:
                for site, cnd in q.act_candidates().items():
                    xs = torch.cat([t.reshape(-1, t.shape[-1]) for t in seen[(i, site)]])
                    out[(i, site)] = (xs, cnd)
        return out
    finally:
        for q, st in zip(quants, found):
            for n, v in st.items():
                setattr(q, n, v)


def _err64(ops, xs, rng, bits):
    return ((xs - ops.actquant_static(xs, rng.contiguous(), n_bits=bits)).double() ** 2).sum(0)


def _check_auto_unit(unit, inp_q, batch, bits):
    """every frozen range of the unit lies inside its max range, is assembled from its site's candidates, and its error on the site's
    inputs, recomputed with `ops.actquant_static` in float64, is within FACTOR of every candidate's -> sites checked"""
    from hipops import ops
    _, quants = _unit_quants(unit)
    byhand = _candidates_by_hand(unit, inp_q, batch)
    n = 0
    for i, q in enumerate(quants):
        assert q.act_frozen() == bool(q.act_range)
        for site, rng in q.act_range.items():
            xs, cnd = byhand[(i, site)]
            c = rng.numel() // 2
            assert q.dynamic_bits == bits and cnd.shape == (4, 2 * c)
            assert bool((rng[:c] >= cnd[0, :c]).all()) and bool((rng[c:] <= cnd[0, c:]).all()) and bool((rng[:c] <= rng[c:]).all())
            rows = torch.stack([cnd[:, :c], cnd[:, c:]], dim=2)
            assert bool((rows == torch.stack([rng[:c], rng[c:]], dim=1)[None]).all(dim=2).any(dim=0).all())
            mine = _err64(ops, xs, rng, bits)
            for k in range(4):
                assert bool((mine <= FACTOR * _err64(ops, xs, cnd[k], bits)).all()), (i, site, k)
            n += 1
    assert len(byhand) == n
    return n


def _expect_frozen(unit, N):
    """`_expect_ranges` of the other activation-quantiser tests: every quantiser of a calibrated Cheng2020 block that the W8A8 forward
    applies is frozen with the right channel count and holds nothing of the passes any more; the others have no range"""
    from quantization import BaseQuantBlock, QuantModule
    sites = {"rbws": [0, 1], "rbu": [0, 1], "rb": [0, 1, 2]}[unit.unit_kind]
    q = unit.act_quantizer
    assert q.act_frozen() and sorted(q.act_range) == sites and all(q.act_range[s].numel() == 2 * N for s in sites)
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            q = m.act_quantizer
            assert q.act_hist == {} and q.act_obs == {} and q.act_err == {} and q.act_cand == {} and q.act_clip == {} and q.act_energy == {}
        if isinstance(m, QuantModule):
            if m.disable_act_quant or m.is_ps:
                assert q.act_range == {} and not q.act_frozen()
            else:
                c = m.org_weight.shape[0]
                assert q.act_frozen() and sorted(q.act_range) == [0] and q.act_range[0].numel() == 2 * c
                assert bool(torch.isfinite(q.act_range[0]).all()) and bool((q.act_range[0][:c] <= q.act_range[0][c:]).all())
        elif isinstance(m, BaseQuantBlock):
            assert m is unit


def _frozen(units):
    return [{k: r.clone() for k, r in m.act_quantizer.act_range.items()} for _, u in units for m in u.modules() if hasattr(m, "act_quantizer")]


@pytest.mark.parametrize("bits", [8, 4])
def test_flow_with_auto_ranges(bits):
    """every calibrated unit's quantisers are frozen, every frozen range lies inside its max range and no channel's error on the cached
    inputs exceeds that of any of its four candidates by more than FACTOR (`_check_auto_unit`); the evaluation runs with the two
    calibrated units in their W8A8 state (the rest of the toy model is not calibrated here and stays in full precision); a second run
    freezes the same bits"""
    from quantization import block_reconstruction
    from quantization.export import activation_report, activation_state
    from quantization.utils import save_inp_oup_data
    from test_datasets import evaluate_images
    runs = []
    for again in (False, True):
        qnn, cali, units, kwargs, g, N = _toy(bits=bits, act_mode="static", act_range="auto", timing=[])
        n = 0
        for name, u in units[:2]:
            (inp_q, _), _ = save_inp_oup_data(qnn, u, cali, asym=True, act_quant=True, batch_size=4, input_prob=True)
            block_reconstruction(qnn, u, name, **kwargs)
            _expect_frozen(u, N)
            if not again:
                n += _check_auto_unit(u, inp_q, 4, bits)
        runs.append(_frozen(units[:2]))
        if again:
            break
        assert n >= 5
        timing = kwargs["args"].timing
        assert len(timing) == 2 and all("act_s" in t and t["act_s"] >= 0 for t in timing)
        assert activation_report(qnn) == {} and len(activation_state(qnn)) == n
        qnn.set_quant_state(False, False)
        for _, u in units[:2]:
            u.set_quant_state(True, True)
        psnr, bpp = evaluate_images(qnn.eval(), [torch.rand(1, 3, 64, 64, generator=g)], p=64)
        assert math.isfinite(psnr) and math.isfinite(bpp)
    assert len(runs[0]) == len(runs[1]) and all(sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a) for a, b in zip(*runs))


def test_auto_ranges_on_the_first_swin_unit_of_toy_lu2022():
    """a Swin (RSTB) unit takes the mode like any histogram mode (no tape is involved): both sites of every attention wrapper end frozen,
    each on the candidate of least measured error"""
    import lic
    from quantization import BaseQuantBlock, QuantModel, QuantModule, block_reconstruction, layer_reconstruction
    from quantization.quant_block import QuantRSTB, QuantWindowAttention
    from quantization.utils import save_inp_oup_data
    torch.manual_seed(1005)
    cfg = dict(height=64, width=64, in_chans=3, embed_dim=16, latent_dim=32, window_size=8, mlp_ratio=2.0, qkv_bias=True,
               qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_checkpoint=False)
    model = lic.NIC(cfg)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if p_.dim() >= 2 and "entropy_bottleneck" not in n_:
                p_.copy_((torch.rand(p_.shape, generator=g) - 0.5) * 2 * (3.0 / p_[0].numel()) ** 0.5)
    model = model.cuda().eval()
    n_img, B, iters = 8, 4, 6
    cali = torch.rand(n_img, 3, 64, 64, generator=g).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:B])
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Lu2022", act_mode="static", act_range="auto", act_report=True)
    kwargs = dict(cali_data=cali, batch_size=B, iters=iters, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2),
                  warmup=0.2, act_quant=True, opt_mode="mse", config=None, args=args)
    units = [(n, m) for n, m in qnn.model.named_children() if isinstance(m, (QuantModule, BaseQuantBlock))]
    assert [n for n, _ in units[:2]] == ["g_a0", "g_a1"] and isinstance(units[1][1], QuantRSTB)
    layer_reconstruction(qnn, units[0][1], units[0][0], **kwargs)
    assert units[0][1].act_quantizer.act_frozen()
    name, u = units[1]
    (inp_q, _), _ = save_inp_oup_data(qnn, u, cali, asym=True, act_quant=True, batch_size=n_img, input_prob=True)
    block_reconstruction(qnn, u, name, **kwargs)
    attns = [m for m in u.modules() if isinstance(m, QuantWindowAttention)]
    assert attns
    for a in attns:
        q = a.act_quantizer
        assert q.act_frozen() and sorted(q.act_range) == [0, 1] and q.act_hist == {} and q.act_cand == {}
        assert q.act_range[0].numel() == 2 * a.num_heads and q.act_range[1].numel() == 2 * a.dim
        assert sorted(q.act_stats) == [0, 1] and q.act_stats[0]["err"].numel() == a.num_heads and q.act_stats[1]["err"].numel() == a.dim
    assert _check_auto_unit(u, inp_q, n_img, 8) >= 2 * len(attns)
    rep = qnn.act_report()
    assert list(rep) == list(qnn.act_ranges()) and len(rep) >= 2 * len(attns) + 1


@pytest.mark.parametrize("how", ["max", "auto"])
def test_report_of_the_frozen_ranges(how):
    """`act_report=True`: the report lists exactly the sites of `act_ranges()`; n is the pixels the site saw; sqnr_db is finite and
    positive on non-constant channels; the report survives a pickle round trip and .to('cpu'); without `act_report` nothing is recorded
    and the frozen ranges are the same bits.
    With 'max' no value is clipped, at EVERY site of the two units: a unit's four cached inputs are one batch here, so the observing
    pass quantised every tensor dynamically on the very min | max that was then frozen, the report pass's static outputs are the same
    bits (test_static_equals_dynamic_on_the_tensor_it_was_calibrated_on), and every site sees in the report pass exactly the values
    whose min | max it froze.  (With several batches this holds only for the sites that read the unit's cached input directly: the
    others observed values behind per-batch dynamic grids.)"""
    from quantization import block_reconstruction
    from quantization.export import activation_report
    from quantization.utils import save_inp_oup_data
    bits = 4
    qnn, cali, units, kwargs, g, N = _toy(bits=bits, act_mode="static", act_range=how, act_report=True, timing=[])
    inputs = []
    for name, u in units[:2]:
        (inp_q, _), _ = save_inp_oup_data(qnn, u, cali, asym=True, act_quant=True, batch_size=4, input_prob=True)
        inputs.append(inp_q)
        block_reconstruction(qnn, u, name, **kwargs)
        _expect_frozen(u, N)
    assert all("act_s" in t and t["act_s"] >= 0 for t in kwargs["args"].timing)
    rep = activation_report(qnn)
    ranges = qnn.act_ranges()
    assert list(rep) == list(ranges) and len(rep) >= 5 and list(qnn.act_report()) == list(rep)
    # the pixels every site saw: one more pass by hand over the frozen unit
    pixels = {}
    for (name, u), inp_q in zip(units[:2], inputs):
        seen = {}
        quants = _run_w8a8(u, inp_q, 4, seen=seen)
        qnames = {id(q): nm for nm, q in qnn.act_quantizers()}
        for (i, site), xs in seen.items():
            nm = qnames[id(quants[i])]
            pixels[nm if site == 0 else f"{nm}#{site}"] = (torch.cat([t.reshape(-1, t.shape[-1]) for t in xs]), quants[i].act_range[site])
    assert sorted(pixels) == sorted(rep)
    from hipops import ops
    for nm, r in rep.items():
        xs, rng = pixels[nm]
        c = r["channels"]
        assert r["n"] == xs.shape[0] and r["n_bits"] == bits and c == xs.shape[1] == ranges[nm][0].numel()
        assert all(r[f].numel() == c and r[f].device.type == "cpu" for f in ("err", "energy", "clip_lo", "clip_hi", "sqnr_db", "clipped_share"))
        assert r["clip_lo"].dtype == torch.int32 and r["sqnr_db"].dtype == torch.float64
        assert torch.equal(r["clip_lo"].long(), (xs < rng[:c]).sum(0).cpu()) and torch.equal(r["clip_hi"].long(), (xs > rng[c:]).sum(0).cpu())
        assert torch.equal(r["clipped_share"], (r["clip_lo"].double() + r["clip_hi"].double()) / r["n"])
        want = _err64(ops, xs, rng, bits).cpu()
        assert _rel_err(r["err"].double(), want) <= 1e-4 and _rel_err(r["energy"].double(), (xs.double() ** 2).sum(0).cpu()) <= 1e-4
        if how == "max":
            assert int(r["clip_lo"].sum()) == 0 and int(r["clip_hi"].sum()) == 0
        live = (xs.amax(0) > xs.amin(0)).cpu() & (r["err"] > 0)
        assert bool(live.any()) and bool(torch.isfinite(r["sqnr_db"][live]).all()) and bool((r["sqnr_db"][live] > 0).all())
        assert bool((r["sqnr_db"][r["err"] == 0] == float("inf")).all())
    if how == "auto":
        assert sum(int(r["clip_lo"].sum()) + int(r["clip_hi"].sum()) for r in rep.values()) > 0
    buf = io.BytesIO()
    torch.save(qnn, buf)
    buf.seek(0)
    rep2 = activation_report(torch.load(buf, weights_only=False).to("cpu"))
    assert list(rep2) == list(rep)
    for nm in rep:
        assert rep2[nm]["n"] == rep[nm]["n"] and all(torch.equal(rep2[nm][f], rep[nm][f]) for f in ("err", "energy", "clip_lo", "clip_hi", "sqnr_db"))
    # without the report: nothing recorded, the same frozen bits
    qnn0, cali0, units0, kwargs0, _, _ = _toy(bits=bits, act_mode="static", act_range=how)
    for name, u in units0[:2]:
        block_reconstruction(qnn0, u, name, **kwargs0)
    assert activation_report(qnn0) == {}
    a, b = _frozen(units[:2]), _frozen(units0[:2])
    assert len(a) == len(b) and all(sorted(x) == sorted(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- the modes that were there
def _dp_unit():
    """a trained ResidualBlock unit (N = 16, nearest-rounded 8-bit weights, 4-bit static activation grid) and 8 inputs of 16^2: the same
    on every rank"""
    import lic
    from helpers import WQ
    from quantization import BaseQuantBlock, QuantModule
    from quantization.quant_block import QuantRB
    torch.manual_seed(77)
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False, "dynamic_bits": 4, "act_mode": "static"}
    unit = QuantRB(lic.ResidualBlock(16, 16), WQ, aq).cuda().eval()
    x = torch.randn(8, 16, 16, 16, generator=torch.Generator().manual_seed(78)).cuda()
    unit.set_quant_state(False, False)
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.trained = True
    return unit, x


@pytest.mark.parametrize("how", ["max", "l2", "percentile", "hist_mse"])
def test_default_flow_did_not_move(how):
    """The four modes that were there freeze what they froze: `calibrate_act_ranges` against the same passes made by hand through the
    quantiser's phases, with the selection RESTATED here -- the observed range; the 'l2' clipping as `act_freeze` held it before the
    helper (lo * s | hi * s put back on an end that left the observed range); `ops.act_percentile_select` / `ops.act_hist_mse_select` on
    the recounted histograms (their own tests pin them) -- and no statistics are recorded."""
    from hipops import ops
    from quantization.recon import calibrate_act_ranges
    unit, x = _dp_unit()
    calibrate_act_ranges(unit, x, how, batch=4, percentile=99.0)
    _, quants = _unit_quants(unit)
    got = [{k: r.clone() for k, r in q.act_range.items()} for q in quants]
    assert sum(len(r) for r in got) >= 3
    assert all(getattr(q, "act_stats", {}) == {} and q.act_cand == {} and q.act_clip == {} and q.act_obs == {} for q in quants)
    _run_w8a8(unit, x, 4, prepare=lambda qs: [q.act_observe() for q in qs])
    obs = [{k: r.clone() for k, r in q.act_range.items()} for q in quants]
    if how == "l2":
        _run_w8a8(unit, x, 4, prepare=lambda qs: [q.act_search() for q in qs if q.act_range])
    elif how != "max":
        _run_w8a8(unit, x, 4, prepare=lambda qs: [q.act_histogram(99.0, rule="mse" if how == "hist_mse" else "percentile") for q in qs if q.act_range])
    moved = 0
    for q, mine, o in zip(quants, got, obs):
        assert sorted(mine) == sorted(o)
        for k, rng in o.items():
            c = rng.numel() // 2
            if how == "max":
                want = rng
            elif how == "l2":
                table = torch.tensor([1.0 - 0.05 * i for i in range(10)], dtype=torch.float32, device="cuda")
                s = table[q.act_err[k].argmin(dim=1)]
                lo, hi = torch.maximum(rng[:c] * s, rng[:c]), torch.minimum(rng[c:] * s, rng[c:])
                keep = lo > hi
                want = torch.cat([torch.where(keep, rng[:c], lo), torch.where(keep, rng[c:], hi)])
            elif how == "percentile":
                want = ops.act_percentile_select(q.act_hist[k], rng, 1.0 - 99.0 / 100.0)
            else:
                want = ops.act_hist_mse_select(q.act_hist[k], rng, 4)
            assert torch.equal(mine[k], want), (how, k)
            moved += int(not torch.equal(want, rng))
    assert (moved > 0) == (how != "max")


# ----------------------------------------------------------------------------- two ranks on one GPU
def _dp_calibrate(unit, x):
    """-> (the ranges 'auto' freezes, the ranges 'hist_mse' freezes, the statistics of a report pass over the latter), per quantiser"""
    from quantization.recon import calibrate_act_ranges, report_act_ranges
    _, quants = _unit_quants(unit)
    calibrate_act_ranges(unit, x, "auto", batch=4)
    auto = [{k: r.cpu() for k, r in q.act_range.items()} for q in quants]
    calibrate_act_ranges(unit, x, "hist_mse", batch=4)
    report_act_ranges(unit, x, batch=4)
    mse = [{k: r.cpu() for k, r in q.act_range.items()} for q in quants]
    stats = [{k: {f: (v.cpu() if torch.is_tensor(v) else v) for f, v in st.items()} for k, st in q.act_stats.items()} for q in quants]
    return auto, mse, stats


def _plain(obj, back=False):
    """tensors <-> numpy arrays, through lists, tuples and dicts: a queue hands a tensor over through a descriptor of the sending process,
    which may have ended by the time the parent unpickles; an array travels by value"""
    if isinstance(obj, dict):
        return {k: _plain(v, back) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_plain(v, back) for v in obj)
    if back and isinstance(obj, np.ndarray):
        return torch.from_numpy(obj)
    return obj.numpy() if torch.is_tensor(obj) else obj


def _dp_rank(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "rdo-ptq_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from quantization import dp
        unit, x = _dp_unit()
        lo, hi = dp.shard_range(x.shape[0], rank, world)
        out_q.put((rank, _plain(_dp_calibrate(unit, x[lo:hi].contiguous()))))
        dist.barrier()
    except BaseException as e:          # the parent must not wait out its queue timeout for a rank that failed
        out_q.put(("error", f"rank {rank}: {e!r}"))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_freeze_the_same_ranges_and_count_like_one():
    """Two processes on cuda:0 over gloo, each on its half of the inputs.  Under 'auto' both ranks pick from the same reduced sums: they
    freeze identical ranges (the fp32 sums of two ranks need not be the bits of one process, so these are compared between the ranks).
    The reported COUNTS are compared with one process on all inputs where the scored ranges are its ranges bit for bit: behind
    'hist_mse' (integer histograms: test_two_ranks_select_the_same_ranges_as_one); clip_lo, clip_hi and n are then exactly its counts,
    err and energy within 1e-4."""
    unit, x = _dp_unit()
    ref_auto, ref_mse, ref_stats = _dp_calibrate(unit, x)
    assert sum(len(r) for r in ref_auto) >= 3 and sum(len(s) for s in ref_stats) == sum(len(r) for r in ref_mse)
    assert sum(int(st["clip_lo"].sum() + st["clip_hi"].sum()) for s in ref_stats for st in s.values()) > 0
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(2):
            rk, val = q.get(timeout=180)
            assert rk != "error", val
            got[rk] = _plain(val, back=True)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    (auto0, mse0, stats0), (auto1, mse1, stats1) = got[0], got[1]
    assert len(auto0) == len(auto1) == len(ref_auto)
    for a, b, want in zip(auto0, auto1, ref_auto):
        assert sorted(a) == sorted(b) == sorted(want) and all(torch.equal(a[k], b[k]) for k in a)
    for stats, mse in ((stats0, mse0), (stats1, mse1)):
        for mine, rng, want, want_rng in zip(stats, mse, ref_stats, ref_mse):
            assert sorted(mine) == sorted(want)
            for k in want:
                assert torch.equal(rng[k], want_rng[k])
                assert mine[k]["n"] == want[k]["n"] == x.shape[0] * 16 * 16
                assert torch.equal(mine[k]["clip_lo"], want[k]["clip_lo"]) and torch.equal(mine[k]["clip_hi"], want[k]["clip_hi"])
                assert _rel_err(mine[k]["err"].double(), want[k]["err"].double()) <= 1e-4
                assert _rel_err(mine[k]["energy"].double(), want[k]["energy"].double()) <= 1e-4
