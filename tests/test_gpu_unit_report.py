"""The per-unit output error report on the GPU: `ops.pair_moments` (rdo_pair_moments of csrc/actquant.hip) against a float64 restatement,
its exact cases and its NaN containment; `args.unit_report` / `recon.report_unit` on toy Cheng2020 units, a Swin unit, frozen static
activation ranges and two data-parallel ranks.

Tolerance of the kernel (every test that says "the bound"): err and energy relative to their float64 values, shift relative to float64
sum |d|, the worst over the channels and the three sums.  A float32 restatement of the same sums on the SAME inputs is measured the
same way -- a numpy float32 sequential chain of 1024 pixels followed by pairwise sums, and numpy's own float32 `np.sum` of each
channel; the larger of the two -- and the kernel is allowed 4 x that (the project's convention).  Measured on an MI355X, kernel |
allowed:
    (1, 4)            3.2e-8   | 1.3e-7     (one term per sum: the kernel gives the restatement's bits)
    (7, 3)            6.5e-8   | 2.6e-7     (one workgroup, one pixel a lane: the restatement's order and bits)
    (257, 192)        1.2e-7   | 3.4e-6
    (16387, 192)      1.2e-7   | 1.8e-6
    (35, 1280)        1.6e-7   | 1.3e-6
    (4096, 320)       1.3e-7   | 3.5e-6
    (1024, 192) off   1.1e-7   | 5.5e-6
    (2**25 + 5, 2)    7.3e-8   | 7.6e-6
"""
import copy
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

FACTOR = 4.0
STATES = ("nearest", "learned")


# ----------------------------------------------------------------------------- restatements
def _ref64(a, b):
    """float64 restatement on the tensors' device: d formed in float32, squared and summed in float64 -> ([3, C] = shift | err | energy,
    sum |d| [C])"""
    a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    d = (a2 - b2).double()
    return torch.stack([d.sum(0), (d * d).sum(0), (a2.double() ** 2).sum(0)]), d.abs().sum(0)


def _ratio(got, ref, absd):
    """worst over the channels and the three sums of |got - ref| / scale, scale = sum |d| for shift, the float64 value for err and energy
    (a channel whose scale is 0 must match exactly: it counts as 0 then, as inf otherwise)"""
    got, ref, absd = (t.detach().double().cpu() for t in (got, ref, absd))
    scale = torch.stack([absd, ref[1], ref[2]])
    diff = (got - ref).abs()
    r = torch.where(scale > 0, diff / scale.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))
    assert not bool(torch.isnan(r).any())
    return float(r.max())


def _chain_sum32(t):
    """float32 [n, C] -> [C]: sequential float32 sums of 1024 consecutive pixels, then pairwise float32 sums of those"""
    n, C = t.shape
    m = -(-n // 1024)
    if m * 1024 != n:
        t = np.concatenate([t, np.zeros((m * 1024 - n, C), np.float32)])
    t = t.reshape(m, 1024, C)
    acc = np.zeros((m, C), np.float32)
    for j in range(1024):
        acc = acc + t[:, j, :]
    while acc.shape[0] > 1:
        if acc.shape[0] % 2:
            acc = np.concatenate([acc, np.zeros((1, C), np.float32)])
        acc = acc[0::2] + acc[1::2]
    assert acc.dtype == np.float32
    return acc[0]


def _restated32(a, b):
    """-> the two float32 restatements [3, C] (chain of 1024 + pairwise; np.sum of each channel) as float64 CPU tensors"""
    an = a.reshape(-1, a.shape[-1]).cpu().numpy()
    bn = b.reshape(-1, b.shape[-1]).cpu().numpy()
    d = an - bn
    terms = [d, d * d, an * an]
    assert all(t.dtype == np.float32 for t in terms)
    chain = np.stack([_chain_sum32(t) for t in terms])
    plain = np.stack([np.sum(np.ascontiguousarray(t.T), axis=1, dtype=np.float32) for t in terms])
    return torch.from_numpy(chain.astype(np.float64)), torch.from_numpy(plain.astype(np.float64))


def _allowed(a, b, ref=None):
    """the bound for these inputs: FACTOR x the worse of the two float32 restatements, measured like the kernel"""
    ref, absd = _ref64(a, b) if ref is None else ref
    return FACTOR * max(_ratio(r, ref, absd) for r in _restated32(a, b))


def _pair(npix, C, seed, device="cuda", err=0.02):
    """a = channels of different scale and offset, b = a + a small error with a per-channel mean (a quantised output next to its
    full-precision one)"""
    g = torch.Generator(device=device).manual_seed(seed)
    scale = 0.25 + 2.0 * torch.rand(C, generator=g, device=device)
    a = torch.randn(npix, C, generator=g, device=device) * scale + (torch.rand(C, generator=g, device=device) - 0.5)
    e = err * scale * (torch.rand(npix, C, generator=g, device=device) - 0.5 + 0.2 * (torch.rand(C, generator=g, device=device) - 0.5))
    return a.contiguous(), (a - e).contiguous()


def _off_by_one_float(x):
    """the same values at an address one float past a 16-byte boundary: the W = 1 path although C % 4 == 0"""
    buf = torch.empty(x.numel() + 4, device=x.device, dtype=x.dtype)
    assert buf.data_ptr() % 16 == 0
    y = buf[1:1 + x.numel()].view(x.shape)
    y.copy_(x)
    assert y.data_ptr() % 16 == 4 and y.is_contiguous()
    return y


def _measure(ops, a, b, what):
    """-> (kernel result, float64 reference, sum |d|, allowed); prints kernel | allowed before anything is asserted"""
    ref, absd = _ref64(a, b)
    got = ops.pair_moments(a, b)
    torch.cuda.synchronize()
    assert got.shape == (3, a.shape[-1]) and got.dtype == torch.float32 and got.is_cuda
    allowed = _allowed(a, b, (ref, absd))
    print(f"pair_moments {what}: kernel {_ratio(got, ref, absd):.3e} | allowed {allowed:.3e}")
    return got, ref, absd, allowed


# ----------------------------------------------------------------------------- 1. the kernel against the restatement
SHAPES = [(1, 4), (7, 3), (257, 192), (16387, 192), (35, 1280), (4096, 320)]


@pytest.mark.parametrize("npix,C", SHAPES)
def test_kernel_matches_the_float64_restatement(npix, C):
    from hipops import ops
    a, b = _pair(npix, C, seed=1000 + npix + C)
    got, ref, absd, allowed = _measure(ops, a, b, (npix, C))
    assert _ratio(got, ref, absd) <= allowed
    # channels-last of any rank: the pixels are all the leading dimensions
    if npix % 7 == 0:
        assert torch.equal(ops.pair_moments(a.view(7, npix // 7, C), b.view(7, npix // 7, C)), got)
    # `out` is added to
    acc = got.clone()
    assert ops.pair_moments(a, b, out=acc) is acc
    assert torch.equal(acc, got + got)


def test_kernel_off_alignment_takes_the_scalar_path():
    """both operands one float past a 16-byte boundary, C % 4 == 0: W = 1 (one pixel lane a workgroup at this width, another
    order of the additions than W = 4); the same sums within the bound"""
    from hipops import ops
    a, b = _pair(1024, 192, seed=5)
    a1, b1 = _off_by_one_float(a), _off_by_one_float(b)
    got, ref, absd, allowed = _measure(ops, a1, b1, "(1024, 192) off alignment")
    assert _ratio(got, ref, absd) <= allowed
    for x, y in ((a1, b), (a, b1)):                       # one operand off alignment is enough
        assert _ratio(ops.pair_moments(x, y), ref, absd) <= allowed


def test_kernel_closes_the_chain_beyond_1024_pixels_a_thread():
    """(2**25 + 5, 2): 128 pixel lanes x 256 workgroups walk 1024 pixels and a few each, so the running sums are closed into the second
    ones; the reference is formed with torch float64 on the device"""
    from hipops import ops
    npix, C = 2 ** 25 + 5, 2
    a, b = _pair(npix, C, seed=77)
    got, ref, absd, allowed = _measure(ops, a, b, (npix, C))
    assert _ratio(got, ref, absd) <= allowed


def test_kernel_chain_closure_loses_nothing():
    """(2**25 + 5, 2) again, exactly: channel 0 holds a = 1 on the pixels p % 4 == 0, channel 1 a = 2 on p % 4 == 1, b = 0.  A thread's
    pixels are 32768 apart, so a thread sees only ones (or twos, or zeros), 1024 or 1025 of them: its running sum is closed into the
    second one.  The counts are 2**23 + 2 and 2**23 + 1: every partial sum is an integer (a multiple of 4 for the squares of channel 1)
    of at most 24 bits, so all three sums are exact, and a closure that drops what it closed is 1024 short per thread"""
    from hipops import ops
    npix = 2 ** 25 + 5
    p = torch.arange(npix, device="cuda") % 4
    a = torch.stack([(p == 0).float(), 2.0 * (p == 1).float()], dim=1).contiguous()
    got = ops.pair_moments(a, torch.zeros_like(a))
    n0, n1 = 2 ** 23 + 2, 2 ** 23 + 1
    assert int((p == 0).sum()) == n0 and int((p == 1).sum()) == n1
    assert got.tolist() == [[float(n0), float(2 * n1)], [float(n0), float(4 * n1)], [float(n0), float(4 * n1)]]


# ----------------------------------------------------------------------------- 2. exact cases
def test_equal_operands_give_zero_shift_and_error():
    from hipops import ops
    a, _ = _pair(16387, 192, seed=9)
    b = a.clone()
    got, ref, absd, allowed = _measure(ops, a, b, "b = a (16387, 192)")
    assert bool((got[0] == 0).all()) and bool((got[1] == 0).all())
    assert _ratio(got, ref, absd) <= allowed


@pytest.mark.parametrize("npix,C", [(16387, 192), (35, 1280)])
def test_every_pixel_is_counted_once(npix, C):
    """a - b = 0.25 everywhere with a on a 2^-4 grid in [-2, 2]: every d is 0.25 and every d^2 is 2^-4 exactly, every partial sum is a
    multiple of 2^-4 below 2^24 * 2^-4: exactly representable, so shift == n / 4 and err == n / 16 bit for bit"""
    from hipops import ops
    g = torch.Generator().manual_seed(3)
    a = (torch.randint(-32, 33, (npix, C), generator=g).float() / 16).cuda()
    b = a - 0.25
    assert bool(((a - b) == 0.25).all())
    got = ops.pair_moments(a, b)
    assert bool((got[0] == npix / 4).all()) and bool((got[1] == npix / 16).all())
    assert torch.equal(got[2].double(), (a.double() ** 2).sum(0))        # multiples of 2^-8 below 2^24 * 2^-8: exact too


# ----------------------------------------------------------------------------- 3. NaN containment
def test_a_nan_stays_in_its_channel():
    from hipops import ops
    a, b = _pair(4099, 192, seed=21)
    clean = ops.pair_moments(a, b)
    for which in (0, 1):
        x, y = a.clone(), b.clone()
        (x, y)[which][1234, 5] = float("nan")
        got = ops.pair_moments(x, y)
        assert bool(torch.isnan(got[:2, 5]).all()) and bool(torch.isnan(got[2, 5])) == (which == 0)
        keep = torch.arange(192, device="cuda") != 5
        assert torch.equal(got[:, keep], clean[:, keep])
    x = a.clone()
    x[1234, 5] = float("nan")
    assert bool(torch.isnan(ops.pair_moments(x, b)[:, 5]).all())          # a NaN in `a`: all three sums of the channel


# ----------------------------------------------------------------------------- the calibration flow
def _toy(**extra):
    """the toy Cheng2020 of the activation-quantiser tests (N = 8, four 64^2 images), seeded -> (model, images, units of g_a, kwargs)"""
    import lic
    from quantization import QuantModel
    torch.manual_seed(1005)
    N, n_img, B, iters = 8, 4, 2, 20
    model = lic.Cheng2020Anchor(N=N).cuda().eval()
    g = torch.Generator().manual_seed(13)
    cali = torch.rand(n_img, 3, 64, 64, generator=g).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
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
    return qnn, cali, dict(qnn.model.g_a.named_children()), kwargs


def _quant_modules(unit):
    from quantization import QuantModule
    return [m for m in unit.modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def _run(unit, inp_q, batch):
    """the unit over its cached inputs, batch for batch, in the state it is in -> list of channels-last outputs"""
    from quantization.quant_block import QuantRSTB
    from quantization.quant_layer import _nhwc
    outs = []
    with torch.no_grad():
        for i in range(0, inp_q.shape[0], batch):
            h = inp_q[i:i + batch]
            outs.append(_nhwc(unit(h, (h.shape[2], h.shape[3])) if isinstance(unit, QuantRSTB) else unit(h)).clone())
    return outs


def _moments_by_hand(outs, out_fp, batch):
    """`ops.pair_moments` of every batch's outputs against the full-precision ones, added in float64 -> ([3, C] float64 on the CPU, pixels)"""
    from hipops import ops
    from quantization.quant_layer import _nhwc
    acc, n = None, 0
    for k, out in enumerate(outs):
        ref = _nhwc(out_fp[k * batch:(k + 1) * batch])
        mom = ops.pair_moments(ref, out).double()
        acc = mom if acc is None else acc + mom
        n += ref.numel() // ref.shape[-1]
    return acc.cpu(), n


def _nearest_copy(unit):
    """a copy of the unit whose trained weights are overwritten with their round-to-nearest values on the quantisers' delta | zero point,
    (clamp(floor(w / delta) + (frac >= 0.5) + z, 0, n_levels - 1) - z) * delta with frac = w / delta - floor(w / delta) in fp32 (a tie
    rounds up: the rule `report_unit` states), and run as plain weights (weight quantisation off on those modules) -> (copy, weights moved
    against the learned rounding)"""
    from quantization.quantizer import AdaRoundQuantizer
    twin = copy.deepcopy(unit)
    moved = n = 0
    for m in _quant_modules(twin):
        q = m.weight_quantizer
        if not isinstance(q, AdaRoundQuantizer):           # not trained: the same weights in both states
            continue
        w = m.weight.detach()
        r = w / q.delta
        fl = torch.floor(r)
        up = ((r - fl) >= 0.5).to(w.dtype)
        moved += int((up != (q.alpha.detach() >= 0).to(w.dtype)).sum())
        n += up.numel()
        m.org_weight = ((torch.clamp(fl + up + q.zero_point, 0, q.n_levels - 1) - q.zero_point) * q.delta).contiguous()
        m.org_bias = None if m.bias is None else m.bias.detach().clone()
        m.use_weight_quant = False
        m.drop_weight_pack()
    assert n > 0
    return twin, moved


def _state(unit):
    """flags, alpha, delta, zero point and `_weight_state()` of every module of the unit, the frozen ranges of its quantisers"""
    from quantization import BaseQuantBlock, QuantModule
    out = []
    for name, m in unit.named_modules():
        if not isinstance(m, (QuantModule, BaseQuantBlock)):
            continue
        row = {"name": name, "flags": (m.use_weight_quant, m.use_act_quant, m.trained),
               "ranges": {k: r.clone() for k, r in m.act_quantizer.act_range.items()},
               "act_stats": sorted(getattr(m.act_quantizer, "act_stats", None) or {})}
        if isinstance(m, QuantModule) and m.org_weight is not None:
            q = m.weight_quantizer
            row.update(alpha=q.alpha.detach().clone(), alpha_id=id(q.alpha), delta=q.delta.clone(), zp=q.zero_point.clone(),
                       soft=q.soft_targets, wstate=m._weight_state())
        out.append(row)
    return out


def _same_state(x, y):
    assert len(x) == len(y) and len(x) > 0
    for r, s in zip(x, y):
        assert sorted(r) == sorted(s)
        for k in r:
            if torch.is_tensor(r[k]):
                assert torch.equal(r[k], s[k]), (r["name"], k)
            elif k == "ranges":
                assert sorted(r[k]) == sorted(s[k]) and all(torch.equal(r[k][i], s[k][i]) for i in r[k]), (r["name"], k)
            else:
                assert r[k] == s[k], (r["name"], k)


def _same_stats(x, y):
    assert x["name"] == y["name"] and x["n"] == y["n"]
    for state in STATES:
        for f in ("shift", "err", "energy"):
            assert x[state][f].dtype == torch.float64 and x[state][f].device.type == "cpu"
            assert torch.equal(x[state][f], y[state][f]), (state, f)


def _calibrate(which, **extra):
    """a fresh toy model whose named units of g_a are calibrated in order; a generator: after each unit -> (qnn, name, unit, inp_q,
    out_fp, cache batch), with the unit still in the state its loop and its report ran it in (the cache passes of a LATER unit switch a
    trained block wrapper's own flags off: utils.set_mode re-enables QuantModules only)"""
    from quantization import BaseQuantBlock, block_reconstruction, layer_reconstruction
    from quantization.utils import save_inp_oup_data
    qnn, cali, units, kwargs = _toy(**extra)
    static = extra.get("act_mode") == "static"
    batch = cali.shape[0] if static else 1                # `cache_bs` of recon._reconstruct
    for k, name in enumerate(which):
        u = units[name]
        torch.manual_seed(1005 + k)                       # the unit's mini-batch draws do not depend on what ran in between
        (inp_q, _), out_fp = save_inp_oup_data(qnn, u, cali, asym=True, act_quant=True, batch_size=batch, input_prob=True)
        (block_reconstruction if isinstance(u, BaseQuantBlock) else layer_reconstruction)(qnn, u, name, **kwargs)
        yield qnn, name, u, inp_q.clone(), out_fp.clone(), batch


def _check_unit_against_hand(u, name, inp_q, out_fp, batch, stats):
    """(b) and (c): both states of the recorded statistics against `ops.pair_moments` applied here, batch for batch -> weights the
    nearest rounding moves"""
    learned, n = _moments_by_hand(_run(u, inp_q, batch), out_fp, batch)
    twin, moved = _nearest_copy(u)
    nearest, n2 = _moments_by_hand(_run(twin, inp_q, batch), out_fp, batch)
    assert stats["name"] == name and stats["n"] == n == n2 == out_fp.numel() // out_fp.shape[1]
    for state, want in (("learned", learned), ("nearest", nearest)):
        got = torch.stack([stats[state][f] for f in ("shift", "err", "energy")])
        assert got.dtype == torch.float64 and got.device.type == "cpu"
        # exact: the nearest pass runs the quantiser's own kernel on a sign tensor, the copy holds the same fp32 expression evaluated by
        # torch; both go through the same weight pack
        assert torch.equal(got, want), (name, state)
    return moved


def test_flow_records_both_states_and_changes_nothing():
    """A block unit (g_a.0, a ResidualBlockWithStride with its GDN) and a layer unit (g_a.6) of the toy Cheng2020, W8A8 with dynamic
    activation grids, 20 iterations each, with and without `unit_report`:
    (a) alpha, delta, zero points, ranges and the unit's outputs on its cache are the same bits in both runs;
    (b) 'learned' is `ops.pair_moments` of unit(inp_q) against out_fp, batch for batch, exactly;
    (c) 'nearest' is the same for a copy of the unit that holds the round-to-nearest weights as plain weights: exactly (the pack path is
        the same);
    (d) `report_unit` leaves flags, alpha (the same Parameter objects) and `_weight_state()` as it found them, and gives the bits the
        flag gave.
    The sign of gain_db is not asserted: on a random-init model calibration is nearly a no-op."""
    from quantization.export import unit_report
    from quantization.recon import report_unit
    names = ["0", "6"]
    moved = 0
    for (qnn1, name, u1, inp1, fp1, batch), (qnn0, _, u0, inp0, fp0, _) in zip(_calibrate(names, unit_report=True),
                                                                              _calibrate(names, unit_report=False)):
        assert torch.equal(inp1, inp0) and torch.equal(fp1, fp0)
        assert getattr(u0, "unit_stats", None) is None and unit_report(qnn0) == {} and qnn0.unit_report() == {}
        # (a)
        _same_state([{k: v for k, v in r.items() if k not in ("alpha_id", "wstate")} for r in _state(u1)],
                    [{k: v for k, v in r.items() if k not in ("alpha_id", "wstate")} for r in _state(u0)])
        assert all(torch.equal(x, y) for x, y in zip(_run(u1, inp1, batch), _run(u0, inp0, batch)))
        # (b), (c)
        stats = u1.unit_stats
        moved += _check_unit_against_hand(u1, name, inp1, fp1, batch, stats)
        # (d)
        before = _state(u0)
        again = report_unit(u0, name, inp0, fp0, batch=batch)
        _same_state(before, _state(u0))
        _same_stats(again, stats)
        u0.__dict__.pop("unit_stats")
        # the read-out
        rep = qnn1.unit_report()
        assert list(rep) == names[:names.index(name) + 1]
        r = rep[name]
        C = fp1.shape[1]
        assert r["channels"] == C and r["n"] == stats["n"]
        for state in STATES:
            assert torch.equal(r["err"][state], stats[state]["err"]) and bool((r["err"][state] > 0).all())
            assert bool(((r["shift_share"][state] >= 0) & (r["shift_share"][state] <= 1)).all())
            assert bool(torch.isfinite(r["sqnr_db"][state]).all())
        assert torch.equal(r["gain_db"], r["sqnr_db"]["learned"] - r["sqnr_db"]["nearest"])
        print(f"unit {name}: sqnr nearest {r['total']['sqnr_db']['nearest']:.3f} dB, learned {r['total']['sqnr_db']['learned']:.3f} dB, "
              f"moved {moved}")
    assert moved > 0                                       # the two states differ in at least one weight: (c) is not (b) again


def test_report_matches_the_float64_restatement_of_the_cache():
    """the recorded sums of a unit against the float64 restatement over its whole cache: within the bound of these inputs"""
    from quantization.quant_layer import _nhwc
    (_, _, u, inp_q, out_fp, batch), = _calibrate(["0"], unit_report=True)
    a, b = _nhwc(out_fp), torch.cat(_run(u, inp_q, batch))
    ref, absd = _ref64(a, b)
    got = torch.stack([u.unit_stats["learned"][f] for f in ("shift", "err", "energy")])
    allowed = _allowed(a, b, (ref, absd))
    print(f"unit_stats learned: {_ratio(got, ref, absd):.3e} | allowed {allowed:.3e}")
    assert _ratio(got, ref, absd) <= allowed


# ----------------------------------------------------------------------------- 5. a Swin unit
def test_report_of_the_first_swin_unit_of_toy_lu2022():
    import lic
    from quantization import BaseQuantBlock, QuantModel, QuantModule, block_reconstruction, layer_reconstruction
    from quantization.quant_block import QuantRSTB
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
    n_img, B, iters = 4, 2, 6
    cali = torch.rand(n_img, 3, 64, 64, generator=g).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:B])
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Lu2022", unit_report=True)
    kwargs = dict(cali_data=cali, batch_size=B, iters=iters, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2),
                  warmup=0.2, act_quant=True, opt_mode="mse", config=None, args=args)
    units = [(n, m) for n, m in qnn.model.named_children() if isinstance(m, (QuantModule, BaseQuantBlock))]
    assert [n for n, _ in units[:2]] == ["g_a0", "g_a1"] and isinstance(units[1][1], QuantRSTB)
    layer_reconstruction(qnn, units[0][1], units[0][0], **kwargs)
    name, u = units[1]
    (inp_q, _), out_fp = save_inp_oup_data(qnn, u, cali, asym=True, act_quant=True, batch_size=1, input_prob=True)
    block_reconstruction(qnn, u, name, **kwargs)
    rep = qnn.unit_report()
    assert list(rep) == ["g_a0", "g_a1"]
    r = rep[name]
    assert out_fp.dim() == 4 and out_fp.shape[1] == cfg["embed_dim"]
    assert r["n"] == n_img * out_fp.shape[2] * out_fp.shape[3] and r["channels"] == cfg["embed_dim"]
    _check_unit_against_hand(u, name, inp_q, out_fp, 1, u.unit_stats)


# ----------------------------------------------------------------------------- 6. frozen static ranges
def test_report_runs_on_the_frozen_static_ranges():
    """act_mode='static', act_range='max', W8A8, the layer unit g_a.6: the report comes after freezing; both states run the frozen grid
    (the hand-made passes here do: they match exactly); `act_ranges()` is what a run without the report freezes, and `report_unit`
    leaves it alone"""
    from quantization.recon import report_unit
    extra = dict(act_mode="static", act_range="max")
    (qnn1, _, u1, inp1, fp1, batch), = _calibrate(["6"], unit_report=True, **extra)
    (qnn0, _, u0, inp0, fp0, _), = _calibrate(["6"], **extra)
    assert batch == 4 and u1.act_quantizer.act_frozen() and sorted(u1.act_quantizer.act_range) == [0]
    r1, r0 = qnn1.act_ranges(), qnn0.act_ranges()
    assert list(r1) == list(r0) and len(r1) == 1
    for k in r1:
        assert torch.equal(r1[k][0], r0[k][0]) and torch.equal(r1[k][1], r0[k][1]) and r1[k][2] == r0[k][2]
    assert qnn1.act_report() == {} and list(qnn1.unit_report()) == ["6"] and qnn0.unit_report() == {}
    _check_unit_against_hand(u1, "6", inp1, fp1, batch, u1.unit_stats)
    # the frozen grid is in the outputs both passes measured: every output value of a channel is one of its 256 levels
    rng = u1.act_quantizer.act_range[0]
    C = rng.numel() // 2
    out = torch.cat(_run(u1, inp1, batch)).reshape(-1, C)
    lo, w = rng[:C], torch.clamp(rng[C:] - rng[:C], min=1e-6)
    lev = (out - lo) / w * 255.0
    assert bool(((lev - lev.round()).abs() <= 1e-2).all()) and bool((lev >= -1e-2).all()) and bool((lev <= 255.01).all())
    before = _state(u0)
    again = report_unit(u0, "6", inp0, fp0, batch=batch)
    _same_state(before, _state(u0))
    _same_stats(again, u1.unit_stats)
    r2 = qnn0.act_ranges()
    assert all(torch.equal(r2[k][0], r0[k][0]) and torch.equal(r2[k][1], r0[k][1]) for k in r0)


# ----------------------------------------------------------------------------- 7. two ranks on one GPU
def _dp_unit():
    """a trained ResidualBlock unit (N = 16, 8-bit AdaRound weights whose alpha is drawn, not trained; dynamic 8-bit activation grids),
    8 inputs of 16^2 and its full-precision outputs: the same on every rank"""
    import lic
    from helpers import AQ, WQ
    from quantization import BaseQuantBlock, QuantModule
    from quantization.quant_block import QuantRB
    from quantization.quantizer import AdaRoundQuantizer
    torch.manual_seed(77)
    unit = QuantRB(lic.ResidualBlock(16, 16), WQ, AQ).cuda().eval()
    x = torch.randn(8, 16, 16, 16, generator=torch.Generator().manual_seed(78)).cuda()
    unit.set_quant_state(False, False)
    with torch.no_grad():
        out_fp = unit(x).clone()
    unit.set_quant_state(True, False)
    with torch.no_grad():
        unit(x[:1])                                        # the weight quantisers take their scales
    g = torch.Generator().manual_seed(79)
    for m in unit.modules():
        if isinstance(m, QuantModule) and m.org_weight is not None:
            ada = AdaRoundQuantizer(uaq=m.weight_quantizer, round_mode="learned_hard_sigmoid", weight_tensor=m.org_weight.data)
            with torch.no_grad():
                ada.alpha.add_(torch.randn(ada.alpha.shape, generator=g).to(ada.alpha.device))
            m.weight_quantizer = ada
            m.drop_weight_pack()
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.trained = True
    unit.set_quant_state(True, True)
    return unit, x, out_fp


def _plain(stats, back=False):
    """the statistics with numpy arrays for tensors (a queue hands a tensor over through a descriptor of the sending process, which may
    have ended by the time the parent unpickles; an array travels by value), and back"""
    conv = (lambda v: torch.from_numpy(v)) if back else (lambda v: v.numpy())
    return {k: ({f: conv(v) for f, v in s.items()} if k in STATES else s) for k, s in stats.items()}


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
        from quantization.recon import report_unit
        unit, x, out_fp = _dp_unit()
        lo, hi = dp.shard_range(x.shape[0], rank, world)
        stats = report_unit(unit, "rb", x[lo:hi].contiguous(), out_fp[lo:hi].contiguous(), batch=4)
        out_q.put((rank, _plain(stats)))
        dist.barrier()
    except BaseException as e:          # the parent must not wait out its queue timeout for a rank that failed
        out_q.put(("error", f"rank {rank}: {e!r}"))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_statistics_of_one():
    """Two processes on cuda:0 over gloo, each on its half of the inputs: both hold identical `unit_stats`, `n` is the global pixel
    count, and the sums are those of one process on all inputs within the bound of these inputs (in fact the same bits: a rank's one
    batch is a batch of the single process, and the float64 sum of two terms does not depend on their order)"""
    from quantization.quant_layer import _nhwc
    from quantization.recon import report_unit
    unit, x, out_fp = _dp_unit()
    want = report_unit(unit, "rb", x, out_fp, batch=4)
    assert want["n"] == 8 * 16 * 16
    assert not torch.equal(want["nearest"]["err"], want["learned"]["err"])
    a = _nhwc(out_fp)
    bounds = {}
    twin, moved = _nearest_copy(unit)
    assert moved > 0
    for state, mod in (("learned", unit), ("nearest", twin)):
        b = torch.cat(_run(mod, x, 4))
        ref, absd = _ref64(a, b)
        bounds[state] = (_allowed(a, b, (ref, absd)), absd.cpu())
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
    _same_stats(got[0], got[1])
    assert got[0]["n"] == want["n"] and got[0]["name"] == "rb"
    for state in STATES:
        mine = torch.stack([got[0][state][f] for f in ("shift", "err", "energy")])
        ref = torch.stack([want[state][f] for f in ("shift", "err", "energy")])
        allowed, absd = bounds[state]
        ratio = _ratio(mine, ref, absd)
        print(f"two ranks, {state}: {ratio:.3e} | allowed {allowed:.3e}")
        assert ratio <= allowed
