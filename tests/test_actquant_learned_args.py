"""CPU checks of the learned activation ranges' surface: `act_range='learned'` and its two optional arguments are validated before any
work is done, Swin units are refused up front, the quantiser's "learn" phase brackets leaf ranges and the observed max ranges, a
quantiser pickled before `act_ste` existed behaves as before, only a frozen quantiser with `act_ste` and a tracked input goes on
torch's tape, and the header declares the new entries."""
import os
import pickle
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("rdo_actquant_static_bwd", "rdo_actquant_static_bwd_workspace", "rdo_act_range_step")


def _frozen(channels=3, bits=8, sites=(0,)):
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(n_bits=8, channel_wise=True, scale_method="max", act=True, dynamic_bits=bits, act_mode="static")
    for s in sites:
        lo = -torch.arange(1, channels + 1, dtype=torch.float32) - s
        q.act_range[s] = torch.cat([lo, -lo * 2])
    q.act_phase = "frozen"
    return q


def test_header_declares_every_new_export_and_they_validate_arguments():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_hip.h")).read()
    declared = set(re.findall(r"\b(rdo_[a-z0-9_]+)\s*\(", hdr))
    h = L.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(h, name)
    assert h.rdo_actquant_static_bwd(None, None, 4, 4, 8, None, None, None, None, None) != 0
    assert h.rdo_act_range_step(None, None, None, None, None, 4, 1, 1e-3, None) != 0
    assert h.rdo_actquant_static_bwd_workspace(0) == 0 and h.rdo_actquant_static_bwd_workspace(192) >= 2 * 192


def test_learned_is_an_accepted_act_range():
    from quantization.recon import _act_args, _act_learn_args
    assert _act_args(types.SimpleNamespace(act_mode="static", act_range="learned")) == ("static", "learned")
    assert _act_args(types.SimpleNamespace(act_mode="static", act_range="learned", act_iters=7, act_lr=0.5)) == ("static", "learned")
    assert _act_learn_args(None) == (500, 1e-3) and _act_learn_args(types.SimpleNamespace()) == (500, 1e-3)
    assert _act_learn_args(types.SimpleNamespace(act_iters=7, act_lr=1)) == (7, 1.0)
    for how in ("learn", "Learned", "lsq", ""):
        with pytest.raises(ValueError, match="act_range"):
            _act_args(types.SimpleNamespace(act_mode="static", act_range=how))


@pytest.mark.parametrize("kw", [dict(act_iters=0), dict(act_iters=-3), dict(act_iters=2.5), dict(act_iters=True), dict(act_iters="5"),
                                dict(act_lr=0.0), dict(act_lr=-1e-3), dict(act_lr=float("inf")), dict(act_lr=float("nan")),
                                dict(act_lr="1e-3"), dict(act_lr=None)])
def test_act_iters_and_act_lr_are_refused_before_any_work(kw):
    from quantization import block_reconstruction, layer_reconstruction
    from quantization.recon import _act_args, learn_act_ranges
    with pytest.raises(ValueError, match="act_iters|act_lr"):
        _act_args(types.SimpleNamespace(act_mode="static", act_range="learned", **kw))
    for recon in (layer_reconstruction, block_reconstruction):            # refused before the model, the unit or a device is looked at
        with pytest.raises(ValueError, match="act_iters|act_lr"):
            recon(None, None, "0", torch.zeros(2, 3, 64, 64), batch_size=2, iters=1, act_quant=True,
                  args=types.SimpleNamespace(task_loss=2.0, act_mode="static", act_range="learned", **kw))
    with pytest.raises(ValueError, match="act_iters|act_lr"):
        learn_act_ranges(torch.nn.Identity(), torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4), kw.get("act_iters", 5), kw.get("act_lr", 1e-3))


def test_swin_units_are_refused_up_front():
    import lic
    from helpers import AQ, WQ
    from quantization import block_reconstruction
    from quantization.quant_block import QuantRSTB
    from quantization.recon import learn_act_ranges
    unit = QuantRSTB(lic.RSTB(dim=16, input_resolution=(8, 8), depth=2, num_heads=2, window_size=4, mlp_ratio=2.0), WQ, AQ)
    x = torch.zeros(2, 16, 8, 8)
    with pytest.raises(NotImplementedError, match="RSTB"):
        learn_act_ranges(unit, x, x, 5, 1e-3, 2)
    args = types.SimpleNamespace(task_loss=2.0, act_mode="static", act_range="learned")
    with pytest.raises(NotImplementedError, match="RSTB"):                # before the model (None) or a device is looked at
        block_reconstruction(None, unit, "g_a1", torch.zeros(2, 3, 64, 64), batch_size=2, iters=1, act_quant=True, args=args)
    assert not unit.use_act_quant and not unit.use_weight_quant


def test_learn_phase_brackets_leaf_ranges_and_observed_ranges():
    q = _frozen(channels=4, sites=(0, 1))
    before = {k: r.clone() for k, r in q.act_range.items()}
    assert q.act_ste is False and q.act_obs == {}
    q.act_learn()
    assert q.act_phase == "learn" and not q.act_frozen() and sorted(q.act_obs) == [0, 1]
    for k, r in q.act_range.items():
        assert r.is_leaf and r.requires_grad and torch.equal(r.detach(), before[k])
        assert torch.equal(q.act_obs[k], before[k]) and not q.act_obs[k].requires_grad
        assert q.act_obs[k].data_ptr() != r.data_ptr()
    with torch.no_grad():
        q.act_range[1][0] = -0.5
    q2 = pickle.loads(pickle.dumps(q))                                   # (a quantiser caught mid-phase still pickles)
    assert q2.act_phase == "learn" and torch.equal(q2.act_range[1].detach(), q.act_range[1].detach())
    q.act_freeze()
    assert q.act_frozen() and q.act_obs == {} and q.act_err == {}
    assert all(not r.requires_grad for r in q.act_range.values())
    assert torch.equal(q.act_range[0], before[0]) and float(q.act_range[1][0]) == -0.5
    idle = type(q)(act=True, act_mode="static")
    with pytest.raises(RuntimeError, match="not frozen"):
        idle.act_learn()


def test_a_search_keeps_the_observed_ranges_only_when_asked():
    from quantization.quantizer import UniformAffineQuantizer
    for keep in (False, True):
        q = UniformAffineQuantizer(act=True, act_mode="static")
        mx = torch.tensor([-2.0, -1.0, 2.0, 3.0])
        q.act_range = {0: mx.clone()}
        q.act_phase = "observe"
        # (act_search allocates the error sums next to the ranges: on the CPU here)
        q.act_search()
        err = torch.ones(2, 10)
        err[:, 4] = 0.5
        q.act_err = {0: err}
        q.act_freeze(keep_obs=keep)
        assert q.act_frozen() and bool((q.act_range[0][:2] > mx[:2]).all()) and bool((q.act_range[0][2:] < mx[2:]).all())
        assert (sorted(q.act_obs) == [0] and torch.equal(q.act_obs[0], mx)) if keep else q.act_obs == {}
        q.act_learn()
        assert torch.equal(q.act_obs[0], mx if keep else q.act_range[0].detach())
        q.act_freeze()
        assert q.act_obs == {}


def test_only_a_frozen_quantiser_with_act_ste_and_a_tracked_input_goes_on_the_tape(monkeypatch):
    import hipops.autograd as A
    import quantization.quantizer as Q
    calls = []
    monkeypatch.setattr(Q.ops, "actquant_static", lambda xr, rng, out=None, n_bits=8: calls.append(("plain", rng.requires_grad)) or xr)
    monkeypatch.setattr(A.ActQuantStaticFn, "apply", staticmethod(lambda x, rng, bits, cl: calls.append(("tape", bits, cl)) or x))
    q = _frozen(channels=3, bits=10)
    x = torch.zeros(1, 3, 2, 2)
    xt = x.clone().requires_grad_(True)
    q(xt, True)                                                           # act_ste off: detached, as before
    q.act_ste = True
    q(x, True)                                                            # input not tracked
    with torch.no_grad():
        q(xt, True)                                                       # no tape
    assert calls == [("plain", False)] * 3
    q(xt, True)
    assert calls[-1] == ("tape", 10, False)
    q.act_ste = False
    q.act_learn()
    q(x, True)                                                            # learning: the ranges are what is tracked
    assert calls[-1] == ("tape", 10, False)
    with torch.no_grad():
        q(x, True)
    assert calls[-1] == ("plain", False)


def test_quantiser_pickled_before_act_ste_existed_behaves_as_before(monkeypatch):
    import hipops.autograd as A
    import quantization.quantizer as Q
    q = _frozen(channels=3, sites=(0, 1))
    for name in ("act_ste", "act_obs"):
        del q.__dict__[name]
    q = pickle.loads(pickle.dumps(q))
    assert not hasattr(q, "act_ste") and not hasattr(q, "act_obs") and q.act_frozen() and sorted(q.act_range) == [0, 1]
    seen = []
    monkeypatch.setattr(Q.ops, "actquant_static", lambda xr, rng, out=None, n_bits=8: seen.append(n_bits) or xr)

    def never(*a):
        raise AssertionError("an old artefact went on the tape")
    monkeypatch.setattr(A.ActQuantStaticFn, "apply", staticmethod(never))
    xt = torch.zeros(1, 3, 2, 2, requires_grad=True)
    out = q(xt, True, site=1)
    assert seen == [8] and not out.requires_grad                          # the detached static call
    moved = q.to("cpu")                                                   # _apply copes with the missing dictionaries
    assert sorted(moved.act_range) == [0, 1]
    q.act_learn()                                                         # ... and the new phase works on it
    assert sorted(q.act_obs) == [0, 1]
    q.act_freeze()
    assert q.act_frozen() and q.act_obs == {}


def test_range_gradient_reduction_without_a_process_group_is_the_identity():
    from quantization import dp
    g = torch.tensor([1.0, -2.0, 3.0, 4.0])
    assert dp.reduce_act_grads(g) is g and g.tolist() == [1.0, -2.0, 3.0, 4.0]
