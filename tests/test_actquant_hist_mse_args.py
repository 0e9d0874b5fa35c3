"""CPU checks of the histogram-MSE activation ranges' surface: `act_range='hist_mse'` is accepted and every unknown value still refused,
the new entry point is exported, declared and refuses bad arguments before any launch, the op checks its tensors and the grid width on
the host, the histogram phase knows its two rules, and a quantiser pickled before the rule existed freezes as percentile."""
import os
import pickle
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hist_mse_is_an_accepted_act_range():
    from quantization.recon import _act_args
    assert _act_args(types.SimpleNamespace(act_mode="static", act_range="hist_mse")) == ("static", "hist_mse")
    for how in ("kl", "hist", "mse", "l1"):
        with pytest.raises(ValueError, match="act_range.*hist_mse"):
            _act_args(types.SimpleNamespace(act_mode="static", act_range=how))


def test_symbol_is_exported_declared_and_validates_arguments():
    from hipops import _lib as L
    assert "rdo_act_hist_mse_select" in L.EXPORTS
    with open(os.path.join(ROOT, "include", "rdo_ptq_hip.h")) as f:
        assert "int rdo_act_hist_mse_select(const int32_t* hist" in f.read()
    h = L.lib()
    one = torch.zeros(4096, dtype=torch.float32)                          # (host memory: never touched, the arguments are refused first)
    p = one.data_ptr()
    assert h.rdo_act_hist_mse_select(None, 4, None, 8, None, None, None) != 0
    assert h.rdo_act_hist_mse_select(None, 4, p, 8, p, None, None) != 0
    assert h.rdo_act_hist_mse_select(p, 4, None, 8, p, None, None) != 0
    assert h.rdo_act_hist_mse_select(p, 4, p, 8, None, p, None) != 0
    for C in (0, -3):
        assert h.rdo_act_hist_mse_select(p, C, p, 8, p, None, None) != 0
        assert h.rdo_act_hist_mse_select(p, C, p, 8, p, p, None) != 0
    for bits in (1, 17):
        assert h.rdo_act_hist_mse_select(p, 4, p, bits, p, None, None) != 0
        assert h.rdo_act_hist_mse_select(p, 4, p, bits, p, p, None) != 0
    assert b"n_bits" in h.rdo_last_error()


def test_host_side_checks_of_the_op():
    from hipops import ops
    rng = torch.zeros(8)
    with pytest.raises(ValueError, match="act_hist_mse_select"):
        ops.act_hist_mse_select(torch.zeros(4, 1024), rng, 8)                              # a float histogram
    with pytest.raises(ValueError, match="act_hist_mse_select"):
        ops.act_hist_mse_select(torch.zeros(4, 512, dtype=torch.int32), rng, 8)
    with pytest.raises(ValueError, match="act_hist_mse_select"):
        ops.act_hist_mse_select(torch.zeros(4, 1024, dtype=torch.int32), torch.zeros(6), 8)
    with pytest.raises(ValueError, match="act_hist_mse_select"):
        ops.act_hist_mse_select(torch.zeros(8, 1024, dtype=torch.int32)[::2], rng, 8)      # not contiguous
    for bits in (1, 17, 8.0, True):
        with pytest.raises(ValueError, match="n_bits"):
            ops.act_hist_mse_select(torch.zeros(4, 1024, dtype=torch.int32), rng, bits, score=True)


def _observed():
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(n_bits=8, channel_wise=True, scale_method="max", act=True, act_mode="static", dynamic_bits=4)
    q.act_range = {0: torch.tensor([-1.0, -2.0, 3.0, 4.0])}
    return q


def test_histogram_rules():
    from quantization.quantizer import ACT_HIST_RULES, UniformAffineQuantizer
    assert ACT_HIST_RULES == ("percentile", "mse")
    q = UniformAffineQuantizer(act=True, act_mode="static")
    assert q.act_hist_rule == "percentile"
    for rule in ACT_HIST_RULES:                                           # before observing: the existing refusal
        with pytest.raises(RuntimeError, match="act_histogram"):
            q.act_histogram(rule=rule)
    q.act_observe()
    with pytest.raises(RuntimeError, match="act_histogram"):
        q.act_histogram(99.0, rule="mse")
    assert q.act_hist == {} and q.act_phase == "observe"
    q = _observed()
    for rule in ("kl", "", None, "MSE"):
        with pytest.raises(ValueError, match="rule"):
            q.act_histogram(rule=rule)
    assert q.act_hist == {} and q.act_hist_rule == "percentile" and q.act_phase == "idle"
    q.act_histogram()                                                     # the default is today's behaviour
    assert q.act_hist_rule == "percentile" and q.act_phase == "hist" and q.act_tail == pytest.approx(1e-4)
    q.act_histogram(rule="mse")
    assert q.act_hist_rule == "mse" and q.act_phase == "hist" and sorted(q.act_hist) == [0]
    assert q.act_hist[0].dtype == torch.int32 and tuple(q.act_hist[0].shape) == (2, 1024)
    q2 = pickle.loads(pickle.dumps(q))
    assert q2.act_hist_rule == "mse" and torch.equal(q2.act_hist[0], q.act_hist[0])


def test_freeze_calls_the_selection_of_the_rule(monkeypatch):
    """which op `act_freeze` hands the histogram to, and with which grid width (the ops themselves run on the GPU: they are replaced)"""
    from hipops import ops
    calls = []
    monkeypatch.setattr(ops, "act_hist_mse_select", lambda hist, rng, n_bits: (calls.append(("mse", n_bits)), rng * 0.5)[1])
    monkeypatch.setattr(ops, "act_percentile_select", lambda hist, rng, tail: (calls.append(("percentile", tail)), rng * 0.25)[1])
    q = _observed()
    q.act_histogram(rule="mse")
    q.act_freeze()
    assert calls == [("mse", 4)] and q.act_frozen() and q.act_hist == {}
    assert q.act_range[0].tolist() == [-0.5, -1.0, 1.5, 2.0]
    q = _observed()
    q.act_histogram(99.0)
    q.act_freeze()
    assert calls[1][0] == "percentile" and calls[1][1] == pytest.approx(0.01) and len(calls) == 2


def test_quantiser_pickled_before_the_rule_existed_freezes_as_percentile(monkeypatch):
    from hipops import ops
    calls = []
    monkeypatch.setattr(ops, "act_hist_mse_select", lambda hist, rng, n_bits: (calls.append("mse"), rng)[1])
    monkeypatch.setattr(ops, "act_percentile_select", lambda hist, rng, tail: (calls.append(("percentile", tail)), rng)[1])
    q = _observed()
    q.act_histogram(99.0)
    del q.__dict__["act_hist_rule"]
    q = pickle.loads(pickle.dumps(q))
    assert not hasattr(q, "act_hist_rule") and q.act_phase == "hist"
    q.act_freeze()
    assert len(calls) == 1 and calls[0][0] == "percentile" and calls[0][1] == pytest.approx(0.01)
    assert q.act_frozen() and q.act_range[0].tolist() == [-1.0, -2.0, 3.0, 4.0]
