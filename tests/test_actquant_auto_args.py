"""CPU checks of the measured range choice's surface: `act_range='auto'` is accepted and every unknown value still refused, `act_report`
must be a bool, the scoring entry point is exported, declared and refuses bad arguments before any launch, the op checks its tensors on
the host, the selection rule breaks ties and skips NaN sums as documented, the 'l2' clipping helper is the arithmetic `act_freeze` had,
a quantiser pickled before the new attributes existed still loads, freezes and reports nothing, and a dynamic model reports nothing."""
import os
import pickle
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_auto_is_an_accepted_act_range():
    from quantization.recon import _act_args
    assert _act_args(types.SimpleNamespace(act_mode="static", act_range="auto")) == ("static", "auto")
    for how in ("kl", "hist", "mse", "best", ""):
        with pytest.raises(ValueError, match="act_range.*'max', 'l2', 'learned', 'percentile', 'hist_mse' or 'auto'"):
            _act_args(types.SimpleNamespace(act_mode="static", act_range=how))


def test_act_report_must_be_a_bool():
    from quantization import block_reconstruction, layer_reconstruction
    from quantization.recon import _act_args
    for ok in (True, False):
        assert _act_args(types.SimpleNamespace(act_mode="static", act_range="max", act_report=ok)) == ("static", "max")
    for bad in (1, 0, "yes", None, 1.0):
        args = types.SimpleNamespace(task_loss=2.0, act_mode="static", act_range="auto", act_report=bad)
        with pytest.raises(ValueError, match="act_report"):
            _act_args(args)
        for recon in (layer_reconstruction, block_reconstruction):        # refused before the model, the unit or a device is looked at
            with pytest.raises(ValueError, match="act_report"):
                recon(None, None, "0", torch.zeros(2, 3, 64, 64), batch_size=2, iters=1, act_quant=True, args=args)


def test_symbol_is_exported_declared_and_validates_arguments():
    from hipops import _lib as L
    from hipops import ops
    assert "rdo_actquant_score" in L.EXPORTS and "rdo_actquant_score_workspace" in L.EXPORTS
    with open(os.path.join(ROOT, "include", "rdo_ptq_hip.h")) as f:
        text = f.read()
    assert "int rdo_actquant_score(const float* x, int64_t npix, int32_t C, int32_t n_bits, const float* cand" in text
    assert "#define RDO_ACT_SCORE_MAX 4" in text and ops.ACT_SCORE_MAX == 4
    h = L.lib()
    assert h.rdo_actquant_score_workspace(5, 4) == 5 * 13 * 256 and h.rdo_actquant_score_workspace(5, 1) == 5 * 4 * 256
    assert h.rdo_actquant_score_workspace(0, 4) == 0 and h.rdo_actquant_score_workspace(5, 5) == 0 and h.rdo_actquant_score_workspace(5, 0) == 0
    one = torch.zeros(4096, dtype=torch.float32)                          # (host memory: never touched, the arguments are refused first)
    p = one.data_ptr()

    def call(x=p, npix=8, C=4, bits=8, cand=p, K=4, err=p, clip=p, energy=p, ws=p):
        return h.rdo_actquant_score(x, npix, C, bits, cand, K, err, clip, energy, ws, None)
    for name in ("x", "cand", "err", "ws"):
        assert call(**{name: None}) != 0, name
        assert b"rdo_actquant_score" in h.rdo_last_error()
    for C in (0, -3):
        assert call(C=C) != 0
    for npix in (0, -1, 2 ** 31):
        assert call(npix=npix) != 0
    for K in (0, -1, 5):
        assert call(K=K) != 0
        assert b"K" in h.rdo_last_error()
    for bits in (1, 17):
        assert call(bits=bits) != 0
        assert call(bits=bits, clip=None, energy=None) != 0
        assert b"n_bits" in h.rdo_last_error()


def test_host_side_checks_of_the_op():
    from hipops import ops
    C = 6
    x, cand, err = torch.zeros(6, C), torch.zeros(4, 2 * C), torch.zeros(C, 4)
    clip, energy = torch.zeros(C, 4, 2, dtype=torch.int32), torch.zeros(C)
    bad = [
        dict(x=torch.zeros(6, C, dtype=torch.float64)), dict(x=torch.zeros(6, 2 * C)[:, ::2]), dict(x=torch.zeros(0, C)),
        dict(cand=torch.zeros(5, 2 * C)), dict(cand=torch.zeros(0, 2 * C)), dict(cand=torch.zeros(2 * C)), dict(cand=torch.zeros(4, C)),
        dict(cand=torch.zeros(4, 2 * C, dtype=torch.float64)), dict(cand=torch.zeros(8, 2 * C)[::2]),
        dict(err=torch.zeros(C, 3)), dict(err=torch.zeros(4, C)), dict(err=torch.zeros(C, 4, dtype=torch.float64)), dict(err=torch.zeros(C, 8)[:, ::2]),
        dict(clip=torch.zeros(C, 4, 2)), dict(clip=torch.zeros(C, 4, dtype=torch.int32)), dict(clip=torch.zeros(C, 4, 4, dtype=torch.int32)[:, :, ::2]),
        dict(energy=torch.zeros(C + 1)), dict(energy=torch.zeros(C, dtype=torch.int32)), dict(energy=torch.zeros(2 * C)[::2]),
        dict(n_bits=1), dict(n_bits=17), dict(n_bits=8.0), dict(n_bits=True),
    ]
    for kw in bad:
        a = dict(x=x, cand=cand, err=err, clip=clip, energy=energy, n_bits=8)
        a.update(kw)
        with pytest.raises(ValueError, match="actquant_score"):
            ops.actquant_score(a.pop("x"), a.pop("cand"), a.pop("err"), **a)
    with pytest.raises(ValueError, match="actquant_score"):                # K = 1 candidates against a K = 4 table
        ops.actquant_score(x, torch.zeros(1, 2 * C), err)


def test_selection_rule_on_hand_made_tables():
    from quantization.quantizer import ACT_AUTO_CANDIDATES, act_score_winner
    assert ACT_AUTO_CANDIDATES == ("max", "l2", "percentile", "hist_mse")
    err = torch.tensor([
        [4.0, 3.0, 2.0, 1.0],          # the smallest
        [1.0, 1.0, 1.0, 1.0],          # all equal: the earliest
        [2.0, 1.0, 1.0, 3.0],          # a tie of the middle two: the earlier
        [3.0, 2.0, 2.5, 2.0],          # a tie of l2 and hist_mse
        [NAN, 5.0, 4.0, 4.0],          # NaN never wins, ties behind it as usual
        [NAN, NAN, NAN, 7.0],
        [NAN, NAN, NAN, NAN],          # all NaN: the max range
        [INF, NAN, INF, NAN],          # inf is a sum like any other
        [NAN, INF, 1.0, 1.0],
        [0.0, 0.0, NAN, 0.0],
        [1.0, 0.0, -0.0, 0.0],         # -0 == 0: a tie
    ])
    assert act_score_winner(err).tolist() == [3, 0, 1, 1, 2, 3, 0, 0, 2, 0, 1]
    assert act_score_winner(torch.tensor([[NAN], [1.0]])).tolist() == [0, 0]              # K = 1


def _observed(bits=4):
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(n_bits=8, channel_wise=True, scale_method="max", act=True, act_mode="static", dynamic_bits=bits)
    q.act_range = {0: torch.tensor([-1.0, -2.0, 3.0, 4.0])}
    return q


def test_auto_freeze_assembles_each_channel_from_its_winner():
    from quantization.quantizer import UniformAffineQuantizer
    q = _observed()
    with pytest.raises(RuntimeError, match="act_candidates"):
        q.act_candidates()
    cands = {0: torch.tensor([[-1.0, -2.0, 3.0, 4.0], [-0.9, -1.9, 2.9, 3.9], [-0.8, -1.8, 2.8, 3.8], [-0.7, -1.7, 2.7, 3.7]])}
    with pytest.raises(RuntimeError, match="candidates"):
        q.act_score()                                                     # not frozen: there is nothing to score without candidates
    with pytest.raises(ValueError, match="act_score"):
        q.act_score({1: cands[0]})
    with pytest.raises(ValueError, match="act_score"):
        q.act_score({0: torch.zeros(5, 4)})
    with pytest.raises(ValueError, match="act_score"):
        q.act_score({0: torch.zeros(4, 6)})
    assert q.act_phase == "idle"
    q.act_score(cands)
    assert q.act_phase == "score" and q.act_score_kind == "auto" and not q.act_frozen()
    assert tuple(q.act_err[0].shape) == (2, 4) and tuple(q.act_clip[0].shape) == (2, 4, 2) and q.act_clip[0].dtype == torch.int32
    assert tuple(q.act_energy[0].shape) == (2,) and q.act_score_n == {0: 0}
    assert torch.equal(q.act_range[0], cands[0][0])                       # the max range goes downstream until the winner is frozen
    q2 = pickle.loads(pickle.dumps(q)).to("cpu")
    assert q2.act_phase == "score" and torch.equal(q2.act_cand[0], cands[0])
    q.act_err[0] = torch.tensor([[2.0, 1.0, 1.0, 3.0], [NAN, NAN, NAN, NAN]])
    q.act_freeze()
    assert q.act_frozen() and q.act_err == {} and q.act_cand == {} and q.act_clip == {} and q.act_energy == {} and q.act_obs == {}
    assert q.act_range[0].tolist() == pytest.approx([-0.9, -2.0, 2.9, 4.0]) and q.act_stats == {}
    with pytest.raises(RuntimeError, match="act_score"):
        UniformAffineQuantizer(act=True, act_mode="static").act_score({})


def test_report_pass_keeps_the_ranges_and_records_the_statistics():
    q = _observed()
    q.act_phase = "frozen"
    rng = q.act_range[0].clone()
    q.act_score()
    assert q.act_phase == "score" and q.act_score_kind == "report" and tuple(q.act_cand[0].shape) == (1, 4)
    assert torch.equal(q.act_cand[0][0], rng) and torch.equal(q.act_range[0], rng)
    q.act_err[0] = torch.tensor([[0.5], [0.0]])
    q.act_energy[0] = torch.tensor([8.0, 2.0])
    q.act_clip[0] = torch.tensor([[[1, 2]], [[0, 0]]], dtype=torch.int32)
    q.act_score_n[0] = 40
    q.act_freeze()
    assert q.act_frozen() and torch.equal(q.act_range[0], rng) and q.act_err == {} and q.act_cand == {}
    st = q.act_stats[0]
    assert st["err"].tolist() == [0.5, 0.0] and st["energy"].tolist() == [8.0, 2.0] and st["n"] == 40
    assert st["clip_lo"].tolist() == [1, 0] and st["clip_hi"].tolist() == [2, 0] and st["clip_lo"].dtype == torch.int32
    q = pickle.loads(pickle.dumps(q)).to("cpu")
    assert q.act_stats[0]["clip_hi"].tolist() == [2, 0] and q.act_stats[0]["n"] == 40
    model = types.SimpleNamespace(act_quantizers=lambda: [("m.act_quantizer", q)])
    from quantization.export import activation_report
    rep = activation_report(model)
    assert list(rep) == ["m.act_quantizer"]
    r = rep["m.act_quantizer"]
    assert r["n"] == 40 and r["n_bits"] == 4 and r["channels"] == 2 and r["sqnr_db"].dtype == torch.float64
    assert r["sqnr_db"][0].item() == pytest.approx(10.0 * 1.2041199826559248) and r["sqnr_db"][1].item() == INF
    assert r["clipped_share"].tolist() == pytest.approx([3 / 40, 0.0])
    q.act_observe()                                                       # a new calibration: the old measurement is gone
    assert q.act_stats == {} and activation_report(model) == {}


def test_l2_clipping_helper_is_the_arithmetic_of_act_freeze():
    """`act_l2_range` against the expressions `act_freeze` held before the helper existed, restated here, and through `act_freeze`"""
    from quantization.quantizer import UniformAffineQuantizer, act_l2_range
    g = torch.Generator().manual_seed(5)
    C = 64
    lo = torch.randn(C, generator=g) - 0.3
    hi = lo + torch.rand(C, generator=g) * 3
    rng = torch.cat([lo, hi])
    err = torch.rand(C, 10, generator=g)
    table = torch.tensor([1.0 - 0.05 * i for i in range(10)], dtype=torch.float32)
    s = table[err.argmin(dim=1)]
    l2, h2 = torch.maximum(lo * s, lo), torch.minimum(hi * s, hi)
    keep = l2 > h2
    want = torch.cat([torch.where(keep, lo, l2), torch.where(keep, hi, h2)])
    assert int(keep.sum()) > 0 and int((want != rng).sum()) > C // 2
    assert torch.equal(act_l2_range(rng, err), want)
    q = UniformAffineQuantizer(act=True, act_mode="static")
    q.act_range = {0: rng.clone()}
    q.act_search()
    q.act_err[0] = err.clone()
    q.act_freeze()
    assert q.act_frozen() and torch.equal(q.act_range[0], want)


def test_search_and_histogram_share_a_phase():
    q = _observed()
    q.act_histogram(99.0, rule="mse", search=True)
    assert q.act_phase == "search+hist" and tuple(q.act_err[0].shape) == (2, 10) and tuple(q.act_hist[0].shape) == (2, 1024)
    assert q.act_tail == pytest.approx(0.01) and torch.equal(q.act_obs[0], q.act_range[0])
    with pytest.raises(RuntimeError, match="act_score"):                  # the pass selects nothing by itself
        q.act_freeze()
    assert q.act_phase == "search+hist"
    q = _observed()
    q.act_histogram()
    assert q.act_phase == "hist" and q.act_err == {}


def test_quantiser_pickled_before_the_attributes_existed():
    from quantization.export import activation_report
    q = _observed()
    for name in ("act_cand", "act_clip", "act_energy", "act_score_n", "act_score_kind", "act_stats"):
        del q.__dict__[name]
    q = pickle.loads(pickle.dumps(q))
    assert not hasattr(q, "act_stats") and not hasattr(q, "act_cand")
    q = q.to("cpu")
    q.act_freeze()
    assert q.act_frozen() and q.act_range[0].tolist() == [-1.0, -2.0, 3.0, 4.0]
    model = types.SimpleNamespace(act_quantizers=lambda: [("m.act_quantizer", q)])
    assert activation_report(model) == {}
    q.act_score()                                                         # and it takes the report pass like a new one
    assert q.act_phase == "score" and q.act_score_kind == "report"
    q.act_freeze()
    assert q.act_frozen() and sorted(q.act_stats) == [0]


def test_activation_report_of_a_dynamic_model_is_empty():
    import lic
    from quantization import QuantModel
    from quantization.export import activation_report
    torch.manual_seed(0)
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=lic.Cheng2020Anchor(N=8).eval(), weight_quant_params=wq, act_quant_params=aq, is_cheng=True)
    assert activation_report(qnn) == {} and qnn.act_report() == {}
    qnn.set_act_mode("static")                                            # static but never calibrated: still nothing to report
    assert qnn.act_report() == {} and len(qnn.act_quantizers()) > 0
