"""CPU checks of the percentile activation ranges' surface: `act_range='percentile'` and `act_percentile` are validated before any work
is done, the new entry points are exported and refuse bad arguments, the histogram phase needs observed ranges, and a quantiser pickled
before `act_hist` existed still loads, reports and moves."""
import io
import pickle
import types

import pytest
import torch

BAD = [50, 0, 100.1, float("nan"), float("inf"), True, "99"]


def test_percentile_is_an_accepted_act_range():
    from quantization.recon import _act_args
    assert _act_args(types.SimpleNamespace(act_mode="static", act_range="percentile")) == ("static", "percentile")
    with pytest.raises(ValueError, match="act_range.*percentile"):
        _act_args(types.SimpleNamespace(act_mode="static", act_range="kl"))


def test_act_percentile_defaults_and_accepted_values():
    from quantization.recon import _act_percentile_args
    assert _act_percentile_args(None) == 99.99
    assert _act_percentile_args(types.SimpleNamespace()) == 99.99
    assert _act_percentile_args(types.SimpleNamespace(act_percentile=50.5)) == 50.5
    assert _act_percentile_args(types.SimpleNamespace(act_percentile=100)) == 100.0


@pytest.mark.parametrize("p", BAD, ids=[repr(p) for p in BAD])
def test_bad_act_percentile_is_refused_before_any_work(p):
    from quantization import block_reconstruction, layer_reconstruction
    from quantization.recon import _act_args, _act_percentile_args, calibrate_act_ranges
    args = types.SimpleNamespace(task_loss=2.0, act_mode="static", act_range="percentile", act_percentile=p)
    with pytest.raises(ValueError, match="act_percentile"):
        _act_percentile_args(args)
    with pytest.raises(ValueError, match="act_percentile"):
        _act_args(args)
    for recon in (layer_reconstruction, block_reconstruction):            # refused before the model, the unit or a device is looked at
        with pytest.raises(ValueError, match="act_percentile"):
            recon(None, None, "0", torch.zeros(2, 3, 64, 64), batch_size=2, iters=1, act_quant=True, args=args)
    with pytest.raises(ValueError, match="act_percentile"):
        calibrate_act_ranges(None, None, "percentile", percentile=p)


def test_symbols_are_exported_and_validate_arguments():
    from hipops import _lib as L
    from hipops import ops
    h = L.lib()
    for name in ("rdo_actquant_hist_bins", "rdo_actquant_hist", "rdo_act_percentile_select"):
        assert name in L.EXPORTS
    assert h.rdo_actquant_hist_bins() == 1024 == ops.ACT_HIST_BINS
    assert h.rdo_actquant_hist(None, 4, 4, None, None, None) != 0
    assert h.rdo_act_percentile_select(None, 4, None, 0.01, None, None) != 0
    one = torch.zeros(4096, dtype=torch.float32)                          # (host memory: never touched, the arguments are refused first)
    p = one.data_ptr()
    for C in (0, -3):
        assert h.rdo_actquant_hist(p, 4, C, p, p, None) != 0
        assert h.rdo_act_percentile_select(p, C, p, 0.01, p, None) != 0
    assert h.rdo_actquant_hist(p, 0, 4, p, p, None) != 0
    for tail in (0.5, -0.1, float("nan")):
        assert h.rdo_act_percentile_select(p, 4, p, tail, p, None) != 0


def test_histogram_needs_observed_ranges():
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(act=True, act_mode="static")
    with pytest.raises(RuntimeError, match="act_histogram"):
        q.act_histogram(99.0)
    q.act_observe()
    with pytest.raises(RuntimeError, match="act_histogram"):
        q.act_histogram(99.0)
    assert q.act_hist == {}


def test_host_side_shape_checks():
    from hipops import ops
    x, rng = torch.zeros(5, 4), torch.zeros(8)
    with pytest.raises(ValueError):
        ops.actquant_hist(x, torch.zeros(6), torch.zeros(4, 1024, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.actquant_hist(x, rng, torch.zeros(3, 1024, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.actquant_hist(x, rng, torch.zeros(4, 1024))
    with pytest.raises(ValueError):
        ops.act_percentile_select(torch.zeros(4, 1024, dtype=torch.int32), torch.zeros(6), 0.01)


def test_counter_overflow_is_refused_before_the_launch():
    """the running pixel count is kept on the host: the refusal comes before any tensor is handed to the library"""
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(act=True, act_mode="static")
    q.act_range = {0: torch.tensor([0.0, 0.0, 1.0, 1.0])}
    q.act_phase = "hist"
    q.act_hist = {0: torch.zeros(2, 1024, dtype=torch.int32)}
    q.act_hist_n = {0: 2 ** 31 - 4}
    with pytest.raises(OverflowError, match="32-bit"):
        q(torch.zeros(1, 2, 2, 2), True)                        # 4 more pixels: 2^31 in all
    assert q.act_hist_n[0] == 2 ** 31 - 4


def _frozen():
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(n_bits=8, channel_wise=True, scale_method="max", act=True, act_mode="static")
    q.act_range[0] = torch.tensor([-1.0, -2.0, 3.0, 4.0])
    q.act_phase = "frozen"
    return q


def test_quantiser_pickled_before_act_hist_existed():
    q = _frozen()
    for name in ("act_hist", "act_tail", "act_hist_n"):
        del q.__dict__[name]
    q = pickle.loads(pickle.dumps(q))
    assert not hasattr(q, "act_hist") and q.act_frozen()
    moved = q.to("cpu")
    assert moved.act_frozen() and torch.equal(moved.act_range[0], torch.tensor([-1.0, -2.0, 3.0, 4.0]))
    q.act_freeze()                                              # freezing again finds no histogram and keeps the range
    assert q.act_frozen() and q.act_range[0].tolist() == [-1.0, -2.0, 3.0, 4.0]
    q.set_act_mode("static")
    assert q.act_hist == {}


def test_frozen_quantiser_pickles_with_an_empty_act_hist():
    q = _frozen()
    buf = io.BytesIO()
    torch.save(q, buf)
    buf.seek(0)
    for r in (pickle.loads(pickle.dumps(q)), torch.load(buf, weights_only=False)):
        assert r.act_frozen() and r.act_hist == {} and torch.equal(r.act_range[0], q.act_range[0])
