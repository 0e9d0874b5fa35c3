"""CPU checks of the per-unit output error report: `args.unit_report` is validated before any work is done, `ops.pair_moments` refuses
malformed operands with ValueError before any pointer is taken or library call made, the C entry `rdo_pair_moments` returns RDO_EINVAL
with a message for null pointers and non-positive counts without touching a device, and `export.unit_report` derives its columns from
hand-made `unit_stats` as documented."""
import ctypes as C
import math
import types

import pytest
import torch

RDO_EINVAL = -22


# ----------------------------------------------------------------------------- the flag
def test_unit_report_flag_is_a_bool_and_defaults_to_false():
    from quantization.recon import _act_args, _unit_report_args
    assert _unit_report_args(None) is False
    assert _unit_report_args(types.SimpleNamespace()) is False
    assert _unit_report_args(types.SimpleNamespace(unit_report=False)) is False
    assert _unit_report_args(types.SimpleNamespace(unit_report=True)) is True
    for bad in (1, "yes", None, 0, 1.0, [True]):
        with pytest.raises(ValueError, match="unit_report must be True or False"):
            _unit_report_args(types.SimpleNamespace(unit_report=bad))
        with pytest.raises(ValueError, match="unit_report must be True or False"):       # together with the activation arguments
            _act_args(types.SimpleNamespace(unit_report=bad))
    assert _act_args(types.SimpleNamespace(unit_report=True)) == ("dynamic", "max")


def test_reconstruct_refuses_a_bad_flag_before_any_work():
    """`_reconstruct` validates with the other arguments: nothing of the model or the data is touched (both are None here)"""
    from quantization.recon import reconstruct
    cali = torch.zeros(2, 3, 8, 8)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="unit_report must be True or False"):
            reconstruct(None, None, "g_a.0", cali, args=types.SimpleNamespace(unit_report=bad))


# ----------------------------------------------------------------------------- the wrapper
@pytest.fixture()
def no_library(monkeypatch):
    """any library call or pointer conversion after the argument checks fails the test"""
    from hipops import _lib as L
    from hipops import ops

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(ops, "_ptr", boom)
    return ops


def _t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_pair_moments_refuses_malformed_operands(no_library):
    ops = no_library
    a, b = _t(2, 5, 6), _t(2, 5, 6)
    cases = [
        ((a, _t(2, 5, 7)), {}, "shapes differ"),
        ((a, _t(2, 30)), {}, "shapes differ"),
        ((a, _t(60)), {}, "shapes differ"),
        ((a.double(), b.double()), {}, "must be an fp32 tensor"),
        ((a, b.half()), {}, "b must be an fp32 tensor"),
        ((a.to(torch.int32), b), {}, "a must be an fp32 tensor"),
        ((None, b), {}, "a must be an fp32 tensor"),
        ((a, 1.0), {}, "b must be an fp32 tensor"),
        ((_t(0, 6), _t(0, 6)), {}, "empty"),
        ((_t(4, 0), _t(4, 0)), {}, "empty"),
        ((_t(()), _t(())), {}, "empty or scalars"),
        ((_t(6, 5).t(), _t(5, 6)), {}, "contiguous"),
        ((_t(5, 6), _t(5, 12)[:, ::2]), {}, "contiguous"),
        ((a, torch.zeros(2, 5, 6, device="meta")), {}, "a is on cpu, b on meta"),
        ((a, b), {"out": _t(3, 5)}, "out must be a contiguous fp32"),
        ((a, b), {"out": _t(6, 3)}, "out must be a contiguous fp32"),
        ((a, b), {"out": _t(18)}, "out must be a contiguous fp32"),
        ((a, b), {"out": _t(3, 6).double()}, "out must be a contiguous fp32"),
        ((a, b), {"out": _t(3, 12)[:, ::2]}, "out must be a contiguous fp32"),
        ((a, b), {"out": torch.zeros(3, 6, device="meta")}, "out must be a contiguous fp32"),
        ((a, b), {"out": 0.0}, "out must be a contiguous fp32"),
        ((a, b), {}, "no CPU path"),                    # well formed, but on the CPU
        ((a, b), {"out": _t(3, 6)}, "no CPU path"),
    ]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=f"pair_moments: .*{what}"):
            ops.pair_moments(*args, **kw)


# ----------------------------------------------------------------------------- the C entry
def test_c_abi_refuses_null_pointers_and_non_positive_counts():
    """RDO_REQUIRE runs before any launch: the non-null arguments below are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    for args in [(None, p, 8, 2, p, p), (p, None, 8, 2, p, p), (p, p, 8, 2, None, p), (p, p, 8, 2, p, None), (p, p, 0, 2, p, p),
                 (p, p, -8, 2, p, p), (p, p, 8, 0, p, p), (p, p, 8, -1, p, p)]:
        assert h.rdo_pair_moments(*args, None) == RDO_EINVAL, args
        assert b"rdo_pair_moments" in h.rdo_last_error()
    assert h.rdo_pair_moments_workspace(0) == 0 and h.rdo_pair_moments_workspace(-3) == 0
    assert h.rdo_pair_moments_workspace(1) == 3 * 256 and h.rdo_pair_moments_workspace(192) == 3 * 192 * 256
    assert "rdo_pair_moments" in L.EXPORTS and "rdo_pair_moments_workspace" in L.EXPORTS


# ----------------------------------------------------------------------------- the read-out
class _Unit(torch.nn.Module):
    pass


def _stats(name, n, nearest, learned):
    f = lambda rows: {k: torch.tensor(v, dtype=torch.float64) for k, v in zip(("shift", "err", "energy"), rows)}
    return {"name": name, "n": n, "nearest": f(nearest), "learned": f(learned)}


def _model():
    m = torch.nn.Module()
    m.first, m.plain, m.second = _Unit(), _Unit(), _Unit()
    #                      shift              err                 energy
    m.second.unit_stats = _stats("g_a.1", 10, ([2.0, -4.0, 0.0], [4.0, 1.6, 0.0], [400.0, 16.0, 9.0]),
                                 ([0.0, 1.0, 3.0], [1.0, 0.1, 2.0], [400.0, 16.0, 9.0]))
    m.first.unit_stats = _stats("g_a.0", 4, ([0.0], [0.0], [8.0]), ([2.0], [1.0], [8.0]))
    return m


def test_unit_report_of_hand_made_statistics():
    from quantization.export import unit_report
    rep = unit_report(_model())
    assert list(rep) == ["g_a.0", "g_a.1"]                 # module order, under the names the calibration used
    r = rep["g_a.1"]
    assert r["channels"] == 3 and r["n"] == 10
    for f in ("err", "shift", "energy", "sqnr_db", "shift_share"):
        assert sorted(r[f]) == ["learned", "nearest"]
        assert all(v.dtype == torch.float64 and v.shape == (3,) and v.device.type == "cpu" for v in r[f].values())
    assert r["err"]["nearest"].tolist() == [4.0, 1.6, 0.0] and r["shift"]["learned"].tolist() == [0.0, 1.0, 3.0]
    assert r["energy"]["nearest"].tolist() == [400.0, 16.0, 9.0]
    # sqnr: 10 log10(energy / err), inf at err == 0
    assert r["sqnr_db"]["nearest"][0].item() == pytest.approx(20.0, abs=1e-12)
    assert r["sqnr_db"]["nearest"][1].item() == pytest.approx(10.0, abs=1e-12)
    assert r["sqnr_db"]["nearest"][2].item() == math.inf
    assert r["sqnr_db"]["learned"][0].item() == pytest.approx(10 * math.log10(400.0), abs=1e-12)
    assert r["sqnr_db"]["learned"][1].item() == pytest.approx(10 * math.log10(160.0), abs=1e-12)
    # gain: learned - nearest, per channel
    assert torch.equal(r["gain_db"], r["sqnr_db"]["learned"] - r["sqnr_db"]["nearest"])
    assert r["gain_db"][0].item() == pytest.approx(10 * math.log10(4.0), abs=1e-12)
    assert r["gain_db"][1].item() == pytest.approx(10 * math.log10(16.0), abs=1e-12)
    assert r["gain_db"][2].item() == -math.inf             # nearest was exact on that channel, learned is not
    # shift share: shift^2 / (n err) in [0, 1], 0 at err == 0
    assert r["shift_share"]["nearest"].tolist() == pytest.approx([4.0 / 40.0, 16.0 / 16.0, 0.0], abs=1e-15)
    assert r["shift_share"]["learned"].tolist() == pytest.approx([0.0, 1.0 / 1.0, 9.0 / 20.0], abs=1e-15)
    for state in ("nearest", "learned"):
        assert bool(((r["shift_share"][state] >= 0) & (r["shift_share"][state] <= 1)).all())
    # the total row: the same over the summed channels
    t = r["total"]
    assert t["err"] == {"nearest": pytest.approx(5.6), "learned": pytest.approx(3.1)}
    assert t["shift"] == {"nearest": pytest.approx(-2.0), "learned": pytest.approx(4.0)}
    assert t["energy"] == {"nearest": 425.0, "learned": 425.0}
    assert t["sqnr_db"]["nearest"] == pytest.approx(10 * math.log10(425.0 / 5.6), abs=1e-12)
    assert t["sqnr_db"]["learned"] == pytest.approx(10 * math.log10(425.0 / 3.1), abs=1e-12)
    assert t["gain_db"] == pytest.approx(10 * math.log10(5.6 / 3.1), abs=1e-12)
    # a unit whose nearest pass was exact everywhere
    r0 = rep["g_a.0"]
    assert r0["channels"] == 1 and r0["n"] == 4 and r0["sqnr_db"]["nearest"].tolist() == [math.inf]
    assert r0["shift_share"]["nearest"].tolist() == [0.0] and r0["shift_share"]["learned"].tolist() == [1.0]
    assert r0["total"]["sqnr_db"]["nearest"] == math.inf and r0["total"]["gain_db"] == -math.inf
    # the read-out copies: the recorded statistics are not aliased
    r["err"]["nearest"].zero_()
    assert unit_report(_model())["g_a.1"]["err"]["nearest"].tolist() == [4.0, 1.6, 0.0]


def test_a_model_without_statistics_reports_nothing():
    from quantization.export import unit_report
    m = torch.nn.Module()
    m.a, m.b = _Unit(), torch.nn.Linear(2, 2)
    assert unit_report(m) == {} and isinstance(unit_report(m), dict)
    m.a.unit_stats = None                                  # what an older pickle's getattr default gives
    assert unit_report(m) == {}


def test_quant_model_has_the_read_out():
    from quantization import QuantModel
    assert callable(getattr(QuantModel, "unit_report", None))
