"""CPU checks of the bias correction after calibration: `args.bias_correct` is validated before any work is done, `ops.tap_sums` and
`ops.bias_shift` refuse malformed operands with ValueError before any pointer is taken or library call made, the C entries
`rdo_tap_sums` and `rdo_bias_shift` return RDO_EINVAL with a message that names them for null pointers and every bad geometry without
touching a device, include/rdo_ptq_bias.h declares exactly the entries of `EXPORTS_BIAS`, and `export.bias_report` derives its columns
from hand-made `bias_stats` as documented."""
import ctypes as C
import os
import re
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the flag
def test_bias_correct_flag_names_a_mode_and_defaults_to_off():
    from quantization.recon import _act_args, _bias_correct_args
    assert _bias_correct_args(None) is None
    assert _bias_correct_args(types.SimpleNamespace()) is None
    assert _bias_correct_args(types.SimpleNamespace(bias_correct=None)) is None
    assert _bias_correct_args(types.SimpleNamespace(bias_correct=False)) is None
    assert _bias_correct_args(types.SimpleNamespace(bias_correct="weight")) == "weight"
    assert _bias_correct_args(types.SimpleNamespace(bias_correct="output")) == "output"
    for bad in (True, 1, 0, "yes", "Output", "", ["output"], 1.0):
        with pytest.raises(ValueError, match="bias_correct must be 'weight', 'output' or off"):
            _bias_correct_args(types.SimpleNamespace(bias_correct=bad))
        with pytest.raises(ValueError, match="bias_correct must be 'weight', 'output' or off"):    # together with the activation arguments
            _act_args(types.SimpleNamespace(bias_correct=bad))
    assert _act_args(types.SimpleNamespace(bias_correct="output")) == ("dynamic", "max")


def test_reconstruct_refuses_a_bad_flag_before_any_work():
    """`_reconstruct` validates with the other arguments: nothing of the model or the data is touched (both are None here)"""
    from quantization.recon import reconstruct
    cali = torch.zeros(2, 3, 8, 8)
    for bad in (True, 1, "yes", "Output", ["weight"]):
        with pytest.raises(ValueError, match="bias_correct must be"):
            reconstruct(None, None, "g_a.0", cali, args=types.SimpleNamespace(bias_correct=bad))


def test_correct_unit_bias_refuses_an_unnamed_mode():
    from quantization.recon import correct_unit_bias
    for bad in (True, None, "Weight"):
        with pytest.raises(ValueError, match="bias_correct must be 'weight' or 'output'"):
            correct_unit_bias(None, "u", None, None, None, mode=bad)


# ----------------------------------------------------------------------------- the wrappers
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


def test_tap_sums_refuses_malformed_operands(no_library):
    ops = no_library
    x = _t(2, 5, 7, 4)
    ok = dict(k=3, stride=1, pad=1, out_hw=(5, 7))
    cases = [
        ((x.double(),), ok, "x must be an fp32 tensor"),
        ((None,), ok, "x must be an fp32 tensor"),
        ((x.to(torch.int32),), ok, "x must be an fp32 tensor"),
        ((_t(2, 5, 28),), ok, "rank 4"),
        ((_t(70, 4),), ok, "rank 4"),
        ((_t(4),), dict(k=1, stride=1, pad=0, out_hw=None), "rank"),
        ((_t(0, 5, 7, 4),), ok, "empty"),
        ((_t(2, 5, 7, 0),), ok, "empty"),
        ((_t(2, 5, 4, 7).transpose(2, 3),), ok, "contiguous"),
        ((_t(2, 5, 7, 8)[..., ::2],), ok, "contiguous"),
        ((x,), dict(ok, k=0), "k must be a whole number >= 1"),
        ((x,), dict(ok, k=True), "k must be a whole number"),
        ((x,), dict(ok, k=3.0), "k must be a whole number"),
        ((x,), dict(k=8, stride=1, pad=4, out_hw=(6, 8)), "at most 7"),
        ((x,), dict(ok, stride=0), "stride must be a whole number >= 1"),
        ((x,), dict(ok, pad=-1), "pad must be a whole number >= 0"),
        ((x,), dict(ok, transposed=1), "transposed must be True or False"),
        ((x,), dict(ok, out_hw=(5,)), "out_hw must be a pair"),
        ((x,), dict(ok, out_hw=None), "out_hw must be a pair"),
        ((x,), dict(ok, out_hw=(5.0, 7)), "out_hw must be a pair"),
        ((x,), dict(ok, out_hw=(0, 7)), "out_hw must be a pair"),
        ((x,), dict(ok, out_hw=(4, 7)), "geometry: a conv of 5 inputs .* Ho = 4"),
        ((x,), dict(ok, out_hw=(5, 8)), "geometry: a conv of 7 inputs .* Wo = 8"),
        ((x,), dict(k=7, stride=1, pad=0, out_hw=(1, 1)), "geometry: a conv of 5 inputs"),          # map smaller than the kernel, no padding
        ((x,), dict(k=3, stride=2, pad=1, out_hw=(3, 5)), "geometry: a conv of 7 inputs .* Wo = 5"),
        ((x,), dict(k=3, stride=2, pad=1, out_hw=(8, 13), transposed=True), "geometry: a transposed conv of 5 inputs .* 9 .. 10 outputs, Ho = 8"),
        ((x,), dict(k=3, stride=2, pad=1, out_hw=(9, 15), transposed=True), "geometry: a transposed conv of 7 inputs .* 13 .. 14 outputs, Wo = 15"),
        ((_t(6, 4),), dict(k=1, stride=2, pad=0, out_hw=None), "token tensor takes k = 1, stride 1, pad 0"),
        ((_t(6, 4),), dict(k=1, stride=1, pad=0, out_hw=(1, 6)), "out_hw must be None for a token tensor"),
        ((x,), dict(ok, out=_t(9, 5)), "out must be a contiguous fp32 \\[9, 4\\]"),
        ((x,), dict(ok, out=_t(4, 9)), "out must be a contiguous fp32"),
        ((x,), dict(ok, out=_t(36)), "out must be a contiguous fp32"),
        ((x,), dict(ok, out=_t(9, 4).double()), "out must be a contiguous fp32"),
        ((x,), dict(ok, out=_t(9, 8)[:, ::2]), "out must be a contiguous fp32"),
        ((x,), dict(ok, out=torch.zeros(9, 4, device="meta")), "out must be a contiguous fp32"),
        ((x,), dict(ok, out=0.0), "out must be a contiguous fp32"),
        ((torch.zeros(1, 1, 1, 44_000_000, device="meta"),), dict(k=7, stride=1, pad=3, out_hw=(1, 1)), "too many for 32-bit entry indices"),
        ((_t(1, 60, 60, 4),), dict(k=3, stride=1, pad=25, out_hw=(12, 12), transposed=True), "more than 48 border indices"),
        ((x,), ok, "no CPU path"),                      # well formed, but on the CPU
        ((x,), dict(k=np.int64(3), stride=np.int32(1), pad=np.int64(1), out_hw=(np.int64(5), 7)), "no CPU path"),      # numpy integers count
        ((x,), dict(ok, out=_t(9, 4)), "no CPU path"),
        ((x,), dict(k=3, stride=2, pad=1, out_hw=(9, 14), transposed=True), "no CPU path"),
        ((_t(3, 6, 4),), dict(k=1, stride=1, pad=0, out_hw=None), "no CPU path"),
        ((x,), dict(k=1, stride=1, pad=0, out_hw=None), "no CPU path"),
    ]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=f"tap_sums: .*{what}"):
            ops.tap_sums(*args, **kw)


def test_bias_shift_refuses_malformed_operands(no_library):
    ops = no_library
    w, s, b = _t(3, 2, 2, 4), _t(16, dtype=torch.float64), _t(3)
    cases = [
        ((w.double(), w, s, s, 10, b), {}, "w_ref must be a float32 tensor"),
        ((w, None, s, s, 10, b), {}, "w_q must be a float32 tensor"),
        ((w, w, s.float(), s, 10, b), {}, "s_ref must be a float64 tensor"),
        ((w, w, s, s.float(), 10, b), {}, "s_q must be a float64 tensor"),
        ((w, w, s, s, 10, b.double()), {}, "org_bias must be a float32 tensor"),
        ((_t(0, 4), _t(0, 4), s, s, 10, b), {}, "w_ref is empty"),
        ((w, w, _t(0, dtype=torch.float64), s, 10, b), {}, "s_ref is empty"),
        ((_t(3, 32)[:, ::2], _t(3, 16), s, s, 10, b), {}, "w_ref must be contiguous"),
        ((w, w, _t(32, dtype=torch.float64)[::2], s, 10, b), {}, "s_ref must be contiguous"),
        ((w, torch.zeros(3, 2, 2, 4, device="meta"), s, s, 10, b), {}, "w_q is on meta, w_ref on cpu"),
        ((w, _t(3, 16), s, s, 10, b), {}, "must be the same rows"),
        ((_t(48), _t(48), s, s, 10, b), {}, "must be the same rows"),
        ((w, w, _t(15, dtype=torch.float64), s, 10, b), {}, "s_ref holds 15 elements, the weight rows 16"),
        ((w, w, s, _t(17, dtype=torch.float64), 10, b), {}, "s_q holds 17 elements"),
        ((w, w, s, s, 10, _t(4)), {}, "org_bias has shape"),
        ((w, w, s, s, 10, _t(3, 1)), {}, "org_bias has shape"),
        ((w, w, s, s, 0, b), {}, "n must be a positive whole number"),
        ((w, w, s, s, 2.5, b), {}, "n must be a positive whole number"),
        ((w, w, s, s, True, b), {}, "n must be a positive whole number"),
        ((w, w, s, s, 10, b), {"shift": _t(3)}, "shift must be a contiguous float64 \\[3\\]"),
        ((w, w, s, s, 10, b), {"shift": _t(4, dtype=torch.float64)}, "shift must be a contiguous float64"),
        ((w, w, s, s, 10, b), {"bias_out": _t(3, dtype=torch.float64)}, "bias_out must be a contiguous float32"),
        ((w, w, s, s, 10, b), {"bias_out": _t(6)[::2]}, "bias_out must be a contiguous float32"),
        ((w, w, s, s, 10, b), {}, "no CPU path"),
        ((w, w, s, s, 10, b), {"shift": _t(3, dtype=torch.float64), "bias_out": _t(3)}, "no CPU path"),
    ]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=f"bias_shift: .*{what}"):
            ops.bias_shift(*args, **kw)


def test_tap_out_size():
    from hipops import ops
    assert ops.tap_out_size(5, 3, 1, 1) == 5 and ops.tap_out_size(6, 3, 2, 0) == 2 and ops.tap_out_size(1, 3, 1, 1) == 1
    assert ops.tap_out_size(4, 3, 2, 1, True, 1) == 8 and ops.tap_out_size(2, 4, 2, 1, True) == 4


# ----------------------------------------------------------------------------- the C entries
def test_header_declares_and_library_exports_the_entries():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_bias.h")).read()
    declared = set(re.findall(r"^int(?:64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == {"rdo_tap_sums", "rdo_tap_sums_workspace", "rdo_tap_sums_lane_pixels", "rdo_bias_shift"} == set(L.EXPORTS_BIAS)
    assert '#include "rdo_ptq_hip.h"' in hdr
    assert int(re.search(r"^#define RDO_TAP_MAX_K (\d+)", hdr, re.M).group(1)) == L.TAP_MAX_K == 7
    h = L.lib()
    for name in declared:
        assert hasattr(h, name) and name not in L.EXPORTS and name not in L.EXPORTS_GDN


def test_tap_sums_c_entry_refuses_nulls_and_bad_geometry():
    """RDO_REQUIRE runs before any launch: the non-null arguments below are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    #         x  N  H  W  C  k  s  pad Ho Wo tr out ws
    good = [p, 2, 5, 7, 4, 3, 1, 1, 5, 7, 0, p, p]

    def call(**kw):
        names = ["x", "N", "H", "W", "C", "k", "stride", "pad", "Ho", "Wo", "transposed", "out", "ws"]
        a = list(good)
        for k_, v in kw.items():
            a[names.index(k_)] = v
        return h.rdo_tap_sums(*a, None)

    bad = [dict(x=None), dict(out=None), dict(ws=None), dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(W=-7), dict(C=0), dict(C=-4),
           dict(k=0), dict(k=-3), dict(k=8, pad=4, Ho=8, Wo=10), dict(stride=0), dict(stride=-1), dict(pad=-1), dict(transposed=2),
           dict(Ho=0), dict(Wo=-1),
           dict(Ho=4), dict(Ho=6), dict(Wo=8), dict(Wo=6),                            # not what the conv gives
           dict(k=7, pad=0, Ho=1, Wo=1),                                             # map smaller than the kernel, no padding
           dict(stride=2, Ho=3, Wo=5), dict(stride=2, Ho=2, Wo=4),
           dict(transposed=1, stride=2, Ho=8, Wo=13), dict(transposed=1, stride=2, Ho=11, Wo=13), dict(transposed=1, stride=2, Ho=9, Wo=12),
           dict(transposed=1, stride=2, Ho=9, Wo=15), dict(transposed=1, Ho=5, Wo=8),
           dict(N=1 << 20, H=1 << 6, W=1 << 6, Ho=1 << 6, Wo=1 << 6),                  # 2^32 pixels
           dict(N=1, H=1, W=1, k=1, pad=0, Ho=1, Wo=1, C=0x7fffffff)]                # entry indices beyond 32 bits
    for kw in bad:
        assert call(**kw) == RDO_EINVAL, kw
        assert b"rdo_tap_sums" in h.rdo_last_error(), kw
    # the lane count of the chain-closure tests: the same refusals, and a count for what is accepted
    assert h.rdo_tap_sums_lane_pixels(2, 5, 7, 4, 3, 1, 1, 5, 8, 0, 1) == -1 and b"rdo_tap_sums" in h.rdo_last_error()
    assert h.rdo_tap_sums_lane_pixels(2, 5, 7, 4, 8, 1, 4, 5, 7, 0, 1) == -1
    assert h.rdo_tap_sums_lane_pixels(1, 1, 1, 4, 1, 1, 0, 1, 1, 0, 1) == 1
    assert h.rdo_tap_sums_lane_pixels(1, 1, 65536, 192, 1, 1, 0, 1, 65536, 0, 1) >= 65536 // (560 * 5)
    assert h.rdo_tap_sums_lane_pixels(1, 1, 1 << 30, 2, 1, 1, 0, 1, 1 << 30, 0, 0) > 1024          # (an axis of 2^30 indices: the plan is O(k))
    assert h.rdo_tap_sums_workspace(0, 3) == 0 and h.rdo_tap_sums_workspace(-3, 3) == 0
    assert h.rdo_tap_sums_workspace(4, 0) == 0 and h.rdo_tap_sums_workspace(4, 8) == 0
    assert h.rdo_tap_sums_workspace(1, 1) > 0
    assert h.rdo_tap_sums_workspace(192, 3) == 192 * h.rdo_tap_sums_workspace(1, 3)
    assert h.rdo_tap_sums_workspace(1, 7) > h.rdo_tap_sums_workspace(1, 3) > h.rdo_tap_sums_workspace(1, 1)


def test_bias_shift_c_entry_refuses_nulls_and_bad_sizes():
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    #       w_ref w_q s_ref s_q inv_n org O  K  shift bias
    good = [p, p, p, p, 0.25, p, 3, 16, p, p]
    for i in (0, 1, 2, 3, 5, 8, 9):
        a = list(good)
        a[i] = None
        assert h.rdo_bias_shift(*a, None) == RDO_EINVAL, i
        assert b"rdo_bias_shift" in h.rdo_last_error()
    for i, v in ((6, 0), (6, -3), (7, 0), (7, -1), (4, 0.0), (4, -0.5), (4, 2.0), (4, float("nan")), (4, float("inf"))):
        a = list(good)
        a[i] = v
        assert h.rdo_bias_shift(*a, None) == RDO_EINVAL, (i, v)
        assert b"rdo_bias_shift" in h.rdo_last_error()


# ----------------------------------------------------------------------------- the read-out
class _Unit(torch.nn.Module):
    pass


def _f64(v):
    return torch.tensor(v, dtype=torch.float64)


def _stats(name, mode, n, before, after, layers, skipped):
    f = lambda rows: {k: _f64(v) for k, v in zip(("shift", "err", "energy"), rows)}
    return {"name": name, "mode": mode, "n": n, "before": f(before), "after": f(after),
            "layers": OrderedDict((k, {"shift": _f64(v), "n": nn_, "kind": kind}) for k, (v, nn_, kind) in layers.items()),
            "skipped": OrderedDict(skipped)}


def _model():
    m = torch.nn.Module()
    m.first, m.plain, m.second = _Unit(), _Unit(), _Unit()
    #                                       shift              err                 energy
    m.second.bias_stats = _stats("g_a.1", "output", 10, ([2.0, -4.0, 0.0], [4.0, 1.6, 0.0], [400.0, 16.0, 9.0]),
                                 ([0.0, 1.0, 0.0], [3.6, 0.1, 0.0], [400.0, 16.0, 9.0]),
                                 {"conv2": ([0.5, -0.25], 40, "conv"), "conv1": ([0.0, 0.0, -3.0], 10, "tconv")},
                                 [("gdn", "gdn: why"), ("skip", "no bias")])
    m.first.bias_stats = _stats("g_a.0", "weight", 4, ([2.0], [1.0], [8.0]), ([0.0], [0.0], [8.0]), {"layer": ([0.125], 4, "linear")}, [])
    return m


def test_bias_report_of_hand_made_statistics():
    from quantization.export import bias_report
    rep = bias_report(_model())
    assert list(rep) == ["g_a.0", "g_a.1"]                 # module order, under the names the calibration used
    r = rep["g_a.1"]
    assert r["mode"] == "output" and r["channels"] == 3 and r["n"] == 10
    for f in ("err", "shift", "energy", "shift_share"):
        assert sorted(r[f]) == ["after", "before"]
        assert all(v.dtype == torch.float64 and v.shape == (3,) and v.device.type == "cpu" for v in r[f].values())
    assert r["err"]["before"].tolist() == [4.0, 1.6, 0.0] and r["shift"]["after"].tolist() == [0.0, 1.0, 0.0]
    # shift share: shift^2 / (n err) in [0, 1], 0 at err == 0
    assert r["shift_share"]["before"].tolist() == pytest.approx([4.0 / 40.0, 16.0 / 16.0, 0.0], abs=1e-15)
    assert r["shift_share"]["after"].tolist() == pytest.approx([0.0, 1.0 / 1.0, 0.0], abs=1e-15)
    assert r["removed"].tolist() == pytest.approx([0.4, 1.5, 0.0], abs=1e-15)
    # the layers in the order they were corrected, the skipped ones with their reasons
    assert list(r["layers"]) == ["conv2", "conv1"]
    assert r["layers"]["conv2"]["shift"].tolist() == [0.5, -0.25] and r["layers"]["conv2"]["shift"].dtype == torch.float64
    assert r["layers"]["conv2"]["n"] == 40 and r["layers"]["conv2"]["kind"] == "conv" and r["layers"]["conv2"]["max_abs"] == 0.5
    assert r["layers"]["conv1"]["max_abs"] == 3.0 and r["layers"]["conv1"]["kind"] == "tconv"
    assert r["skipped"] == OrderedDict([("gdn", "gdn: why"), ("skip", "no bias")])
    t = r["total"]
    assert t["err"] == {"before": pytest.approx(5.6), "after": pytest.approx(3.7)}
    assert t["shift"] == {"before": pytest.approx(-2.0), "after": pytest.approx(1.0)}
    assert t["energy"] == {"before": 425.0, "after": 425.0}
    assert t["shift_share"]["before"] == pytest.approx(20.0 / 56.0) and t["shift_share"]["after"] == pytest.approx(1.0 / 37.0)
    assert t["removed"] == pytest.approx(1.9)
    r0 = rep["g_a.0"]
    assert r0["mode"] == "weight" and r0["channels"] == 1 and r0["shift_share"]["before"].tolist() == [1.0]
    assert r0["shift_share"]["after"].tolist() == [0.0] and r0["total"]["shift_share"]["after"] == 0.0 and r0["skipped"] == OrderedDict()
    # the read-out copies: the recorded statistics are not aliased
    r["err"]["before"].zero_()
    r["layers"]["conv2"]["shift"].zero_()
    again = bias_report(_model())["g_a.1"]
    assert again["err"]["before"].tolist() == [4.0, 1.6, 0.0] and again["layers"]["conv2"]["shift"].tolist() == [0.5, -0.25]


def test_a_model_without_statistics_reports_nothing():
    from quantization.export import bias_report
    m = torch.nn.Module()
    m.a, m.b = _Unit(), torch.nn.Linear(2, 2)
    assert bias_report(m) == {} and isinstance(bias_report(m), dict)
    m.a.bias_stats = None
    assert bias_report(m) == {}


def test_quant_model_has_the_read_out_and_the_undo():
    from quantization import QuantModel
    assert callable(getattr(QuantModel, "bias_report", None)) and callable(getattr(QuantModel, "clear_bias_correction", None))
