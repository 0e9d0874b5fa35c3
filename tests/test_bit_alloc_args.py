"""CPU checks of the mixed-precision weight widths: include/rdo_ptq_bits.h declares exactly the entries of `EXPORTS_BITS`, the C entry
`rdo_uaq_width_scan` returns RDO_EINVAL with a message that names it for every refusal without touching a device, `ops.uaq_width_scan`
refuses malformed operands with ValueError before any pointer is taken, `bit_report` and `set_weight_bits` refuse bad arguments and
trained modules before anything is done or written, `set_weight_bits` / `weight_bits` round-trip on the toy models (fields only), and
`export.allocate_bits` follows its documented rule on hand-made tables whose costs are dyadic rationals (float64 sums are exact)."""
import ctypes as C
import itertools
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

from test_rd_report_args import _toy

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the header, the exports
def test_header_declares_and_library_exports_the_entries():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_bits.h")).read()
    declared = set(re.findall(r"^int(?:64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == {"rdo_uaq_width_scan", "rdo_uaq_width_scan_workspace"} == set(L.EXPORTS_BITS)
    assert '#include "rdo_ptq_hip.h"' in hdr
    for name, value in (("MAX_K", L.WIDTH_SCAN_MAX_K), ("MIN_BITS", L.WIDTH_SCAN_MIN_BITS), ("MAX_BITS", L.WIDTH_SCAN_MAX_BITS),
                        ("LDS_ROW", L.WIDTH_SCAN_LDS_ROW), ("CHUNK", L.WIDTH_SCAN_CHUNK)):
        assert int(re.search(rf"^#define RDO_WIDTH_SCAN_{name} (\d+)", hdr, re.M).group(1)) == value
    from quantization.quantizer import MAX_BITS
    assert (L.WIDTH_SCAN_MAX_K, L.WIDTH_SCAN_MIN_BITS, L.WIDTH_SCAN_MAX_BITS) == (8, 2, MAX_BITS)
    h = L.lib()
    for name in declared:
        assert hasattr(h, name) and name not in L.EXPORTS and name not in L.EXPORTS_GDN and name not in L.EXPORTS_BIAS
    assert len(L.EXPORTS) == 124


# ----------------------------------------------------------------------------- the C entry
def test_c_entry_refuses_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments below are host addresses that are never dereferenced (the widths are a
    host array by contract)"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    names = ["w", "rows", "inner", "widths", "K", "delta_in", "zp_in", "delta", "zp", "err", "energy", "ws"]

    def call(widths=(4, 6, 8), **kw):
        K = kw.pop("K", 3 if widths is None else len(widths))
        arr = None if widths is None else (C.c_int32 * max(len(widths), 1))(*widths)
        a = dict(w=p, rows=3, inner=40, widths=arr, K=K, delta_in=None, zp_in=None, delta=p, zp=p, err=p, energy=p, ws=p)
        a.update(kw)
        return h.rdo_uaq_width_scan(*[a[n] for n in names], None)

    bad = [dict(w=None), dict(widths=None), dict(delta=None), dict(zp=None), dict(err=None), dict(energy=None), dict(ws=None),
           dict(rows=0), dict(rows=-3), dict(inner=0), dict(inner=-40),
           dict(K=0), dict(K=-1), dict(K=9, widths=tuple(range(2, 11))),
           dict(widths=(1, 4)), dict(widths=(4, 17)), dict(widths=(0,)), dict(widths=(-8,)), dict(widths=(4, 256)),
           dict(widths=(4, 4)), dict(widths=(8, 6, 4, 6)), dict(widths=(2, 3, 4, 5, 6, 7, 8, 2)),
           dict(delta_in=p), dict(zp_in=p),
           dict(err=C.c_void_p(C.addressof(buf) + 4)), dict(ws=C.c_void_p(C.addressof(buf) + 4)),
           dict(rows=2 ** 31 - 1, inner=2 ** 40)]
    for kw in bad:
        assert call(**kw) == RDO_EINVAL, kw
        assert b"rdo_uaq_width_scan" in h.rdo_last_error(), kw
    ws = h.rdo_uaq_width_scan_workspace
    for args in ((0, 40, 3), (-1, 40, 3), (3, 0, 3), (3, -5, 3), (3, 40, 0), (3, 40, 9), (3, 40, -1), (2 ** 31 - 1, 2 ** 40, 3)):
        assert ws(*args) == 0, args
    # accepted geometries: never 0 (ws is never NULL); a split row needs (K + 1) doubles and 2 floats per share
    T, Ck = L.WIDTH_SCAN_LDS_ROW, L.WIDTH_SCAN_CHUNK
    assert ws(3, 40, 3) > 0 and ws(1, T, 8) > 0 and ws(1, T, 8) == ws(3, 40, 3)
    assert ws(2, T + 3, 5) == 2 * 3 * (6 * 8 + 8) and -(-(T + 3) // Ck) == 3
    assert ws(1, 921600, 4) == 225 * (5 * 8 + 8)


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


def test_uaq_width_scan_refuses_malformed_operands(no_library):
    ops = no_library
    w = _t(3, 40)
    ok = (4, 6, 8)
    cases = [
        ((w.double(), ok), {}, "w_rows must be an fp32 tensor"),
        ((None, ok), {}, "w_rows must be an fp32 tensor"),
        ((w.to(torch.int32), ok), {}, "w_rows must be an fp32 tensor"),
        ((_t(120), ok), {}, "rank 2"),
        ((_t(3, 4, 10), ok), {}, "rank 2"),
        ((_t(0, 40), ok), {}, "empty"),
        ((_t(3, 0), ok), {}, "empty"),
        ((_t(3, 80)[:, ::2], ok), {}, "contiguous"),
        ((_t(40, 3).t(), ok), {}, "contiguous"),
        ((w, ()), {}, "1 .. 8 entries"),
        ((w, tuple(range(2, 11))), {}, "1 .. 8 entries"),
        ((w, 8), {}, "widths must be a sequence"),
        ((w, "468"), {}, "widths must be a sequence"),
        ((w, None), {}, "widths must be a sequence"),
        ((w, torch.tensor([4, 8])), {}, "widths must be a sequence"),
        ((w, (4, 1)), {}, "whole number in 2 .. 16"),
        ((w, (17,)), {}, "whole number in 2 .. 16"),
        ((w, (4.0, 8)), {}, "whole number in 2 .. 16"),
        ((w, (True, 8)), {}, "whole number in 2 .. 16"),
        ((w, ("8",)), {}, "whole number in 2 .. 16"),
        ((w, (4, 8, 4)), {}, "distinct"),
        ((w, ok), {"delta": _t(3, 3)}, "given together"),
        ((w, ok), {"zp": _t(3, 3)}, "given together"),
        ((w, ok), {"delta": _t(3, 4), "zp": _t(3, 3)}, "delta must be a contiguous fp32 \\[3, 3\\]"),
        ((w, ok), {"delta": _t(3, 3), "zp": _t(9)}, "zp must be a contiguous fp32 \\[3, 3\\]"),
        ((w, ok), {"delta": _t(3, 3).double(), "zp": _t(3, 3)}, "delta must be a contiguous fp32"),
        ((w, ok), {"delta": _t(3, 3), "zp": _t(3, 6)[:, ::2]}, "zp must be a contiguous fp32"),
        ((w, ok), {"delta": _t(3, 3), "zp": torch.zeros(3, 3, device="meta")}, "zp must be a contiguous fp32"),
        ((w, ok), {"delta": 0.1, "zp": _t(3, 3)}, "delta must be a contiguous fp32"),
        ((torch.zeros(2 ** 20, 2 ** 24, device="meta"), ok), {}, "more shares than 32-bit"),
        ((w, ok), {}, "no CPU path"),
        ((w, [np.int64(4), np.int32(8)]), {}, "no CPU path"),                       # numpy integers count
        ((w, (8,)), {"delta": _t(1, 3), "zp": _t(1, 3)}, "no CPU path"),
        ((_t(1, 1), (2, 3, 4, 5, 6, 7, 8, 16)), {}, "no CPU path"),
    ]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=f"uaq_width_scan: .*{what}"):
            ops.uaq_width_scan(*args, **kw)


# ----------------------------------------------------------------------------- bit_report / set_weight_bits: refusals
def _quantiser_fields(qnn):
    from quantization import QuantModule
    out = []
    for m in qnn.modules():
        if isinstance(m, QuantModule):
            for q in (m.weight_quantizer, m.act_quantizer):
                out.append((id(q), q.n_bits, q.n_levels, q.inited, None if q.delta is None else id(q.delta),
                            None if q.zero_point is None else id(q.zero_point)))
            out.append((m.use_weight_quant, m.use_act_quant, m.trained))
    return out


def test_bit_report_refuses_bad_arguments_before_any_gpu_work(monkeypatch):
    from hipops import _lib as L
    from quantization import QuantModel
    from quantization.export import bit_report
    qnn = _toy("cheng")
    before = _quantiser_fields(qnn)

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(QuantModel, "forward", boom)
    img = torch.rand(2, 3, 64, 128)
    cases = [
        (dict(images=torch.rand(3, 64, 64)), "images must be \\[n, 3, H, W\\]"),
        (dict(images=torch.rand(0, 3, 64, 64)), "images is empty"),
        (dict(images=torch.rand(2, 3, 64, 96)), "multiples of 64"),
        (dict(images=torch.rand(2, 3, 64, 64).double()), "images must be an fp32 tensor"),
        (dict(lmbda=0.0), "lmbda must be a positive finite number"),
        (dict(lmbda=float("nan")), "lmbda must be a positive finite number"),
        (dict(lmbda=True), "lmbda must be a positive finite number"),
        (dict(batch=0), "batch must be an integer >= 1"),
        (dict(batch=2.0), "batch must be an integer >= 1"),
        (dict(units=["g_a.0", "g_a.99"]), "unknown unit name\\(s\\) \\['g_a.99'\\]"),
        (dict(units="g_a.0"), "units must be None or a list of unit names"),
        (dict(widths=()), "1 .. 8 entries"),
        (dict(widths=tuple(range(2, 11))), "1 .. 8 entries"),
        (dict(widths=8), "widths must be a sequence"),
        (dict(widths=(4, 1)), "whole number in 2 .. 16"),
        (dict(widths=(4, 17)), "whole number in 2 .. 16"),
        (dict(widths=(4.0,)), "whole number in 2 .. 16"),
        (dict(widths=(True, 4)), "whole number in 2 .. 16"),
        (dict(widths=(4, 8, 4)), "distinct"),
    ]
    for kw in cases:
        kw, what = dict(dict(images=img), **kw[0]), kw[1]
        with pytest.raises(ValueError, match=f"bit_report: .*{what}"):
            bit_report(qnn, **kw)
        with pytest.raises(ValueError, match=f"bit_report: .*{what}"):
            qnn.bit_report(**kw)
    # a module made "trained" by hand: its unit is refused, whether it is chosen by name or by default; other units are not its business
    from quantization.export import weighted_modules
    m = weighted_modules(qnn.units()["g_a.0"])[-1]
    m.trained = True
    for kw in (dict(), dict(units=["g_a.0", "g_a.1"])):
        with pytest.raises(ValueError, match="bit_report: unit 'g_a.0' holds a trained module"):
            qnn.bit_report(img, **kw)
    m.trained = False
    # the argument checks are passed: the scan is the first GPU work, and on a CPU model it refuses; everything is put back
    with pytest.raises(ValueError, match="uaq_width_scan: .*no CPU path"):
        qnn.bit_report(img, units=["g_a.1"])
    assert before == _quantiser_fields(qnn)


def test_an_adaround_quantiser_counts_as_trained():
    from quantization.export import is_trained
    from quantization.quantizer import AdaRoundQuantizer
    qnn = _toy("cheng")
    m = qnn.units()["g_a.6"]
    assert not is_trained(m)
    uaq = m.weight_quantizer
    uaq.delta, uaq.zero_point = torch.ones(m.weight.shape[0], 1, 1, 1), torch.zeros(m.weight.shape[0], 1, 1, 1)
    rows = uaq._rows(m.weight.detach())
    m.weight_quantizer = AdaRoundQuantizer(uaq, m.weight.data, round_mode="learned_hard_sigmoid", alpha_rows=torch.zeros_like(rows))
    assert is_trained(m) and not m.trained
    with pytest.raises(ValueError, match="bit_report: unit 'g_a.6' holds a trained module"):
        qnn.bit_report(torch.rand(1, 3, 64, 64), units=["g_a.6"])
    with pytest.raises(ValueError, match="set_weight_bits: unit 'g_a.6' holds a trained module"):
        qnn.set_weight_bits(6)


def test_set_weight_bits_refuses_before_anything_is_written():
    qnn = _toy("cheng")
    before = _quantiser_fields(qnn)
    names = list(qnn.units())
    cases = [
        (None, "bits must be a whole number in 2 .. 16 or a mapping"),
        (1, "bits must be a whole number"),
        (17, "bits must be a whole number"),
        (6.0, "bits must be a whole number"),
        (True, "bits must be a whole number"),
        ("6", "bits must be a whole number"),
        ([6, 6], "bits must be a whole number"),
        ({"g_a.99": 6}, "unknown unit name\\(s\\) \\['g_a.99'\\]"),
        ({names[0]: 6, "model.g_a.0": 6}, "unknown unit name"),
        ({names[0]: 6, names[1]: 1}, f"the width of unit '{re.escape(names[1])}' must be a whole number"),
        ({names[0]: 6, names[-1]: 6.5}, "must be a whole number in 2 .. 16"),
        ({names[0]: 6, names[2]: None}, "must be a whole number in 2 .. 16"),
        ({names[0]: True}, "must be a whole number in 2 .. 16"),
    ]
    for bits, what in cases:
        with pytest.raises(ValueError, match=f"set_weight_bits: .*{what}"):
            qnn.set_weight_bits(bits)
        assert before == _quantiser_fields(qnn)
    # a trained module in the LAST named unit: the first one is not written either
    from quantization.export import weighted_modules
    last = weighted_modules(qnn.units()[names[-1]])[-1]
    for bits in (6, {names[0]: 6, names[-1]: 4}):
        last.trained = True
        with pytest.raises(ValueError, match=f"set_weight_bits: unit '{re.escape(names[-1])}' holds a trained module"):
            qnn.set_weight_bits(bits)
        last.trained = False
        assert before == _quantiser_fields(qnn)
    qnn.set_weight_bits({names[0]: 6})                                          # units that are not named are not looked at
    assert before != _quantiser_fields(qnn)


# ----------------------------------------------------------------------------- set_weight_bits / weight_bits
@pytest.mark.parametrize("arch", ["cheng", "minnen", "lu2022"])
def test_set_weight_bits_and_weight_bits_round_trip(arch):
    """fields only: no kernel runs, so the CPU-built toy models do"""
    from quantization import QuantModule
    qnn = _toy(arch)
    units = qnn.units()
    names = list(units)

    def weighted(u):
        return [(n, m) for n, m in u.named_modules() if isinstance(m, QuantModule) and m.org_weight is not None]
    for u in units.values():                                                    # as if a forward had initialised the scales
        for _, m in weighted(u):
            m.weight_quantizer.inited, m._pack_memo = True, {"q": "stale"}
    act = [(id(m.act_quantizer), m.act_quantizer.n_bits, m.act_quantizer.n_levels) for m in qnn.modules() if hasattr(m, "act_quantizer")]
    first = qnn.weight_bits()
    assert list(first) == names + ["total"]
    count = sum(p.numel() for u in units.values() for _, m in weighted(u) for p in [m.weight])
    assert first["total"] == {"weights": count, "size_bits": 8 * count, "avg_bits": 8.0}
    for n in names:
        mods = weighted(units[n])
        assert list(first[n]["bits"]) == [mn for mn, _ in mods] and set(first[n]["bits"].values()) == {8}
        assert first[n]["weights"] == sum(m.weight.numel() for _, m in mods) and first[n]["size_bits"] == 8 * first[n]["weights"]
    plan = OrderedDict((n, 3 + k % 5) for k, n in enumerate(names[:-2]))          # the last two units keep their width
    qnn.set_weight_bits(plan)
    got = qnn.weight_bits()
    size = 0
    for n in names:
        b = plan.get(n, 8)
        for _, m in weighted(units[n]):
            q = m.weight_quantizer
            assert (q.n_bits, q.n_levels) == (b, 2 ** b) and q.inited == (n not in plan) and (m._pack_memo == {}) == (n in plan)
        assert set(got[n]["bits"].values()) == {b} and got[n]["size_bits"] == b * first[n]["weights"] == b * got[n]["weights"]
        size += got[n]["size_bits"]
    assert got["total"] == {"weights": count, "size_bits": size, "avg_bits": size / count}
    assert act == [(id(m.act_quantizer), m.act_quantizer.n_bits, m.act_quantizer.n_levels) for m in qnn.modules() if hasattr(m, "act_quantizer")]
    qnn.set_weight_bits(np.int64(5))                                            # one width for every unit; numpy integers count
    assert qnn.weight_bits()["total"] == {"weights": count, "size_bits": 5 * count, "avg_bits": 5.0}
    assert all(isinstance(m.weight_quantizer.n_bits, int) and not m.weight_quantizer.inited for u in units.values() for _, m in weighted(u))


# ----------------------------------------------------------------------------- allocate_bits
def _table(costs, weights, widths=(4, 6, 8)):
    """costs: name -> [d_loss per width]"""
    rep = OrderedDict(units=OrderedDict(), weights=OrderedDict())
    for (name, cs), w in zip(costs.items(), weights):
        rep["weights"][name] = w
        rep["units"][name] = OrderedDict((b, {"size_bits": b * w, "d_loss": c}) for b, c in zip(widths, cs))
    return rep


def test_allocation_starts_at_the_least_cost_and_prunes_to_the_hull():
    from quantization.export import allocate_bits
    rep = _table(OrderedDict(a=[4.0, 1.0, 0.5],         # convex: every point on the hull
                             b=[2.0, 1.75, 0.0],        # 6 bits above the chord 4 -> 8 (8 -> 6 costs 1.75 / 32 a bit, 6 -> 4 only 0.25 / 32)
                             c=[1.0, 0.25, 0.5],        # 8 bits costs more than 6: dropped, the start is 6
                             d=[0.5, 3.0, -0.25],       # non-monotone, a negative cost (noise of either sign): hull {4, 8}
                             e=[1.0, 1.0, 1.0]),        # equal costs: the smallest is the least-cost point, nothing to step
                 [16, 16, 16, 16, 16])
    free = allocate_bits(rep, budget_bits=10 ** 6)
    assert free["bits"] == OrderedDict(a=8, b=8, c=6, d=8, e=4) and free["steps"] == []
    assert free["size_bits"] == 16 * 34 and free["cost"] == 0.5 + 0.0 + 0.25 - 0.25 + 1.0 and free["budget_bits"] == 10 ** 6
    assert free["avg_bits"] == 34 / 5
    # every step in slope order: d 8->4 (0.75 / 64), a 8->6 (0.5 / 32), c 6->4 (0.75 / 32), b 8->4 (2 / 64), a 6->4 (3 / 32)
    low = allocate_bits(rep, budget_bits=16 * 20)
    assert low["steps"] == [("d", 8, 4, 0.75 / 64), ("a", 8, 6, 0.5 / 32), ("c", 6, 4, 0.75 / 32), ("b", 8, 4, 2.0 / 64), ("a", 6, 4, 3.0 / 32)]
    assert low["bits"] == OrderedDict(a=4, b=4, c=4, d=4, e=4) and low["size_bits"] == 16 * 20 and low["cost"] == 4.0 + 2.0 + 1.0 + 0.5 + 1.0
    # the first total <= budget stops it, even where the step overshoots (d saves 64 bits where 1 was asked for)
    mid = allocate_bits(rep, budget_bits=16 * 34 - 1)
    assert mid["steps"] == low["steps"][:1] and mid["size_bits"] == 16 * 30 and mid["bits"] == OrderedDict(a=8, b=8, c=6, d=4, e=4)
    assert mid["cost"] == 0.5 + 0.0 + 0.25 + 0.5 + 1.0
    two = allocate_bits(rep, budget_bits=16 * 30 - 1)
    assert two["steps"] == low["steps"][:2] and two["size_bits"] == 16 * 28 and two["bits"] == OrderedDict(a=6, b=8, c=6, d=4, e=4)


def test_allocation_ties_go_to_the_earlier_unit():
    from quantization.export import allocate_bits
    rep = _table(OrderedDict(x=[3.0, 1.0, 0.0], y=[3.0, 1.0, 0.0], z=[3.0, 1.0, 0.0]), [8, 8, 8])
    got = allocate_bits(rep, budget_bits=8 * 24 - 1)
    assert got["steps"] == [("x", 8, 6, 1.0 / 16)] and got["bits"] == OrderedDict(x=6, y=8, z=8)
    got = allocate_bits(rep, budget_bits=8 * 18 - 1)
    assert [s[:3] for s in got["steps"]] == [("x", 8, 6), ("y", 8, 6), ("z", 8, 6), ("x", 6, 4)]
    # points on one chord are kept, so a unit can stop between them
    line = _table(OrderedDict(p=[2.0, 1.0, 0.0], q=[8.0, 4.0, 0.0]), [8, 8])
    got = allocate_bits(line, budget_bits=8 * 14)
    assert got["bits"] == OrderedDict(p=6, q=8) and got["steps"] == [("p", 8, 6, 1.0 / 16)]


def test_allocation_with_fixed_units_and_both_budget_forms():
    from quantization.export import allocate_bits
    rep = _table(OrderedDict(a=[4.0, 1.0, 0.5], b=[2.0, 1.75, 0.0], c=[1.0, 0.25, 0.5]), [16, 32, 16])
    got = allocate_bits(rep, avg_bits=6.0, fixed={"b": 8})
    assert got["budget_bits"] == 6 * 64 and got["bits"]["b"] == 8 and all(s[0] != "b" for s in got["steps"])
    assert got["bits"] == OrderedDict(a=4, b=8, c=4) and got["size_bits"] == 64 + 256 + 64 and got["avg_bits"] == 6.0
    same = allocate_bits(rep, budget_bits=6 * 64, fixed={"b": 8})
    assert same == got
    assert allocate_bits(rep, avg_bits=5.99, fixed={"a": 6})["budget_bits"] == int(np.floor(5.99 * 64))
    up = allocate_bits(rep, budget_bits=10 ** 6, fixed={"c": 8, "a": 4})       # a fixed width need not be on the hull
    assert up["bits"] == OrderedDict(a=4, b=8, c=8) and up["cost"] == 4.0 + 0.0 + 0.5
    for kw, what in [(dict(), "exactly one of budget_bits and avg_bits"), (dict(budget_bits=400, avg_bits=6.0), "exactly one"),
                     (dict(budget_bits=0), "budget_bits must be a whole number >= 1"), (dict(budget_bits=400.0), "budget_bits must be a whole"),
                     (dict(budget_bits=True), "budget_bits must be a whole"), (dict(avg_bits=0), "avg_bits must be a positive finite"),
                     (dict(avg_bits=float("nan")), "avg_bits must be a positive finite"), (dict(avg_bits="6"), "avg_bits must be a positive"),
                     (dict(avg_bits=6, fixed={"zz": 8}), "fixed names the unknown unit 'zz'"), (dict(avg_bits=6, fixed={"a": 5}), "the width 5"),
                     (dict(avg_bits=6, fixed=["a"]), "fixed must be None or a dict")]:
        with pytest.raises(ValueError, match=f"allocate_bits: .*{what}"):
            allocate_bits(rep, **kw)
    for bad in (None, {}, {"units": {}}, OrderedDict(units=OrderedDict(a={}), weights=OrderedDict(a=4)),
                OrderedDict(units=OrderedDict(a={4: {"size_bits": 16}}), weights=OrderedDict(a=4)),
                OrderedDict(units=OrderedDict(a={4: {"size_bits": 16, "d_loss": float("nan")}}), weights=OrderedDict(a=4)),
                OrderedDict(units=OrderedDict(a={4: {"size_bits": 16, "d_loss": 1.0}}), weights=OrderedDict(b=4))):
        with pytest.raises(ValueError, match="allocate_bits: "):
            allocate_bits(bad, budget_bits=100)


def test_an_unreachable_budget_names_the_smallest_size():
    from quantization.export import allocate_bits
    rep = _table(OrderedDict(a=[4.0, 1.0, 0.5], b=[2.0, 1.75, 0.0]), [16, 32])
    assert allocate_bits(rep, budget_bits=4 * 48)["size_bits"] == 4 * 48
    with pytest.raises(ValueError, match="allocate_bits: the smallest reachable size is 192 bits; the budget is 191"):
        allocate_bits(rep, budget_bits=4 * 48 - 1)
    with pytest.raises(ValueError, match="the smallest reachable size is 320 bits"):
        allocate_bits(rep, avg_bits=4.0, fixed={"b": 8})


def test_no_assignment_within_the_returned_size_costs_less():
    """5 units x 3 widths, costs dyadic (multiples of 1/64 below 2^10: every float64 sum is exact), a sweep of budgets: brute force over
    all 243 assignments finds none of size <= the returned size with a lower cost"""
    from quantization.export import allocate_bits
    g = np.random.default_rng(7)
    widths = (3, 5, 8)
    for trial in range(6):
        weights = [int(v) for v in g.integers(1, 40, 5)]
        costs = OrderedDict((f"u{k}", [float(v) / 64 for v in g.integers(-64, 4096, 3)]) for k in range(5))
        if trial % 2 == 0:                                                      # the usual shape: falling with the width, roughly
            costs = OrderedDict((n, sorted(cs, reverse=True)) for n, cs in costs.items())
        rep = _table(costs, weights, widths)
        every = []
        for pick in itertools.product(range(3), repeat=5):
            every.append((sum(widths[i] * w for i, w in zip(pick, weights)), sum(cs[i] for i, cs in zip(pick, costs.values()))))
        lo, hi = 3 * sum(weights), 8 * sum(weights)
        seen = set()
        for budget in range(lo, hi + 1, max(1, (hi - lo) // 60)):
            got = allocate_bits(rep, budget_bits=budget)
            assert got["size_bits"] <= budget
            assert got["size_bits"] == sum(got["bits"][n] * w for n, w in zip(costs, weights))
            assert got["cost"] == sum(cs[widths.index(got["bits"][n])] for n, cs in costs.items())
            assert not [1 for size, cost in every if size <= got["size_bits"] and cost < got["cost"]]
            slopes = [s[3] for s in got["steps"]]
            assert slopes == sorted(slopes) and all(s >= 0 for s in slopes)
            seen.add(got["size_bits"])
        assert len(seen) > 3
        with pytest.raises(ValueError, match=f"smallest reachable size is {lo} bits"):
            allocate_bits(rep, budget_bits=lo - 1)
