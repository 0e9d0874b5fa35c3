"""CPU checks of the activation widths per unit: include/rdo_ptq_actbits.h declares exactly the entries of `EXPORTS_ACTBITS`, the C entry
`rdo_actquant_width_scan` returns RDO_EINVAL with a message that names it for every refusal without touching a device,
`ops.actquant_width_scan` refuses malformed operands with ValueError before any pointer is taken, `act_bit_report`, `act_width_report`,
`set_act_bits` and `allocate_act_bits` refuse bad arguments before anything is done or written, `set_act_bits` / `act_bits` round-trip on
the toy models (fields only), `act_scan` refuses an unfrozen static quantiser and an active phase, and `allocate_act_bits` is
`allocate_bits` on the renamed table."""
import ctypes as C
import os
import pickle
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
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_actbits.h")).read()
    declared = set(re.findall(r"^int(?:64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == {"rdo_actquant_width_scan", "rdo_actquant_width_scan_workspace"} == set(L.EXPORTS_ACTBITS)
    assert '#include "rdo_ptq_hip.h"' in hdr
    for name, value in (("MAX_K", L.ACT_WIDTH_SCAN_MAX_K), ("MIN_BITS", L.ACT_WIDTH_SCAN_MIN_BITS), ("MAX_BITS", L.ACT_WIDTH_SCAN_MAX_BITS)):
        assert int(re.search(rf"^#define RDO_ACT_WIDTH_SCAN_{name} (\d+)", hdr, re.M).group(1)) == value
    from quantization.quantizer import MAX_BITS
    assert (L.ACT_WIDTH_SCAN_MAX_K, L.ACT_WIDTH_SCAN_MIN_BITS, L.ACT_WIDTH_SCAN_MAX_BITS) == (8, 2, MAX_BITS)
    assert (L.ACT_WIDTH_SCAN_MAX_K, L.ACT_WIDTH_SCAN_MIN_BITS) == (L.WIDTH_SCAN_MAX_K, L.WIDTH_SCAN_MIN_BITS)     # `ops.width_list` serves both
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_BIAS, L.EXPORTS_BITS, L.EXPORTS_PACK, L.EXPORTS_SUBPEL)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert len(L.EXPORTS) == 124


# ----------------------------------------------------------------------------- the C entry
def test_c_entry_refuses_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments below are host addresses that are never dereferenced (the widths are a
    host array by contract)"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    names = ["x", "npix", "C", "range", "widths", "K", "err", "energy", "ws"]

    def call(widths=(4, 6, 8), **kw):
        K = kw.pop("K", 3 if widths is None else len(widths))
        arr = None if widths is None else (C.c_int32 * max(len(widths), 1))(*widths)
        a = dict(x=p, npix=35, C=6, range=p, widths=arr, K=K, err=p, energy=p, ws=p)
        a.update(kw)
        return h.rdo_actquant_width_scan(*[a[n] for n in names], None)

    bad = [dict(x=None), dict(range=None), dict(widths=None), dict(err=None), dict(ws=None),
           dict(x=None, energy=None),                                                 # (a null energy alone is allowed: see the GPU tests)
           dict(npix=0), dict(npix=-35), dict(npix=2 ** 31), dict(npix=2 ** 40),
           dict(C=0), dict(C=-6), dict(C=2 ** 31 - 1),
           dict(K=0), dict(K=-1), dict(K=9, widths=tuple(range(2, 11))),
           dict(widths=(1, 4)), dict(widths=(4, 17)), dict(widths=(0,)), dict(widths=(-8,)), dict(widths=(4, 256)),
           dict(widths=(4, 4)), dict(widths=(8, 6, 4, 6)), dict(widths=(2, 3, 4, 5, 6, 7, 8, 2))]
    for kw in bad:
        assert call(**kw) == RDO_EINVAL, kw
        assert b"rdo_actquant_width_scan" in h.rdo_last_error(), kw
    ws = h.rdo_actquant_width_scan_workspace
    for args in ((0, 3), (-1, 3), (6, 0), (6, 9), (6, -1), (2 ** 31 - 1, 3)):
        assert ws(*args) == 0, args
    # accepted geometries: (K + 1) floats per channel for each of the 256 workgroups
    assert ws(6, 3) == 6 * 4 * 256 and ws(192, 8) == 192 * 9 * 256 and ws(1, 1) == 2 * 256


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


def test_actquant_width_scan_refuses_malformed_operands(no_library):
    ops = no_library
    x, r = _t(35, 6), _t(12)
    ok = (4, 6, 8)
    cases = [
        ((x.double(), r, ok), "x must be an fp32 tensor"),
        ((None, r, ok), "x must be an fp32 tensor"),
        ((x.to(torch.int32), r, ok), "x must be an fp32 tensor"),
        ((_t(0, 6), r, ok), "empty"),
        ((_t(35, 12)[:, ::2], r, ok), "contiguous"),
        ((_t(6, 35).t(), r, ok), "contiguous"),
        ((torch.tensor(1.0), r, ok), "got a scalar"),
        ((x, _t(10), ok), "rng must be a contiguous fp32 \\[12\\]"),
        ((x, _t(2, 6), ok), "rng must be a contiguous fp32 \\[12\\]"),
        ((x, r.double(), ok), "rng must be a contiguous fp32 \\[12\\]"),
        ((x, _t(24)[::2], ok), "rng must be a contiguous fp32 \\[12\\]"),
        ((x, torch.zeros(12, device="meta"), ok), "rng must be a contiguous fp32 \\[12\\] on cpu"),
        ((x, None, ok), "rng must be a contiguous fp32"),
        ((x, r, ()), "1 .. 8 entries"),
        ((x, r, tuple(range(2, 11))), "1 .. 8 entries"),
        ((x, r, 8), "widths must be a sequence"),
        ((x, r, "468"), "widths must be a sequence"),
        ((x, r, None), "widths must be a sequence"),
        ((x, r, torch.tensor([4, 8])), "widths must be a sequence"),
        ((x, r, (4, 1)), "whole number in 2 .. 16"),
        ((x, r, (17,)), "whole number in 2 .. 16"),
        ((x, r, (4.0, 8)), "whole number in 2 .. 16"),
        ((x, r, (True, 8)), "whole number in 2 .. 16"),
        ((x, r, (4, 8, 4)), "distinct"),
        ((torch.zeros(2 ** 31, 2, device="meta"), torch.zeros(4, device="meta"), ok), "beyond 32-bit pixel counts"),
        ((x, r, ok), "no CPU path"),
        ((x, r, [np.int64(4), np.int32(8)]), "no CPU path"),                        # numpy integers count
        ((_t(2, 5, 7, 6), _t(12), (2, 3, 4, 5, 6, 7, 8, 16)), "no CPU path"),       # [..., C] of any rank
    ]
    for args, what in cases:
        with pytest.raises(ValueError, match=f"actquant_width_scan: .*{what}"):
            ops.actquant_width_scan(*args)


# ----------------------------------------------------------------------------- the quantiser hook: refusals
def test_act_scan_refuses_an_unfrozen_static_quantiser_and_an_active_phase():
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(act=True, act_mode="static")
    for phase in ("idle", "observe", "search", "hist", "search+hist", "score", "learn"):
        q.act_phase = phase
        with pytest.raises(RuntimeError, match="act_scan: "):
            q.act_scan((4, 8))
        assert q.act_scan_widths is None
    q.act_phase = "frozen"
    q.act_scan([4, np.int64(8)])
    assert q.act_scan_widths == [4, 8] and q.act_scan_close() == {} and q.act_scan_widths is None
    d = UniformAffineQuantizer(act=True)
    for phase in ("observe", "search", "hist", "score", "learn"):
        d.act_phase = phase
        with pytest.raises(RuntimeError, match="act_scan: "):
            d.act_scan((4, 8))
    d.act_phase = "idle"
    for widths, what in (((), "1 .. 8 entries"), ((4, 4), "distinct"), ((1,), "whole number in 2 .. 16"), (8, "must be a sequence")):
        with pytest.raises(ValueError, match=f"act_scan: .*{what}"):
            d.act_scan(widths)
    d.act_scan((6,))
    assert d.act_scan_widths == [6]
    d.act_scan_close()
    # a quantiser pickled before the fields existed: they are read with getattr
    old = UniformAffineQuantizer(act=True)
    del old.act_scan_widths, old.act_scan_sums
    old = pickle.loads(pickle.dumps(old))
    assert not hasattr(old, "act_scan_widths") and old.act_scan_close() == {}
    assert old.act_scan_widths is None


# ----------------------------------------------------------------------------- the reports and the setter: refusals
def _act_fields(qnn):
    from quantization import BaseQuantBlock, QuantModule
    out = []
    for m in qnn.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            q = m.act_quantizer
            out.append((id(q), q.dynamic_bits, q.act_mode, q.act_phase, id(q.act_stats), sorted(q.act_stats), q.act_scan_widths,
                        m.use_weight_quant, m.use_act_quant, m.trained))
    return out


def _mark_trained(unit):
    from quantization import BaseQuantBlock, QuantModule
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.trained = True


IMAGE_CASES = [
    (dict(images=torch.rand(3, 64, 64)), "images must be \\[n, 3, H, W\\]"),
    (dict(images=torch.rand(0, 3, 64, 64)), "images is empty"),
    (dict(images=torch.rand(2, 3, 64, 96)), "multiples of 64"),
    (dict(images=torch.rand(2, 3, 64, 64).double()), "images must be an fp32 tensor"),
    (dict(batch=0), "batch must be an integer >= 1"),
    (dict(batch=2.0), "batch must be an integer >= 1"),
    (dict(widths=()), "1 .. 8 entries"),
    (dict(widths=tuple(range(2, 11))), "1 .. 8 entries"),
    (dict(widths=8), "widths must be a sequence"),
    (dict(widths=(4, 1)), "whole number in 2 .. 16"),
    (dict(widths=(4, 17)), "whole number in 2 .. 16"),
    (dict(widths=(4.0,)), "whole number in 2 .. 16"),
    (dict(widths=(True, 4)), "whole number in 2 .. 16"),
    (dict(widths=(4, 8, 4)), "distinct"),
]


def test_the_reports_refuse_bad_arguments_before_any_gpu_work(monkeypatch):
    from hipops import _lib as L
    from quantization import QuantModel
    from quantization.export import act_bit_report, act_width_report
    qnn = _toy("cheng")
    _mark_trained(qnn.units()["g_a.0"])
    before = _act_fields(qnn)

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(QuantModel, "forward", boom)
    img = torch.rand(2, 3, 64, 128)
    more = [
        (dict(lmbda=0.0), "lmbda must be a positive finite number"),
        (dict(lmbda=float("nan")), "lmbda must be a positive finite number"),
        (dict(lmbda=True), "lmbda must be a positive finite number"),
        (dict(units=["g_a.0", "g_a.99"]), "unknown unit name\\(s\\) \\['g_a.99'\\]"),
        (dict(units="g_a.0"), "units must be None or a list of unit names"),
        (dict(weight_quant=1), "weight_quant must be True or False"),
        (dict(weight_quant=None), "weight_quant must be True or False"),
        # a named unit in which nothing is applied: nothing trained
        (dict(units=["g_a.0", "g_a.1"]), "unit 'g_a.1': no activation quantiser of the unit is applied"),
    ]
    for kw, what in IMAGE_CASES + more:
        kw = dict(dict(images=img), **kw)
        with pytest.raises(ValueError, match=f"act_bit_report: .*{what}"):
            act_bit_report(qnn, **kw)
        with pytest.raises(ValueError, match=f"act_bit_report: .*{what}"):
            qnn.act_bit_report(**kw)
    for kw, what in IMAGE_CASES:
        kw = dict(dict(images=img), **kw)
        with pytest.raises(ValueError, match=f"act_width_report: .*{what}"):
            act_width_report(qnn, **kw)
        with pytest.raises(ValueError, match=f"act_width_report: .*{what}"):
            qnn.act_width_report(**kw)
    from quantization import QuantModule
    m = qnn.units()["g_a.6"]                                                      # a layer unit: trained, but its one quantiser disabled
    assert isinstance(m, QuantModule) and not m.disable_act_quant
    m.trained, m.disable_act_quant = True, True
    with pytest.raises(ValueError, match="act_bit_report: unit 'g_a.6': no activation quantiser of the unit is applied"):
        qnn.act_bit_report(img, units=["g_a.6"])
    m.trained, m.disable_act_quant = False, False
    assert before == _act_fields(qnn)
    # the argument checks are passed: the first forward is the first GPU work
    with pytest.raises(AssertionError, match="reached the library"):
        qnn.act_bit_report(img, units=["g_a.0"])
    with pytest.raises(AssertionError, match="reached the library"):
        qnn.act_width_report(img)
    assert before == _act_fields(qnn)                                             # widths, scans and flags are put back after a failure too


def test_set_act_bits_refuses_before_anything_is_written():
    qnn = _toy("cheng")
    before = _act_fields(qnn)
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
        with pytest.raises(ValueError, match=f"set_act_bits: .*{what}"):
            qnn.set_act_bits(bits)
        assert before == _act_fields(qnn)
    qnn.set_act_bits({names[0]: 6})
    assert before != _act_fields(qnn)


@pytest.mark.parametrize("arch", ["cheng", "minnen", "lu2022"])
def test_set_act_bits_and_act_bits_round_trip(arch):
    """fields only: no kernel runs, so the CPU-built toy models do"""
    from quantization import BaseQuantBlock, QuantModule
    qnn = _toy(arch)
    units = qnn.units()
    names = list(units)

    def holders(u):
        return [(n, m) for n, m in u.named_modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    weights = [(id(m.weight_quantizer), m.weight_quantizer.n_bits, m.weight_quantizer.inited) for m in qnn.modules()
               if isinstance(m, QuantModule)]
    first = qnn.act_bits()
    assert list(first) == names
    for n in names:
        assert list(first[n]["bits"]) == [mn for mn, _ in holders(units[n])] and set(first[n]["bits"].values()) == {8}
        assert first[n]["applied"] == [] and "" in first[n]["bits"]
    # as if the calibration had frozen a range and recorded statistics on every quantiser, and trained the first unit
    for u in units.values():
        for _, m in holders(u):
            q = m.act_quantizer
            q.act_range, q.act_stats, q.act_phase = {0: torch.zeros(4)}, {0: {"n": 1}}, "frozen"
    _mark_trained(units[names[0]])
    plan = OrderedDict((n, 3 + k % 5) for k, n in enumerate(names[:-2]))          # the last two units keep their width
    qnn.set_act_bits(plan)
    got = qnn.act_bits()
    for n in names:
        b = plan.get(n, 8)
        for _, m in holders(units[n]):
            q = m.act_quantizer
            assert q.dynamic_bits == b and isinstance(q.dynamic_bits, int) and (q.act_stats == {}) == (n in plan)
            assert sorted(q.act_range) == [0] and q.act_phase == "frozen" and q.n_bits == 8          # frozen ranges stay; n_bits is the weights' field
        assert set(got[n]["bits"].values()) == {b}
    applied = [mn for mn, m in holders(units[names[0]]) if not getattr(m, "disable_act_quant", False)]
    assert got[names[0]]["applied"] == applied and applied and got[names[1]]["applied"] == []
    assert weights == [(id(m.weight_quantizer), m.weight_quantizer.n_bits, m.weight_quantizer.inited) for m in qnn.modules()
                       if isinstance(m, QuantModule)]
    qnn.set_act_bits(np.int64(5))                                               # one width for every unit; numpy integers count; after "calibration" too
    assert all(set(r["bits"].values()) == {5} for r in qnn.act_bits().values())
    back = pickle.loads(pickle.dumps(qnn))
    assert back.act_bits() == qnn.act_bits()


# ----------------------------------------------------------------------------- allocate_act_bits
def _table(costs, elements, widths=(4, 6, 8), key="elements"):
    rep = OrderedDict([("units", OrderedDict()), (key, OrderedDict())])
    for (name, cs), w in zip(costs.items(), elements):
        rep[key][name] = w
        rep["units"][name] = OrderedDict((b, {"size_bits": b * w, "d_loss": c}) for b, c in zip(widths, cs))
    return rep


def test_allocation_is_allocate_bits_on_the_renamed_table():
    from quantization.export import allocate_act_bits, allocate_bits
    costs = OrderedDict(a=[4.0, 1.0, 0.5], b=[2.0, 1.75, 0.0], c=[1.0, 0.25, 0.5], d=[0.5, 3.0, -0.25], e=[1.0, 1.0, 1.0])
    elements = [16, 32, 16, 48, 16]
    rep, renamed = _table(costs, elements), _table(costs, elements, key="weights")
    for kw in (dict(budget_bits=10 ** 6), dict(budget_bits=128 * 5), dict(avg_bits=6.0), dict(avg_bits=5.99, fixed={"a": 6}),
               dict(budget_bits=128 * 4), dict(avg_bits=6, fixed={"b": 8, "d": 4})):
        got, want = allocate_act_bits(rep, **kw), allocate_bits(renamed, **kw)
        assert got == want and list(got["bits"]) == list(costs)
    assert allocate_act_bits(rep, budget_bits=128 * 4)["bits"] == OrderedDict(a=4, b=4, c=4, d=4, e=4)
    low = allocate_act_bits(rep, avg_bits=6.0)
    assert low["size_bits"] <= low["budget_bits"] == 6 * 128 and low["steps"]
    for kw, what in [(dict(), "exactly one of budget_bits and avg_bits"), (dict(budget_bits=400, avg_bits=6.0), "exactly one"),
                     (dict(budget_bits=0), "budget_bits must be a whole number >= 1"), (dict(avg_bits=0), "avg_bits must be a positive finite"),
                     (dict(avg_bits=6, fixed={"zz": 8}), "fixed names the unknown unit 'zz'"), (dict(avg_bits=6, fixed={"a": 5}), "the width 5"),
                     (dict(budget_bits=128 * 4 - 1), "the smallest reachable size is 512 bits")]:
        with pytest.raises(ValueError, match=what):
            allocate_act_bits(rep, **kw)
    for bad in (None, {}, {"units": {}}, renamed, 7):                              # a `bit_report` table has no 'elements'
        with pytest.raises(ValueError, match="allocate_act_bits: report must be an `act_bit_report` table"):
            allocate_act_bits(bad, budget_bits=100)
    with pytest.raises(ValueError, match="allocate_bits: "):
        allocate_act_bits({"units": {}, "elements": {}}, budget_bits=100)
