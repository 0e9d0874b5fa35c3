"""CPU checks of `widths.allocate_formats` (re-exported as `export.allocate_formats`): the allocator over MX formats and integer widths.
Hand-made tables of 3 units x 4-6 options, some of equal size, some dominated, with and without a `bit_report`: a brute force over all
assignments confirms the guarantee (no assignment of size <= the returned size costs less); the equal-size rule and 'dominated';
`fixed`; both budget forms; every ValueError, mismatching reports included; and on a `format_report` of distinct sizes the result is
`allocate_bits` of the same table.  No GPU, no library call."""
import copy
import itertools
from collections import OrderedDict

import pytest

from quantization.export import allocate_bits, allocate_formats
from quantization.widths import allocate_formats as from_widths

FORMATS = ("mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8_e4m3", "mxfp8_e5m2")
BITS = {"mxfp4": 4, "mxfp6_e2m3": 6, "mxfp6_e3m2": 6, "mxfp8_e4m3": 8, "mxfp8_e5m2": 8}
# unit -> (elements, blocks): the second unit has ragged rows (more scale bytes a weight)
UNITS = OrderedDict([("a", (4096, 128)), ("b.0", (675, 27)), ("c", (1000, 40))])


def mx_size(unit, fmt):
    n, blocks = UNITS[unit]
    return BITS[fmt] * n + 8 * blocks


def format_table(costs, formats=FORMATS):
    """costs: unit -> format -> d_loss"""
    rep = OrderedDict(fp={"loss": 1.25}, units=OrderedDict(), weights=OrderedDict((u, UNITS[u][0]) for u in UNITS))
    for u in UNITS:
        rep["units"][u] = OrderedDict((f, {"size_bits": mx_size(u, f), "d_loss": costs[u][f], "loss": 1.25 + costs[u][f]}) for f in formats)
    rep["formats"], rep["n"], rep["pixels"], rep["lmbda"], rep["batch"] = list(formats), 4, 4 * 64 * 64, 0.01, 2
    return rep


def bit_table(costs, widths):
    """costs: unit -> width -> d_loss"""
    rep = OrderedDict(fp={"loss": 1.25}, units=OrderedDict(), weights=OrderedDict((u, UNITS[u][0]) for u in UNITS))
    for u in UNITS:
        rep["units"][u] = OrderedDict((b, {"size_bits": b * UNITS[u][0], "d_loss": costs[u][b]}) for b in widths)
    rep["widths"], rep["n"], rep["pixels"], rep["lmbda"], rep["batch"] = list(widths), 4, 4 * 64 * 64, 0.01, 8
    return rep


# the e3m2 twin is the better 6-bit format on 'a' and the worse one on 'b.0'; on 'c' the two 8-bit formats tie (the earlier stays)
F_COSTS = {"a": {"mxfp4": 0.9, "mxfp6_e2m3": 0.31, "mxfp6_e3m2": 0.27, "mxfp8_e4m3": 0.02, "mxfp8_e5m2": 0.11},
           "b.0": {"mxfp4": 0.2, "mxfp6_e2m3": 0.05, "mxfp6_e3m2": 0.09, "mxfp8_e4m3": 0.06, "mxfp8_e5m2": 0.07},
           "c": {"mxfp4": 1.5, "mxfp6_e2m3": 0.4, "mxfp6_e3m2": 0.6, "mxfp8_e4m3": -0.01, "mxfp8_e5m2": -0.01}}
B_COSTS = {"a": {4: 1.4, 6: 0.29, 8: 0.015}, "b.0": {4: 0.5, 6: 0.045, 8: 0.001}, "c": {4: 2.0, 6: 0.7, 8: 0.05}}


def options(frep, brep=None):
    """unit -> [(key, size, cost)]: every option of the two tables, nothing filtered"""
    out = OrderedDict()
    for u in frep["units"]:
        out[u] = [(f, r["size_bits"], r["d_loss"]) for f, r in frep["units"][u].items()]
        if brep is not None:
            out[u] += [(f"int{b}", r["size_bits"], r["d_loss"]) for b, r in brep["units"][u].items()]
    return out


def brute_force_ok(opts, got, fixed=None):
    """no assignment of total size <= got['size_bits'] has a lower total cost than got['cost']; and got is one of the assignments"""
    fixed = fixed or {}
    lists = [[o for o in opts[u] if u not in fixed or o[0] == fixed[u]] for u in opts]
    seen = False
    for pick in itertools.product(*lists):
        size, cost = sum(p[1] for p in pick), 0.0
        for p in pick:
            cost += p[2]
        if [p[0] for p in pick] == list(got["choice"].values()):
            seen = True
            assert size == got["size_bits"] and cost == got["cost"]
        if size <= got["size_bits"]:
            assert cost >= got["cost"], (pick, got["choice"])
    assert seen


def budgets(opts):
    least = sum(min(o[1] for o in opts[u]) for u in opts)
    most = sum(max(o[1] for o in opts[u]) for u in opts)
    return [least, least + 1, (2 * least + most) // 3, (least + most) // 2, (least + 2 * most) // 3, most - 1, most, most + 1000]


def test_it_is_exported_next_to_allocate_bits():
    assert allocate_formats is from_widths


@pytest.mark.parametrize("with_bits", [False, True])
def test_no_cheaper_assignment_of_at_most_the_returned_size(with_bits):
    frep = format_table(F_COSTS)
    brep = bit_table(B_COSTS, (4, 6, 8)) if with_bits else None
    opts = options(frep, brep)
    assert all(4 <= len(o) <= 8 for o in opts.values()) and len(opts) == 3
    sizes_seen = set()
    for budget in budgets(opts):
        got = allocate_formats(frep, brep, budget_bits=budget)
        assert got["size_bits"] <= budget == got["budget_bits"]
        assert got["size_bits"] == sum(dict((k, s) for k, s, _ in opts[u])[got["choice"][u]] for u in opts)
        assert got["avg_bits"] == got["size_bits"] / sum(frep["weights"].values())
        brute_force_ok(opts, got)
        sizes_seen.add(got["size_bits"])
    assert len(sizes_seen) >= 4                                                     # the budgets reached different assignments
    # 3 units x 4 options: a narrower table, the same check
    narrow = format_table(F_COSTS, FORMATS[:4])
    nb = bit_table(B_COSTS, (8,)) if with_bits else None
    for budget in budgets(options(narrow, nb)):
        brute_force_ok(options(narrow, nb), allocate_formats(narrow, nb, budget_bits=budget))


def test_equal_sizes_keep_the_least_cost_and_list_the_rest():
    frep = format_table(F_COSTS)
    big = 10 ** 9
    got = allocate_formats(frep, budget_bits=big)
    assert got["dominated"] == OrderedDict([("a", ["mxfp6_e2m3", "mxfp8_e5m2"]), ("b.0", ["mxfp6_e3m2", "mxfp8_e5m2"]),
                                            ("c", ["mxfp6_e3m2", "mxfp8_e5m2"])])     # 'c': a tie at 8 bits goes to the earlier one
    assert got["choice"] == OrderedDict([("a", "mxfp8_e4m3"), ("b.0", "mxfp6_e2m3"), ("c", "mxfp8_e4m3")]) and got["steps"] == []
    assert got["formats"] == got["choice"] and got["bits"] == OrderedDict()
    for budget in budgets(options(frep)):
        r = allocate_formats(frep, budget_bits=budget)
        assert not any(r["choice"][u] in r["dominated"].get(u, []) for u in UNITS)
    # an integer width of the size of an MX format cannot happen on these units (the scales add bits), but equal sizes across the two
    # tables obey the same rule: make one
    brep = bit_table(B_COSTS, (4, 6, 8))
    brep["units"]["a"][6]["size_bits"] = mx_size("a", "mxfp6_e3m2")
    brep["units"]["a"][6]["d_loss"] = 0.27                                          # ties with mxfp6_e3m2, which comes earlier
    r = allocate_formats(frep, brep, budget_bits=big)
    assert r["dominated"]["a"] == ["mxfp6_e2m3", "mxfp8_e5m2", "int6"]
    brep["units"]["a"][6]["d_loss"] = 0.26
    r = allocate_formats(frep, brep, budget_bits=big)
    assert r["dominated"]["a"] == ["mxfp6_e2m3", "mxfp6_e3m2", "mxfp8_e5m2"]


def test_formats_and_bits_are_what_the_setters_take():
    frep, brep = format_table(F_COSTS), bit_table(B_COSTS, (4, 6, 8))
    seen = set()
    for budget in budgets(options(frep, brep)):
        r = allocate_formats(frep, brep, budget_bits=budget)
        assert list(r["choice"]) == list(r["formats"]) == list(UNITS)
        for u, k in r["choice"].items():
            if k.startswith("int"):
                assert r["formats"][u] == "int" and r["bits"][u] == int(k[3:]) and isinstance(r["bits"][u], int)
            else:
                assert r["formats"][u] == k and k in FORMATS and u not in r["bits"]
            seen.add(r["formats"][u])
        keys = {u: {o[0] for o in o_list} for u, o_list in options(frep, brep).items()}
        assert all(s[1] in keys[s[0]] and s[2] in keys[s[0]] for s in r["steps"])  # the steps name option keys
    assert "int" in seen and len(seen) >= 3                                         # MX formats and integer widths were both chosen


def test_fixed():
    frep, brep = format_table(F_COSTS), bit_table(B_COSTS, (4, 6, 8))
    opts = options(frep, brep)
    for fixed in ({"a": "mxfp4"}, {"b.0": "mxfp6_e3m2", "c": "int6"}, {"a": "int8", "b.0": "mxfp8_e5m2", "c": "mxfp4"}):
        least = sum(min(o[1] for o in opts[u] if u not in fixed or o[0] == fixed[u]) for u in opts)
        for budget in (least, least + 3000, 10 ** 9):
            r = allocate_formats(frep, brep, budget_bits=budget, fixed=fixed)
            assert all(r["choice"][u] == k for u, k in fixed.items())
            assert not any(u in r["dominated"] for u in fixed)                      # a fixed unit has one option: nothing to dominate
            brute_force_ok(opts, r, fixed)
    r = allocate_formats(frep, brep, budget_bits=10 ** 9, fixed={"b.0": "mxfp6_e3m2", "c": "int6"})   # a dominated option can be fixed
    assert r["formats"] == OrderedDict([("a", "int"), ("b.0", "mxfp6_e3m2"), ("c", "int")])   # 'a' is free: int8 is its least cost
    assert r["bits"] == OrderedDict([("a", 8), ("c", 6)])


def test_both_budget_forms():
    frep, brep = format_table(F_COSTS), bit_table(B_COSTS, (4, 6, 8))
    total = sum(frep["weights"].values())
    for avg in (4.3, 5.0, 6.25, 7.999, 9):
        a = allocate_formats(frep, brep, avg_bits=avg)
        b = allocate_formats(frep, brep, budget_bits=int(avg * total // 1))
        assert a == b and a["budget_bits"] == int(avg * total // 1)
    with pytest.raises(ValueError, match="allocate_formats: the smallest reachable size is 23084 bits; the budget is 23083"):
        allocate_formats(frep, brep, budget_bits=23083)                             # 4 x 5771 weights, int4 everywhere
    assert allocate_formats(frep, brep, budget_bits=23084)["formats"] == OrderedDict((u, "int") for u in UNITS)
    assert allocate_formats(frep, budget_bits=4 * total + 8 * 195)["formats"] == OrderedDict((u, "mxfp4") for u in UNITS)


def test_distinct_sizes_alone_give_allocate_bits_of_the_table():
    frep = format_table(F_COSTS, ("mxfp4", "mxfp6_e3m2", "mxfp8_e4m3"))
    for budget in budgets(options(frep)):
        mine, theirs = allocate_formats(frep, budget_bits=budget), allocate_bits(frep, budget_bits=budget)
        assert mine["dominated"] == OrderedDict() and mine["bits"] == OrderedDict() and mine["formats"] == mine["choice"] == theirs["bits"]
        assert {k: mine[k] for k in theirs if k != "bits"} == {k: theirs[k] for k in theirs if k != "bits"}
        assert set(mine) == (set(theirs) - {"bits"}) | {"choice", "formats", "bits", "dominated"}
    f = {"a": "mxfp6_e3m2"}
    assert allocate_formats(frep, avg_bits=7.0, fixed=f)["choice"] == allocate_bits(frep, avg_bits=7.0, fixed=f)["bits"]


def test_every_refusal():
    frep, brep = format_table(F_COSTS), bit_table(B_COSTS, (4, 6, 8))
    kw = dict(budget_bits=10 ** 6)

    def broken(rep, edit):
        rep = copy.deepcopy(rep)
        edit(rep)
        return rep

    def drop(key):
        return lambda r: r.pop(key)
    cases = [
        ((None, None), kw, "format_report must be a `format_report` table"),
        ((broken(frep, drop("weights")), None), kw, "format_report must be a `format_report` table"),
        ((broken(frep, lambda r: r["units"]["a"]["mxfp4"].pop("d_loss")), None), kw, "format_report must be a `format_report` table"),
        ((broken(frep, lambda r: r["units"]["a"].__setitem__("mxfp5", r["units"]["a"]["mxfp4"])), None), kw, "unknown format\\(s\\) \\['mxfp5'\\]"),
        ((broken(frep, lambda r: r["units"]["c"]["mxfp4"].__setitem__("d_loss", float("nan"))), None), kw,
         "unit 'c' at option 'mxfp4': size_bits .* d_loss nan finite"),
        ((broken(frep, lambda r: r["units"]["c"]["mxfp4"].__setitem__("size_bits", 0)), None), kw, "unit 'c' at option 'mxfp4': size_bits 0"),
        ((broken(frep, lambda r: r["units"].__setitem__("a", OrderedDict())), None), kw, "holds no unit, or a unit without a width"),
        ((broken(frep, lambda r: r["weights"].__setitem__("a", 0)), None), kw, "report\\['weights'\\] must give a positive element count"),
        ((frep, brep), {}, "exactly one of budget_bits and avg_bits"),
        ((frep, brep), dict(budget_bits=5, avg_bits=5.0), "exactly one of budget_bits and avg_bits"),
        ((frep, brep), dict(budget_bits=0), "budget_bits must be a whole number >= 1"),
        ((frep, brep), dict(budget_bits=True), "budget_bits must be a whole number >= 1"),
        ((frep, brep), dict(avg_bits=float("inf")), "avg_bits must be a positive finite number"),
        ((frep, brep), dict(avg_bits=2.0), "the smallest reachable size is 23084 bits; the budget is 11542"),
        ((frep, brep), dict(kw, fixed=["a"]), "fixed must be None or a dict name -> option"),
        ((frep, brep), dict(kw, fixed={"z": "mxfp4"}), "fixed names the unknown unit 'z'"),
        ((frep, brep), dict(kw, fixed={"a": "int5"}), "fixed gives unit 'a' the option 'int5'; the table has \\['mxfp4', .*'int8'\\]"),
        ((frep, brep), dict(kw, fixed={"a": 8}), "fixed gives unit 'a' the option 8"),
        ((frep, None), dict(kw, fixed={"a": "int8"}), "fixed gives unit 'a' the option 'int8'"),
        # reports that are not of one measurement
        ((frep, {"units": {}}), kw, "the reports differ in their units"),
        ((frep, broken(brep, lambda r: r["units"].move_to_end("a"))), kw, "the reports differ in their units: .*\\['b.0', 'c', 'a'\\]"),
        ((frep, broken(brep, lambda r: r["weights"].__setitem__("c", 1001))), kw, "the reports differ in 'weights'"),
        ((frep, broken(brep, lambda r: r.__setitem__("n", 8))), kw, "the reports differ in 'n': format_report has 4, bit_report has 8"),
        ((frep, broken(brep, lambda r: r.__setitem__("pixels", 1))), kw, "the reports differ in 'pixels'"),
        ((frep, broken(brep, lambda r: r.__setitem__("lmbda", 0.02))), kw, "the reports differ in 'lmbda'"),
        ((frep, broken(brep, lambda r: r["fp"].__setitem__("loss", 1.26))), kw, "the reports differ in the loss of their 'fp' rows: 1.25 and 1.26"),
        ((frep, broken(brep, drop("fp"))), kw, "bit_report must be a `bit_report` table of the same measurement"),
        ((frep, broken(brep, lambda r: r["units"]["a"].__setitem__("8", r["units"]["a"][8]))), kw, "the width '8', which is no whole number"),
        ((frep, broken(brep, lambda r: r["units"]["b.0"][4].pop("size_bits"))), kw, "bit_report must be a `bit_report` table"),
    ]
    for (f, b), kwargs, why in cases:
        with pytest.raises(ValueError, match=f"allocate_formats: .*{why}"):
            allocate_formats(f, b, **kwargs)
    # the batch size is no part of the measurement: the two tables above differ in it and go together
    assert frep["batch"] != brep["batch"] and allocate_formats(frep, brep, **kw)["cost"] < 0.1
    # nothing was written into the reports
    assert frep == format_table(F_COSTS) and brep == bit_table(B_COSTS, (4, 6, 8))
