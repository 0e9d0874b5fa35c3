"""Widths per unit: which modules of a reconstruction unit carry a weight or an activation quantiser and whether they count as trained or
applied, the validation of a width plan (`QuantModel.set_weight_bits` / `set_act_bits`), and the allocators that choose one width per
unit from a `reports.bit_report` / `reports.act_bit_report` table under a size budget.  Pure host code."""
import math
from collections import OrderedDict
from collections.abc import Mapping
from numbers import Integral

from .quant_block import BaseQuantBlock
from .quant_layer import QuantModule
from .quantizer import MAX_BITS, AdaRoundQuantizer


def weighted_modules(unit):
    """the QuantModules of a unit that hold a weight (pixel shuffles do not), in module order"""
    return [m for m in unit.modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def is_trained(m):
    """has this QuantModule been calibrated?  Its AdaRoundQuantizer's alpha belongs to the delta it was trained on: no other width fits it"""
    return bool(m.trained) or isinstance(m.weight_quantizer, AdaRoundQuantizer)


def act_modules(unit):
    """(name inside the unit, module) of every QuantModule / BaseQuantBlock of a unit, the unit itself included ('' is its name): the
    holders of the unit's activation quantisers, in module order"""
    return [(mn, m) for mn, m in unit.named_modules() if isinstance(m, (QuantModule, BaseQuantBlock))]


def act_applied(m):
    """does a forward with act_quant=True apply this module's activation quantiser?"""
    return bool(m.trained) and not getattr(m, "disable_act_quant", False)


def width_plan(what, known, bits):
    """The `bits` argument of `QuantModel.set_weight_bits` / `set_act_bits` (named `what` in the messages) -> [(unit name, width)] in the
    order of `known` (`QuantModel.units()`): one whole number in 2 .. MAX_BITS for every unit, or a mapping unit name -> width for the
    units it names.  ValueError for anything else, an unknown name or a width out of range; nothing is written here."""
    def whole(b):
        return not isinstance(b, bool) and isinstance(b, Integral) and 2 <= b <= MAX_BITS
    if isinstance(bits, Mapping):
        unknown = [n for n in bits if n not in known]
        if unknown:
            raise ValueError(f"{what}: unknown unit name(s) {unknown}; QuantModel.units() has {list(known)}")
        plan = [(n, bits[n]) for n in known if n in bits]
    elif whole(bits):
        plan = [(n, bits) for n in known]
    else:
        raise ValueError(f"{what}: bits must be a whole number in 2 .. {MAX_BITS} or a mapping unit name -> width, got {bits!r}")
    for n, b in plan:
        if not whole(b):
            raise ValueError(f"{what}: the width of unit {n!r} must be a whole number in 2 .. {MAX_BITS}, got {b!r}")
    return plan


def format_plan(what, known, formats, names):
    """The `formats` argument of `QuantModel.set_weight_format` (named `what` in the messages) -> [(unit name, format name)] in the order
    of `known` (`QuantModel.units()`): one name out of `names` for every unit, or a mapping unit name -> name for the units it names.
    ValueError for anything else, an unknown unit or an unknown format (listing `names`); nothing is written here."""
    def named(f):
        return isinstance(f, str) and f in names
    if isinstance(formats, Mapping):
        unknown = [n for n in formats if n not in known]
        if unknown:
            raise ValueError(f"{what}: unknown unit name(s) {unknown}; QuantModel.units() has {list(known)}")
        plan = [(n, formats[n]) for n in known if n in formats]
    elif named(formats):
        plan = [(n, formats) for n in known]
    else:
        raise ValueError(f"{what}: formats must be one of {list(names)} or a mapping unit name -> format, got {formats!r}")
    for n, f in plan:
        if not named(f):
            raise ValueError(f"{what}: the format of unit {n!r} must be one of {list(names)}, got {f!r}")
    return plan


def _hull(options):
    """options: [(width, size, cost)] of one unit -> its hull points in ascending size: the lower convex hull from the smallest size up to
    the least-cost point (among equal costs the smallest).  Going down the list from the end, the cost per bit saved rises from step to
    step; points on a chord are kept."""
    pts = sorted(options, key=lambda p: p[1])
    best = min(range(len(pts)), key=lambda i: (pts[i][2], pts[i][1]))
    hull = []
    for p in pts[:best + 1]:
        # q = hull[-1] lies above the chord hull[-2] -> p when stepping p -> q costs more per bit than q -> hull[-2]
        while len(hull) >= 2 and (hull[-1][2] - p[2]) / (p[1] - hull[-1][1]) > (hull[-2][2] - hull[-1][2]) / (hull[-1][1] - hull[-2][1]):
            hull.pop()
        hull.append(p)
    return hull


def allocate_bits(report, budget_bits=None, avg_bits=None, fixed=None) -> dict:
    """Choose one weight width per unit from a `bit_report` table under a size budget.  Pure host code.
    `budget_bits`: a whole number of weight bits, or `avg_bits`: a real number of bits per weight, the budget then being
    floor(avg_bits * sum of report['weights']); exactly one of the two.  `fixed`: name -> width, a unit that has that one option.
    The rule.  Each unit's options are the points (size_bits, d_loss) of its row.  Kept is the lower convex hull of the options from the
    smallest size up to the unit's least-cost point (among equal costs the smallest); larger widths that cost more are dropped.  Every
    unit starts at its least-cost hull point.  While the total size exceeds the budget, the hull step with the smallest slope is taken,
    slope = cost added / size saved in float64, ties to the earlier unit in `units()` order; the first total <= budget stops it.
    ValueError, naming the smallest reachable size, when even that exceeds the budget.
    -> {'bits': OrderedDict name -> width, 'size_bits', 'avg_bits' (size_bits / sum of weights), 'cost' (sum of the chosen d_loss, added
    in unit order), 'budget_bits', 'steps': [(unit, from width, to width, slope)] in the order taken}.
    Guaranteed: no assignment of total size <= the returned size_bits has a lower total cost.  (Hull steps taken in slope order visit
    the minimisers of cost + s * size for the rising step slope s >= 0 -- the Lagrangian property; an assignment A' with size' <= size
    has cost' >= cost + s (size - size') >= cost.  Before the first step s = 0: every unit sits at its least cost.)
    Not guaranteed: that no assignment BETWEEN the returned size and the budget costs less (the rule does not search the gap), and
    anything about the calibrated model: the table is round-to-nearest and its costs are not additive (`rd_report`'s 'additivity'); on
    random-init models the costs are noise of either sign."""
    what = "allocate_bits"
    try:
        table, weights = report["units"], report["weights"]
        names = list(table)
        opts = OrderedDict((n, [(b, table[n][b]["size_bits"], float(table[n][b]["d_loss"])) for b in table[n]]) for n in names)
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f"{what}: report must be a `bit_report` table ('units': name -> width -> row with size_bits and d_loss; "
                         f"'weights'): {e!r}")
    if not names or any(not o for o in opts.values()):
        raise ValueError(f"{what}: the table holds no unit, or a unit without a width")
    if list(weights) != names or any(isinstance(w, bool) or not isinstance(w, int) or w < 1 for w in weights.values()):
        raise ValueError(f"{what}: report['weights'] must give a positive element count for every unit of the table, in its order")
    for n, o in opts.items():
        for b, size, cost in o:
            if isinstance(size, bool) or not isinstance(size, int) or size < 1 or not math.isfinite(cost):
                raise ValueError(f"{what}: unit {n!r} at width {b}: size_bits {size!r} must be a positive whole number and d_loss {cost!r} finite")
        if len({size for _, size, _ in o}) != len(o):
            raise ValueError(f"{what}: unit {n!r} has two widths of the same size")
    total_w = sum(weights.values())
    if (budget_bits is None) == (avg_bits is None):
        raise ValueError(f"{what}: exactly one of budget_bits and avg_bits must be given")
    if budget_bits is not None:
        if isinstance(budget_bits, bool) or not isinstance(budget_bits, int) or budget_bits < 1:
            raise ValueError(f"{what}: budget_bits must be a whole number >= 1, got {budget_bits!r}")
        budget = int(budget_bits)
    else:
        if isinstance(avg_bits, bool) or not isinstance(avg_bits, (int, float)) or not math.isfinite(avg_bits) or avg_bits <= 0:
            raise ValueError(f"{what}: avg_bits must be a positive finite number, got {avg_bits!r}")
        budget = math.floor(avg_bits * total_w)
    fixed = {} if fixed is None else fixed
    if not isinstance(fixed, dict):
        raise ValueError(f"{what}: fixed must be None or a dict name -> width, got {fixed!r}")
    for n, b in fixed.items():
        if n not in opts:
            raise ValueError(f"{what}: fixed names the unknown unit {n!r}; the table has {names}")
        if isinstance(b, bool) or b not in table[n]:
            raise ValueError(f"{what}: fixed gives unit {n!r} the width {b!r}; the table has {list(table[n])}")
    hulls = [_hull([p for p in opts[n] if n not in fixed or p[0] == fixed[n]]) for n in names]
    least = sum(h[0][1] for h in hulls)
    if least > budget:
        raise ValueError(f"{what}: the smallest reachable size is {least} bits; the budget is {budget}")
    at = [len(h) - 1 for h in hulls]
    size = sum(h[i][1] for h, i in zip(hulls, at))
    steps = []
    while size > budget:
        pick, slope = None, None
        for u, (h, i) in enumerate(zip(hulls, at)):
            if i == 0:
                continue
            s = (h[i - 1][2] - h[i][2]) / (h[i][1] - h[i - 1][1])
            if pick is None or s < slope:
                pick, slope = u, s
        h, i = hulls[pick], at[pick]
        steps.append((names[pick], h[i][0], h[i - 1][0], slope))
        size -= h[i][1] - h[i - 1][1]
        at[pick] = i - 1
    cost = 0.0
    for h, i in zip(hulls, at):
        cost += h[i][2]
    return {"bits": OrderedDict((n, h[i][0]) for n, h, i in zip(names, hulls, at)), "size_bits": size, "avg_bits": size / total_w,
            "cost": cost, "budget_bits": budget, "steps": steps}


def allocate_formats(format_report, bit_report=None, budget_bits=None, avg_bits=None, fixed=None) -> dict:
    """Choose one weight format per unit from a `format_report` table -- with a `bit_report`, one MX format or one integer width --
    under a size budget: `allocate_bits`'s rule, guarantee and result on options keyed by name.  Pure host code.
    Options.  A unit's options are the formats of its `format_report` row under their names and, with a `bit_report`, its widths under
    "int<b>".  Sizes are the tables' own `size_bits`, and they are not of one kind: an integer width counts n_bits x elements, the
    per-channel delta and zero point of the grid not included; an MX format counts element bits x elements + 8 x blocks, its scale
    bytes included (4.25 / 6.25 / 8.25 bits a weight on rows that are whole blocks).  Costs are the rows' `d_loss`.
    The two reports must be tables of one measurement: the same unit names in the same order, the same 'weights', 'n', 'pixels' and
    'lmbda', and the same 'loss' of the 'fp' row; otherwise ValueError saying what differs.
    Equal sizes.  `allocate_bits` refuses two options of one size (mxfp6_e2m3 and mxfp6_e3m2, mxfp8_e4m3 and mxfp8_e5m2).  Among the
    options of a unit with equal size_bits only the one with the least d_loss is kept, ties to the earlier one (formats in the order
    of the row, then widths); the others can be in no cheapest assignment of any size and are listed under 'dominated'.
    `budget_bits` / `avg_bits`: as in `allocate_bits`.  `fixed`: name -> option key, a unit that has that one option (no other option
    of the unit is looked at, none is listed as dominated).
    -> `allocate_bits`'s keys with 'choice' (OrderedDict name -> option key) in place of 'bits' -- 'steps' name option keys --, and
    'formats': OrderedDict name -> format name, or 'int' (what `QuantModel.set_weight_format` takes), 'bits': OrderedDict name -> width
    for the units on 'int' (what `QuantModel.set_weight_bits` takes), 'dominated': OrderedDict name -> [option keys] (units that
    have any).  With a `format_report` of distinct sizes alone, 'choice' and every shared key are `allocate_bits` of that table."""
    from hipops._lib import MX_FORMATS
    what = "allocate_formats"
    try:
        names = list(format_report["units"])
        table = OrderedDict((n, OrderedDict((f, format_report["units"][n][f]) for f in format_report["units"][n])) for n in names)
        weights = format_report["weights"]
        for n in names:
            for f, row in table[n].items():
                row["size_bits"], row["d_loss"]
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f"{what}: format_report must be a `format_report` table ('units': name -> format -> row with size_bits and "
                         f"d_loss; 'weights'): {e!r}")
    unknown = [f for n in names for f in table[n] if f not in MX_FORMATS]
    if unknown:
        raise ValueError(f"{what}: format_report holds the unknown format(s) {sorted(set(map(str, unknown)))}; the formats are {list(MX_FORMATS)}")
    width_of = {}
    if bit_report is not None:
        try:
            theirs = list(bit_report["units"])
            if theirs != names:
                raise ValueError(f"{what}: the reports differ in their units: format_report has {names}, bit_report has {theirs}")
            if dict(bit_report["weights"]) != dict(weights) or list(bit_report["weights"]) != list(weights):
                raise ValueError(f"{what}: the reports differ in 'weights': {dict(weights)} and {dict(bit_report['weights'])}")
            for key in ("n", "pixels", "lmbda"):
                if bit_report[key] != format_report[key]:
                    raise ValueError(f"{what}: the reports differ in {key!r}: format_report has {format_report[key]!r}, bit_report has "
                                     f"{bit_report[key]!r}")
            if bit_report["fp"]["loss"] != format_report["fp"]["loss"]:
                raise ValueError(f"{what}: the reports differ in the loss of their 'fp' rows: {format_report['fp']['loss']!r} and "
                                 f"{bit_report['fp']['loss']!r}: they were not measured on the same model and images")
            for n in names:
                for b, row in bit_report["units"][n].items():
                    if isinstance(b, bool) or not isinstance(b, Integral):
                        raise ValueError(f"{what}: bit_report gives unit {n!r} the width {b!r}, which is no whole number")
                    row["size_bits"], row["d_loss"]
                    table[n][f"int{int(b)}"] = row
                    width_of[f"int{int(b)}"] = int(b)
        except (KeyError, TypeError, IndexError) as e:
            raise ValueError(f"{what}: bit_report must be a `bit_report` table of the same measurement ('units', 'weights', 'fp', 'n', "
                             f"'pixels', 'lmbda'): {e!r}")
    fixed = {} if fixed is None else fixed
    if not isinstance(fixed, dict):
        raise ValueError(f"{what}: fixed must be None or a dict name -> option, got {fixed!r}")
    for n, k in fixed.items():
        if n not in table:
            raise ValueError(f"{what}: fixed names the unknown unit {n!r}; the table has {names}")
        if not isinstance(k, str) or k not in table[n]:
            raise ValueError(f"{what}: fixed gives unit {n!r} the option {k!r}; the table has {list(table[n])}")
    kept, dominated = OrderedDict(), OrderedDict()
    for n in names:
        rows = OrderedDict((k, r) for k, r in table[n].items() if n not in fixed or k == fixed[n])
        best = {}                                                                # size -> the key kept at that size
        for k, r in rows.items():
            size, cost = r["size_bits"], r["d_loss"]
            if isinstance(size, bool) or not isinstance(size, int) or size < 1 or isinstance(cost, bool) or \
                    not isinstance(cost, (int, float)) or not math.isfinite(cost):
                raise ValueError(f"{what}: unit {n!r} at option {k!r}: size_bits {size!r} must be a positive whole number and d_loss {cost!r} finite")
            if size not in best or float(cost) < float(rows[best[size]]["d_loss"]):
                best[size] = k
        kept[n] = OrderedDict((k, {"size_bits": r["size_bits"], "d_loss": r["d_loss"]}) for k, r in rows.items() if best[r["size_bits"]] == k)
        if len(kept[n]) != len(rows):
            dominated[n] = [k for k in rows if k not in kept[n]]
    try:
        out = allocate_bits({"units": kept, "weights": weights}, budget_bits=budget_bits, avg_bits=avg_bits)
    except ValueError as e:
        raise ValueError(str(e).replace("allocate_bits:", f"{what}:", 1).replace("at width", "at option").replace("`bit_report`", "`format_report`"))
    choice = out.pop("bits")
    out["choice"] = choice
    out["formats"] = OrderedDict((n, "int" if k in width_of else k) for n, k in choice.items())
    out["bits"] = OrderedDict((n, width_of[k]) for n, k in choice.items() if k in width_of)
    out["dominated"] = dominated
    return out


def allocate_act_bits(report, budget_bits=None, avg_bits=None, fixed=None) -> dict:
    """Choose one activation width per unit from an `act_bit_report` table under a size budget: `allocate_bits` on the table with the
    units' elements (activation values per image) in the place of the weight counts -- its rule, its guarantees and its result, with
    sizes in activation bits per image and `avg_bits` in bits per quantised activation value.  What it returns under 'bits' is what
    `QuantModel.set_act_bits` takes."""
    try:
        table = {"units": report["units"], "weights": report["elements"]}
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError(f"allocate_act_bits: report must be an `act_bit_report` table ('units', 'elements'): {e!r}")
    return allocate_bits(table, budget_bits=budget_bits, avg_bits=avg_bits, fixed=fixed)
