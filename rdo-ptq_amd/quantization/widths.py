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
