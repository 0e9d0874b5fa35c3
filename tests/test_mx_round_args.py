"""CPU checks of learned rounding on the MX grids: include/rdo_ptq_mxround.h against `EXPORTS_MXROUND` and the built library, the
refusals of the C entries (RDO_EINVAL without touching a device) and of the `ops.mx_*` wrappers, the float64 reference's own properties
(tests/mx_round_reference.py) for all five formats, `MXAdaRoundQuantizer`'s fields, `QuantModel.set_weight_format(..., rounding=...)`
and the refusals of `reconstruct`, on the toy models built on the CPU (fields only: no kernel runs)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import mx_reference as R
import mx_round_reference as RR
from test_rd_report_args import _toy

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rdo_mx_neighbours", "rdo_mx_round_init_alpha", "rdo_mx_round_fwd", "rdo_mx_round_step"}


# ----------------------------------------------------------------------------- the header, the exports
def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxround.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXROUND) == NAMES
    assert '#include "rdo_ptq_mx.h"' in hdr
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_BIAS, L.EXPORTS_BITS, L.EXPORTS_PACK, L.EXPORTS_SUBPEL, L.EXPORTS_ACTBITS, L.EXPORTS_ATTNQ,
              L.EXPORTS_MX)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert len(L.EXPORTS) == 124 and len(L.EXPORTS_MX) == 4
    mxh = open(os.path.join(ROOT, "include", "rdo_ptq_mx.h")).read()
    assert set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", mxh, re.M)) == set(L.EXPORTS_MX)


def _desc(numel=120, rows=3, kh=0, kw=0, cin=0):
    from hipops import _lib as L
    return L.AdaDesc(numel, rows, 256, 0, 0.0, 0.0, kh, kw, cin)


def test_c_entries_refuse_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    odd = C.c_void_p(C.addressof(buf) + 2)

    def refused(fn, names, base, bad, who):
        for kw in bad:
            a = dict(base, **kw)
            assert fn(*[a[n] for n in names], None) == RDO_EINVAL, (who, kw)
            assert who.encode() in h.rdo_last_error(), (who, kw)

    refused(h.rdo_mx_neighbours, ["w", "rows", "inner", "format", "lo", "gap", "scales"],
            dict(w=p, rows=3, inner=40, format=0, lo=p, gap=p, scales=p),
            [dict(w=None), dict(lo=None), dict(gap=None), dict(rows=0), dict(rows=-3), dict(inner=0), dict(inner=-40), dict(format=-1), dict(format=5),
             dict(w=odd), dict(lo=odd), dict(gap=odd), dict(rows=2 ** 31 - 1, inner=2 ** 40)], "rdo_mx_neighbours")
    refused(h.rdo_mx_round_init_alpha, ["w", "lo", "gap", "numel", "alpha"], dict(w=p, lo=p, gap=p, numel=120, alpha=p),
            [dict(w=None), dict(lo=None), dict(gap=None), dict(alpha=None), dict(numel=0), dict(numel=-4), dict(w=odd), dict(lo=odd), dict(gap=odd),
             dict(alpha=odd)], "rdo_mx_round_init_alpha")
    d = C.byref(_desc())
    refused(h.rdo_mx_round_fwd, ["d", "lo", "gap", "alpha", "soft", "wq", "wd", "codes", "scales", "format"],
            dict(d=d, lo=p, gap=p, alpha=p, soft=0, wq=p, wd=None, codes=None, scales=None, format=0),
            [dict(d=None), dict(lo=None), dict(gap=None), dict(alpha=None), dict(wq=None), dict(format=-1), dict(format=5), dict(lo=odd), dict(gap=odd),
             dict(alpha=odd), dict(wq=odd), dict(wd=odd), dict(codes=p, scales=p, soft=1), dict(codes=p, scales=None),
             dict(d=C.byref(_desc(numel=0))), dict(d=C.byref(_desc(numel=-8))), dict(d=C.byref(_desc(rows=0))), dict(d=C.byref(_desc(numel=121))),
             dict(d=C.byref(_desc(kh=3, kw=3, cin=5)))], "rdo_mx_round_fwd")
    refused(h.rdo_mx_round_step, ["d", "lo", "gap", "slabs", "nsplit", "gs", "rw", "sched", "it", "alpha", "m", "v", "wq", "wd", "log"],
            dict(d=d, lo=p, gap=p, slabs=p, nsplit=2, gs=1.0, rw=0.01, sched=p, it=p, alpha=p, m=p, v=p, wq=p, wd=None, log=None),
            [dict(d=None), dict(lo=None), dict(gap=None), dict(slabs=None), dict(sched=None), dict(it=None), dict(alpha=None), dict(m=None),
             dict(v=None), dict(wq=None), dict(nsplit=0), dict(nsplit=-1), dict(lo=odd), dict(gap=odd), dict(slabs=odd), dict(alpha=odd), dict(m=odd),
             dict(v=odd), dict(wq=odd), dict(wd=odd), dict(log=odd), dict(d=C.byref(_desc(numel=0))), dict(d=C.byref(_desc(rows=-1))),
             dict(d=C.byref(_desc(numel=121))), dict(d=C.byref(_desc(kh=1, kw=1, cin=7)))], "rdo_mx_round_step")


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


def test_wrappers_refuse_malformed_operands(no_library):
    ops = no_library
    w = torch.zeros(3, 40)
    sched, it, log = torch.zeros(5, 4), torch.zeros(1, dtype=torch.int32), torch.zeros(5, 32)
    d = _desc()
    cases = [
        (ops.mx_neighbours, (w.double(), "mxfp4"), {}, "mx_neighbours: w_rows must be an fp32 tensor"),
        (ops.mx_neighbours, (torch.zeros(120), "mxfp4"), {}, "mx_neighbours: .*rank 2"),
        (ops.mx_neighbours, (torch.zeros(3, 80)[:, ::2], "mxfp4"), {}, "mx_neighbours: .*contiguous"),
        (ops.mx_neighbours, (w, "mxfp5"), {}, "mx_neighbours: unknown MX format 'mxfp5'; the formats are"),
        (ops.mx_neighbours, (w, "mxfp4"), {}, "mx_neighbours: .*no CPU path"),
        (ops.mx_round_init_alpha, (w, w, torch.zeros(3, 41)), {}, "mx_round_init_alpha: gap holds 123 elements, expected 120"),
        (ops.mx_round_init_alpha, (w, w.double(), w), {}, "mx_round_init_alpha: lo must be an fp32 tensor"),
        (ops.mx_round_init_alpha, (None, w, w), {}, "mx_round_init_alpha: w must be an fp32 tensor"),
        (ops.mx_round_init_alpha, (w, w, w), {"alpha": torch.zeros(3, 40, device="meta")}, "mx_round_init_alpha: alpha is on meta, w on cpu"),
        (ops.mx_round_init_alpha, (w, w, w), {}, "mx_round_init_alpha: .*no CPU path"),
        (ops.mx_round_fwd, (d, w, w, w, True, "fp4"), {}, "mx_round_fwd: unknown MX format 'fp4'"),
        (ops.mx_round_fwd, (d, w, w, torch.zeros(3, 39), True, "mxfp4"), {}, "mx_round_fwd: alpha holds 117 elements, expected 120"),
        (ops.mx_round_fwd, (_desc(numel=80), w, w, w, True, "mxfp4"), {"wq": torch.zeros(3, 40, device="meta")}, "mx_round_fwd: wq is on meta"),
        (ops.mx_round_fwd, (_desc(numel=80, rows=2), torch.zeros(3, 40, device="meta"), torch.zeros(3, 40, device="meta"),
                            torch.zeros(3, 40, device="meta"), True, "mxfp4"), {}, "mx_round_fwd: .*no CPU path"),
        (ops.mx_round_step, (d, w, w, torch.zeros(2, 3, 40), 1.0, 0.01, sched, it, w, w, torch.zeros(3, 40).double(), w, None, log), {},
         "mx_round_step: v must be an fp32 tensor"),
        (ops.mx_round_step, (d, w, w, torch.zeros(2, 3, 40), 1.0, 0.01, sched, it, w, w, w, w, None, log), {}, "mx_round_step: .*no CPU path"),
    ]
    for fn, args, kw, what in cases:
        with pytest.raises(ValueError, match=what):
            fn(*args, **kw)


def test_wrappers_refuse_what_lies_behind_the_device_check(monkeypatch, no_library):
    """the checks behind `no CPU path`, on meta tensors with the device check switched off"""
    ops = no_library
    monkeypatch.setattr(ops, "_mx_cuda", lambda *a: None)
    t = lambda *s, **k: torch.zeros(*s, device="meta", **k)
    w = t(3, 40)
    sched, it, log = t(5, 4), t(1, dtype=torch.int32), t(5, 32)
    good = lambda **k: dict(dict(d=_desc(), lo=w, gap=w, slabs=t(2, 3, 40), grad_scale=1.0, round_weight=0.01, sched=sched, iter_ptr=it, alpha=w, m=w,
                                 v=w, wq=w, wd=None, round_log=log), **k)
    cases = [
        (ops.mx_round_step, good(d=_desc(numel=80)), "d must be an `ada_desc` of the 120 elements of lo"),
        (ops.mx_round_step, good(d=None), "d must be an `ada_desc`"),
        (ops.mx_round_step, good(slabs=t(2, 3, 41)), "slabs must be \\[nsplit, ...\\] with 120 elements a slab"),
        (ops.mx_round_step, good(slabs=t(0, 3, 40)), "slabs is empty"),
        (ops.mx_round_step, good(sched=t(5, 3)), "sched must be \\[iters, 4\\]"),
        (ops.mx_round_step, good(iter_ptr=t(2, dtype=torch.int32)), "iter_ptr holds 2 elements, expected 1"),
        (ops.mx_round_step, good(iter_ptr=t(1)), "iter_ptr must be an int32 tensor"),
        (ops.mx_round_step, good(round_log=t(4, 32)), "round_log must be a contiguous fp32 \\[5, 32\\]"),
        (ops.mx_round_step, good(wd=t(3, 41)), "wd must be 120 contiguous fp32 elements"),
        (ops.mx_round_fwd, dict(d=_desc(), lo=w, gap=w, alpha=w, soft=True, fmt="mxfp4", codes=True, scales=t(3, 2, dtype=torch.uint8)),
         "codes describe the hard weight"),
        (ops.mx_round_fwd, dict(d=_desc(), lo=w, gap=w, alpha=w, soft=False, fmt="mxfp4", codes=True, scales=t(3, 1, dtype=torch.uint8)),
         "scales must be a contiguous uint8 \\[3, 2\\]"),
        (ops.mx_round_fwd, dict(d=_desc(), lo=w, gap=w, alpha=w, soft=False, fmt="mxfp4", codes=True), "scales must be a contiguous uint8"),
    ]
    for fn, kw, what in cases:
        with pytest.raises(ValueError, match=f"{fn.__name__}: .*{what}"):
            fn(**kw)


# ----------------------------------------------------------------------------- the reference
def _weights(fmt):
    """[24, 180] with per-row scales over two decades and a run of zeros, then planted: elements on the grid, exact ties, +-max X, -0,
    a tiny negative"""
    g = torch.Generator().manual_seed(29)
    w = torch.randn(24, 180, generator=g) * torch.pow(10.0, torch.linspace(-2, 0, 24))[:, None]
    w[0, :40] = 0.0
    q = R.quantize(w, fmt)
    nb = RR.neighbours(w, fmt)
    w[3, :20] = q["wq"][3, :20]
    live = nb["gap"][4] > 0
    tie = nb["lo"][4] + 0.5 * nb["gap"][4]                                 # exact: half a grid step is representable
    w[4, :60] = torch.where(live[:60], tie[:60], w[4, :60])
    X = float(torch.ldexp(torch.ones(()), q["scales"][5, 0].int() - 127))
    vmax = R.FORMATS[fmt][5]
    w[5, 1], w[5, 2], w[5, 3], w[5, 4] = vmax * X, -vmax * X, -0.0, -1e-30
    return w


@pytest.mark.parametrize("fmt", R.NAMES)
def test_reference_neighbours_bracket_the_weight_on_an_exact_grid(fmt):
    w = _weights(fmt)
    nb = RR.neighbours(w, fmt)                                             # (asserts inside that lo and gap are exact in float32)
    lo, gap, pinned = nb["lo"], nb["gap"], nb["pinned"]
    q = R.quantize(w, fmt)
    assert torch.equal(nb["scales"], q["scales"])
    live = gap > 0
    assert torch.equal(live, ~pinned)
    l, gp, wl = lo[live], gap[live], w[live]
    assert bool(((l.double() <= wl.double()) & (wl.double() < l.double() + gp.double())).all())
    assert torch.equal(torch.floor(wl / gp) * gp, l) and float((l / gp).abs().max()) <= 16          # fp32
    hi = (l.double() + gp.double()).float()
    assert torch.equal(hi.double(), l.double() + gp.double())
    # both neighbours are on the grid: round to nearest leaves them where they are (the block scale may only grow with them)
    both = torch.where(live, lo + gap, lo)
    assert torch.equal(R.quantize(lo, fmt)["wq"], lo) or bool((R.quantize(lo, fmt)["scales"] != q["scales"]).any())
    assert not bool(torch.signbit(both[both == 0]).any()) and not bool(torch.signbit(lo[lo == 0]).any())
    # pins == the elements round to nearest saturates from beyond (or at) the maximum
    sc = q["scales"].to(torch.int64).repeat_interleave(R.BLOCK, dim=1)[:, :w.shape[1]]
    top = R.FORMATS[fmt][5] * torch.ldexp(torch.ones(sc.shape, dtype=torch.float64), sc - 127)
    assert torch.equal(pinned, (w.double() >= top) | (w.double() < -top))
    assert bool(pinned[5, 1]) and not bool(pinned[5, 2]) and 0.002 <= float(pinned.float().mean()) <= 0.04
    assert torch.equal(lo[pinned].double(), torch.where(w[pinned] > 0, top[pinned], -top[pinned])) and torch.equal(q["wq"][pinned], lo[pinned])
    assert float(lo[5, 2]) == -float(top[5, 2]) and float(gap[5, 2]) > 0
    # zeros, -0 and an all-zero block: lo = 0, gap = the smallest subnormal times the scale
    _, eb, M, bias, _, _ = R.FORMATS[fmt]
    sub = 2.0 ** (1 - bias - M)
    assert not lo[0, :32].any() and bool((gap[0, :32] == sub * 2.0 ** -127).all())
    assert float(lo[5, 3]) == 0.0 and float(gap[5, 3]) == sub * float(top[5, 3]) / R.FORMATS[fmt][5]
    assert float(lo[5, 4]) == -float(gap[5, 4]) == -sub * float(top[5, 4]) / R.FORMATS[fmt][5]


@pytest.mark.parametrize("fmt", R.NAMES)
def test_reference_init_reproduces_round_to_nearest_and_ties_go_up(fmt):
    w = _weights(fmt)
    nb = RR.neighbours(w, fmt)
    lo, gap = nb["lo"], nb["gap"]
    live = gap > 0
    a0 = RR.init_alpha(w, lo, gap)
    assert bool(torch.isfinite(a0).all()) and not a0[~live].any()
    hard = RR.forward(lo, gap, a0, False).float()
    rest = (w - lo) / torch.where(live, gap, torch.ones_like(gap))
    tie = live & (rest == 0.5)
    assert int(tie.sum()) >= 40 and bool((a0[tie] == 0).all())
    assert torch.equal(hard[tie], (lo + gap)[tie])                                    # ties go up ...
    rtn = R.quantize(w, fmt)["wq"]
    assert 0 < int((hard[tie] != rtn[tie]).sum()) < int(tie.sum())                    # ... the format kernel goes to the even mantissa
    assert torch.equal(hard[~tie], rtn[~tie])                                         # pins included: both give lo
    assert float(rest[5, 4]) == 1.0 and float(a0[5, 4]) == pytest.approx(2.3979, abs=1e-4)      # the tiny negative: rest rounds to 1
    # the step reference's own weight is lo + gap h to float64 rounding
    g = torch.Generator().manual_seed(3)
    alpha = (a0 + torch.randn(a0.shape, generator=g, dtype=torch.float64)).float()
    ref = RR.step(lo, gap, alpha, torch.zeros_like(w), torch.zeros_like(w), torch.randn(w.shape, generator=g) * 1e-2, (14.0, 1.0, 1e-3, 1.0),
                  grad_scale=1.0, round_weight=0.01)
    want = RR.forward(lo, gap, ref["alpha"].float(), True)
    assert bool(((ref["wq"] - want).abs() <= 1e-6 * gap.double() + 1e-300).all())
    assert torch.equal(ref["alpha"][~live], alpha.double()[~live]) and torch.equal(ref["wq"][~live], lo.double()[~live])


# ----------------------------------------------------------------------------- MXAdaRoundQuantizer, set_weight_format
def test_learned_quantiser_carries_the_fields_and_is_no_mx_quantizer():
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer, is_mx, is_mx_learned
    for fmt in R.NAMES:
        q = MXAdaRoundQuantizer(fmt, tconv=True)
        bits = R.element_bits(fmt)
        assert (q.fmt, q.tconv, q.inited, q.n_bits, q.n_levels, q.delta, q.zero_point, q.alpha, q.soft_targets) == \
               (fmt, True, True, bits, 2 ** bits, None, None, None, False)
        assert not isinstance(q, MXQuantizer) and not is_mx(q) and is_mx_learned(q) and not is_mx_learned(MXQuantizer(fmt))
        assert q.size_bits(torch.zeros(5, 8, 3, 3)) == R.size_bits(8, 45, fmt) == MXQuantizer(fmt, tconv=True).size_bits(torch.zeros(5, 8, 3, 3))
        with pytest.raises(NotImplementedError, match=f"MXAdaRoundQuantizer\\({fmt}\\): MX activations are not built"):
            q(torch.zeros(2, 3), True)
        with pytest.raises(ValueError, match="mx_fakequant: .*no CPU path"):           # before calibration: round to nearest
            q(torch.zeros(2, 3))
        q.alpha = torch.zeros(2, 3)
        with pytest.raises(ValueError, match="mx_neighbours: .*no CPU path"):          # after: the learned path
            q(torch.zeros(2, 3))
        assert "alpha" in dict(q.named_buffers())
    with pytest.raises(ValueError, match="MXAdaRoundQuantizer: unknown MX format .*the formats are"):
        MXAdaRoundQuantizer("mxfp5")


def _weighted(qnn):
    from quantization import QuantModule
    return [(n, m) for n, m in qnn.named_modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def _fields(qnn):
    return [(n, id(m.weight_quantizer), type(m.weight_quantizer).__name__, "int_weight_quantizer" in m._modules, m.use_weight_quant, m.trained)
            for n, m in _weighted(qnn)]


@pytest.mark.parametrize("arch", ["cheng", "lu2022"])
def test_set_weight_format_rounding_swaps_and_restores(arch):
    from quantization.export import weighted_modules
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer
    qnn = _toy(arch)
    units = qnn.units()
    names = list(units)
    before = _fields(qnn)
    first = {n: [m.weight_quantizer for m in weighted_modules(u)] for n, u in units.items()}
    for bad in ("soft", None, 1, "Learned", ("learned",)):
        with pytest.raises(ValueError, match="set_weight_format: rounding must be one of \\['nearest', 'learned'\\]"):
            qnn.set_weight_format("mxfp4", rounding=bad)
        with pytest.raises(ValueError, match="set_weight_format: rounding must be one of"):
            qnn.set_weight_format("no-such-format", rounding=bad)
        assert before == _fields(qnn)
    with pytest.raises(ValueError, match="set_weight_format: formats must be one of"):
        qnn.set_weight_format("mxfp5", rounding="learned")
    assert before == _fields(qnn)
    qnn.set_weight_format({names[0]: "mxfp4"}, rounding="learned")
    qnn.set_weight_format({names[2]: "mxfp8_e4m3"}, rounding="nearest")
    qnn.set_weight_format({names[1]: "mxfp6_e2m3"})                                    # the default is today's behaviour
    for n, u in units.items():
        for m, q0 in zip(weighted_modules(u), first[n]):
            q = m.weight_quantizer
            if n in names[:3]:
                cls, fmt = {names[0]: (MXAdaRoundQuantizer, "mxfp4"), names[1]: (MXQuantizer, "mxfp6_e2m3"), names[2]: (MXQuantizer, "mxfp8_e4m3")}[n]
                assert type(q) is cls and q.fmt == fmt and q.tconv == m.if_tconv and m.int_weight_quantizer is q0 and m._pack_memo == {}
            else:
                assert q is q0 and "int_weight_quantizer" not in m._modules
    assert set(qnn.weight_bits()[names[0]]["bits"].values()) == {4}
    # a re-swap in either direction keeps the FIRST quantiser; 'int' puts it back from either class
    qnn.set_weight_format({names[0]: "mxfp6_e3m2", names[2]: "mxfp4"}, rounding="learned")
    qnn.set_weight_format({names[0]: "mxfp8_e5m2"})
    for n, cls in ((names[0], MXQuantizer), (names[2], MXAdaRoundQuantizer)):
        for m, q0 in zip(weighted_modules(units[n]), first[n]):
            assert type(m.weight_quantizer) is cls and m.int_weight_quantizer is q0
    qnn.set_weight_format({names[2]: "int"})
    assert [m.weight_quantizer for m in weighted_modules(units[names[2]])] == first[names[2]]
    qnn.set_weight_format("int", rounding="learned")                                   # (the rounding of 'int' is nobody's)
    assert before == _fields(qnn)
    # the trained-unit refusal stays, for both roundings
    last = weighted_modules(units[names[-1]])[-1]
    last.trained = True
    for r in ("nearest", "learned"):
        with pytest.raises(ValueError, match=f"set_weight_format: unit '{re.escape(names[-1])}' holds a trained module"):
            qnn.set_weight_format("mxfp4", rounding=r)
    last.trained = False
    assert before == _fields(qnn)


def test_reconstruct_refusals_for_the_learned_quantiser(tmp_path, monkeypatch):
    from quantization import block_reconstruction, layer_reconstruction
    from quantization import utils
    from quantization.export import integer_state, weighted_modules
    from quantization.mx import MXQuantizer
    from quantization.recon import reconstruct
    qnn = _toy("cheng")
    units = qnn.units()

    def boom(*a, **k):
        raise AssertionError("a cache was built")
    monkeypatch.setattr(utils, "save_inp_oup_data", boom)
    from quantization import recon
    monkeypatch.setattr(recon, "save_inp_oup_data", boom)
    cali = torch.rand(2, 3, 64, 64)
    qnn.set_weight_format({"g_a.1": "mxfp4", "g_a.6": "mxfp6_e2m3"}, rounding="learned")
    ns = types.SimpleNamespace
    for args, what in ((ns(loss_mode="rd"), "loss_mode='rd'"), (ns(bias_correct="weight"), "args.bias_correct"), (ns(unit_report=True), "args.unit_report")):
        for call in (lambda: reconstruct(qnn, units["g_a.1"], "1", cali, args=args), lambda: block_reconstruction(qnn, units["g_a.1"], "1", cali, args=args),
                     lambda: layer_reconstruction(qnn, units["g_a.6"], "6", cali, args=args)):
            with pytest.raises(NotImplementedError, match=f"reconstruct: learned rounding on MX grids.*{re.escape(what)}"):
                call()
    from quantization import dp
    monkeypatch.setattr(dp, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="reconstruct: learned rounding on MX grids is not built for data-parallel calibration \\(world_size > 1\\)"):
        block_reconstruction(qnn, units["g_a.1"], "1", cali)
    monkeypatch.setattr(dp, "world", lambda: (0, 1))
    # a unit that mixes the two kinds of grid
    mods = weighted_modules(units["g_a.1"])
    kept = mods[-1].weight_quantizer
    mods[-1].weight_quantizer = mods[-1].int_weight_quantizer
    with pytest.raises(NotImplementedError, match="reconstruct: learned rounding on MX grids: module '1\\..*' holds an integer-grid quantiser next to"):
        block_reconstruction(qnn, units["g_a.1"], "1", cali)
    # ... and a plain MXQuantizer among them is refused exactly as before
    mods[-1].weight_quantizer = MXQuantizer("mxfp4")
    with pytest.raises(NotImplementedError, match="reconstruct: module '1.*' holds an MXQuantizer \\(mxfp4\\): learned rounding on MX grids is not built"):
        block_reconstruction(qnn, units["g_a.1"], "1", cali)
    mods[-1].weight_quantizer = kept
    with pytest.raises(ValueError, match="integer_state: module 'model.g_a.1.* holds an MXAdaRoundQuantizer \\(mxfp4\\): an MX grid has no integer levels"):
        integer_state(qnn)
    path = os.path.join(tmp_path, "toy.rdopack")
    with pytest.raises(ValueError, match="save_packed: module 'model.g_a.1.* holds an MXAdaRoundQuantizer \\(mxfp4\\): a packed MX container is not built"):
        qnn.save_packed(path)
    assert os.listdir(tmp_path) == []
    # with nothing refused the call goes on to build its caches
    with pytest.raises(AssertionError, match="a cache was built"):
        block_reconstruction(qnn, units["g_a.1"], "1", cali)
    qnn.set_weight_format("int")
    assert integer_state(qnn) == {}


def test_swin_units_are_refused(monkeypatch):
    from quantization import block_reconstruction, recon
    qnn = _toy("lu2022")
    units = qnn.units()
    monkeypatch.setattr(recon, "save_inp_oup_data", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a cache was built")))
    rstb = [n for n, u in units.items() if recon._is_rstb(u)]
    assert rstb
    qnn.set_weight_format({rstb[0]: "mxfp8_e4m3"}, rounding="learned")
    with pytest.raises(NotImplementedError, match="reconstruct: learned rounding on MX grids is not built for RSTB / Swin units"):
        block_reconstruction(qnn, units[rstb[0]], rstb[0], torch.rand(2, 3, 64, 64))
