"""CPU checks of the RD report: the float64 / float32 restatements of the per-channel rate sums (tests/rate_channels_reference.py) against
plain loops and against the derived bound, the refusals of `ops.neg_log2_channel_sums` (ValueError before any pointer is taken) and of
the C entry, the header and the exports, `QuantModel.units()` on the toy models, and every argument refusal of `rd_report`."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import rate_channels_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDO_EINVAL = -22
WQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
AQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}


# ----------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("outer,C,inner", [(1, 1, 1), (2, 3, 5), (2, 3, 1), (1, 2, 4), (5, 3, 1)])
def test_restatement_matches_plain_loops(outer, C, inner):
    """both layouts ((o, c, i) at ((o C) + c) inner + i; inner == 1 is the channels-last storage of outer pixels)"""
    lik = R.make_lik(outer, C, inner, seed=3)
    flat = lik.reshape(-1).tolist()
    want, wabs = [0.0] * C, [0.0] * C
    for o in range(outer):
        for c in range(C):
            for i in range(inner):
                t = -math.log2(flat[((o * C) + c) * inner + i])
                want[c] += t
                wabs[c] += abs(t)
    bits, tot = R.channel_bits(lik, outer, C, inner)
    assert bits.dtype == torch.float64 and bits.shape == (C,)
    np.testing.assert_allclose(bits.numpy(), want, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(tot.numpy(), wabs, rtol=1e-13, atol=1e-300)
    got32 = R.channel_sums32(lik, outer, C, inner)
    assert got32.dtype == np.float32 and got32.shape == (C,)
    np.testing.assert_allclose(got32, want, rtol=1e-5, atol=1e-6)


def test_geometry_and_depth_of_the_test_shapes():
    assert R.geometry(1, 1, 1) == (256, 1) and R.geometry(2, 192, 256) == (256, 1) and R.geometry(3, 5, 1000) == (256, 2)
    assert R.geometry(3000, 5, 1) == (51, 8) and R.geometry(512, 7, 1) == (36, 2) and R.geometry(1536, 320, 1) == (4, 48)
    assert R.geometry(10 ** 7, 3, 1)[1] == 256                                   # the cap on the workgroups down a channel
    assert R.depth(1, 1, 1) == 1 + 8 + 1 + 4 and R.depth(1536, 320, 1) == 8 + 2 + 3 + 4 and R.depth(3000, 5, 1) == 8 + 6 + 1 + 4


@pytest.mark.parametrize("outer,C,inner", R.SHAPES)
def test_float32_restatement_stays_within_the_derived_bound(outer, C, inner):
    """the GPU test's inputs, both storages: the reference alone must stay inside the bound it sets for the kernel"""
    lik = R.make_lik(outer, C, inner, seed=100 + outer + C + inner)
    bits, tot = R.channel_bits(lik, outer, C, inner)
    for o2, i2 in ((outer, inner), (outer * inner, 1)):
        got = torch.from_numpy(R.channel_sums32(lik if i2 == inner else lik.permute(0, 2, 1).contiguous(), o2, C, i2).astype(np.float64))
        bound = R.channel_bound(o2, C, i2, tot)
        share = float(((got - bits).abs() / bound).max())
        print(f"restatement ({o2}, {C}, {i2}): share of the bound {share:.3f}")
        assert share <= 1.0
    # exact case: integer terms, every order gives the same bits
    idx = torch.arange(outer * C * inner)
    exact = torch.pow(2.0, -(1.0 + (idx % 7).float())).reshape(outer, C, inner)
    want = (1 + idx % 7).reshape(outer, C, inner).sum((0, 2)).double()
    assert torch.equal(torch.from_numpy(R.channel_sums32(exact, outer, C, inner).astype(np.float64)), want)
    assert torch.equal(R.channel_bits(exact, outer, C, inner)[0], want)


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
    return torch.ones(*shape, dtype=dtype)


def test_wrapper_refuses_malformed_operands(no_library):
    ops = no_library
    x = _t(2, 5, 4, 3)
    cases = [
        ((x,), {}, "no CPU path"),
        ((x.contiguous(memory_format=torch.channels_last),), {}, "no CPU path"),
        ((x.double(),), {}, "lik must be an fp32 tensor"),
        ((x.half(),), {}, "lik must be an fp32 tensor"),
        ((x.to(torch.int32),), {}, "lik must be an fp32 tensor"),
        ((None,), {}, "lik must be an fp32 tensor"),
        ((_t(2, 5, 12),), {}, "must be 4-D"),
        ((_t(2, 5, 4, 3, 1),), {}, "must be 4-D"),
        ((_t(()),), {}, "must be 4-D"),
        ((_t(0, 5, 4, 3),), {}, "empty"),
        ((_t(2, 0, 4, 3),), {}, "empty"),
        ((_t(2, 5, 4, 0),), {}, "empty"),
        ((x,), {"out": _t(4)}, "out must be a contiguous fp32 \\[5\\]"),
        ((x,), {"out": _t(1, 5)}, "out must be a contiguous fp32 \\[5\\]"),
        ((x,), {"out": _t(5).double()}, "out must be a contiguous fp32 \\[5\\]"),
        ((x,), {"out": _t(10)[::2]}, "out must be a contiguous fp32 \\[5\\]"),
        ((x,), {"out": torch.ones(5, device="meta")}, "out must be a contiguous fp32 \\[5\\]"),
        ((x,), {"out": 0.0}, "out must be a contiguous fp32 \\[5\\]"),
        ((x,), {"out": _t(5)}, "no CPU path"),
    ]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=f"neg_log2_channel_sums: .*{what}"):
            ops.neg_log2_channel_sums(*args, **kw)


# ----------------------------------------------------------------------------- the C entry, the header, the exports
def test_c_abi_refuses_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments below are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    bad = [(None, 2, 3, 4, p, p), (p, 2, 3, 4, None, p), (p, 2, 3, 4, p, None), (p, 0, 3, 4, p, p), (p, -2, 3, 4, p, p), (p, 2, 0, 4, p, p),
           (p, 2, -3, 4, p, p), (p, 2, 3, 0, p, p), (p, 2, 3, -4, p, p),
           (p, 2 ** 31, 3, 1, p, p), (p, 2 ** 16, 3, 2 ** 15, p, p), (p, 1, 3, 2 ** 31, p, p), (p, 2, 65536, 4, p, p), (p, 2 ** 40, 3, 2 ** 40, p, p)]
    for args in bad:
        assert h.rdo_neg_log2_channel_sums(*args, None) == RDO_EINVAL, args
        assert b"rdo_neg_log2_channel_sums" in h.rdo_last_error()
        if all(a is not None for a in args):
            assert h.rdo_neg_log2_channel_sums_workspace(*args[1:4]) == 0
    # the workspace: C partial rows of S entries, S as in the reference's geometry
    for outer, Cc, inner in R.SHAPES + [(3000, 5, 1), (10 ** 7, 3, 1), (2 ** 31 - 1, 65535, 1)]:
        assert h.rdo_neg_log2_channel_sums_workspace(outer, Cc, inner) == Cc * R.geometry(outer, Cc, inner)[1]


def test_header_declares_and_library_exports_both_symbols():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_hip.h")).read()
    assert re.search(r"^int rdo_neg_log2_channel_sums\(const float\* lik, int64_t outer, int32_t C, int64_t inner,", hdr, re.M)
    assert re.search(r"^int64_t rdo_neg_log2_channel_sums_workspace\(int64_t outer, int32_t C, int64_t inner\);", hdr, re.M)
    h = L.lib()
    for name in ("rdo_neg_log2_channel_sums", "rdo_neg_log2_channel_sums_workspace"):
        assert name in L.EXPORTS and hasattr(h, name)
    assert len(L.EXPORTS) == 124
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "124" in design


# ----------------------------------------------------------------------------- QuantModel.units()
NIC_CFG = dict(height=64, width=64, in_chans=3, embed_dim=16, latent_dim=32, window_size=8, mlp_ratio=2.0, qkv_bias=True, qk_scale=None,
               drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_checkpoint=False)


def _toy(arch):
    import lic
    from quantization import QuantModel
    torch.manual_seed(5)
    if arch == "cheng":
        return QuantModel(lic.Cheng2020Anchor(N=8).eval(), WQ, AQ, is_cheng=True).eval()
    if arch == "minnen":
        return QuantModel(lic.MeanScaleHyperprior(N=8, M=12).eval(), WQ, AQ).eval()
    return QuantModel(lic.NIC(NIC_CFG).eval(), WQ, AQ).eval()


def _walk_rule_from(mod, prefix):
    """the rule restated: children in definition order; a QuantModule or a block is a unit and is not entered, anything else is entered
    where it stands, its name and a dot in front of its children's"""
    from quantization import BaseQuantBlock, QuantModule
    out = []
    for n, c in mod.named_children():
        out.extend([(prefix + n, c)] if isinstance(c, (QuantModule, BaseQuantBlock)) else _walk_rule_from(c, prefix + n + "."))
    return out


@pytest.mark.parametrize("arch", ["cheng", "minnen", "lu2022"])
def test_units_follow_the_walk_rule_and_leave_out_weightless_modules(arch):
    from collections import OrderedDict
    from quantization import BaseQuantBlock, QuantModule
    qnn = _toy(arch)
    units = qnn.units()
    assert isinstance(units, OrderedDict) and len(units) > 4
    walked = _walk_rule_from(qnn.model, "")
    want = [(n, u) for n, u in walked if not (isinstance(u, QuantModule) and u.org_weight is None)]
    assert list(units) == [n for n, _ in want] and all(units[n] is u for n, u in want)
    named = dict(qnn.named_modules())
    for n, u in units.items():
        assert named["model." + n] is u and isinstance(u, (QuantModule, BaseQuantBlock))
        assert not (isinstance(u, QuantModule) and u.org_weight is None)
    # no unit inside another, and every weighted QuantModule of the model inside exactly one unit
    inside = [id(m) for u in units.values() for m in u.modules() if isinstance(m, QuantModule) and m.org_weight is not None]
    every = [id(m) for m in qnn.modules() if isinstance(m, QuantModule) and m.org_weight is not None]
    assert sorted(inside) == sorted(every) and len(set(inside)) == len(inside)
    weightless = [n for n, u in walked if isinstance(u, QuantModule) and u.org_weight is None]
    assert all(n not in units for n in weightless)
    if arch == "cheng":
        assert list(units)[:2] == ["g_a.0", "g_a.1"] and "g_a.6" in units
        assert weightless                                 # the pixel shuffles of the sub-pixel convolutions


def test_units_agree_with_the_bench_walker():
    import bench
    qnn = _toy("cheng")
    assert [(n, id(u)) for n, u in bench.unit_list(qnn)] == [(n, id(u)) for n, u in qnn.units().items()]


# ----------------------------------------------------------------------------- rd_report: the argument refusals
def test_rd_report_refuses_bad_arguments_before_any_gpu_work(monkeypatch):
    from hipops import _lib as L
    from quantization import QuantModel
    from quantization.export import rd_report
    qnn = _toy("cheng")
    flags = [(m.use_weight_quant, m.use_act_quant) for m in qnn.modules() if hasattr(m, "use_weight_quant")]

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(QuantModel, "forward", boom)
    img = torch.rand(2, 3, 64, 128)
    cases = [
        (dict(images=torch.rand(3, 64, 64)), "images must be \\[n, 3, H, W\\]"),
        (dict(images=torch.rand(2, 1, 64, 64)), "images must be \\[n, 3, H, W\\]"),
        (dict(images=torch.rand(2, 4, 64, 64)), "images must be \\[n, 3, H, W\\]"),
        (dict(images=torch.rand(0, 3, 64, 64)), "images is empty"),
        (dict(images=torch.rand(2, 3, 64, 96)), "multiples of 64"),
        (dict(images=torch.rand(2, 3, 63, 64)), "multiples of 64"),
        (dict(images=torch.rand(2, 3, 64, 64).double()), "images must be an fp32 tensor"),
        (dict(images=[[1.0]]), "images must be an fp32 tensor"),
        (dict(lmbda=0.0), "lmbda must be a positive finite number"),
        (dict(lmbda=-0.01), "lmbda must be a positive finite number"),
        (dict(lmbda=float("inf")), "lmbda must be a positive finite number"),
        (dict(lmbda=float("nan")), "lmbda must be a positive finite number"),
        (dict(lmbda="0.01"), "lmbda must be a positive finite number"),
        (dict(lmbda=None), "lmbda must be a positive finite number"),
        (dict(lmbda=True), "lmbda must be a positive finite number"),
        (dict(batch=0), "batch must be an integer >= 1"),
        (dict(batch=-1), "batch must be an integer >= 1"),
        (dict(batch=2.0), "batch must be an integer >= 1"),
        (dict(batch=True), "batch must be an integer >= 1"),
        (dict(batch=None), "batch must be an integer >= 1"),
        (dict(act_quant=1), "act_quant must be True or False"),
        (dict(act_quant=None), "act_quant must be True or False"),
        (dict(act_quant="yes"), "act_quant must be True or False"),
        (dict(units=["g_a.0", "g_a.99"]), "unknown unit name\\(s\\) \\['g_a.99'\\]"),
        (dict(units=["model.g_a.0"]), "unknown unit name"),
        (dict(units="g_a.0"), "units must be None or a list of unit names"),
        (dict(units=[0]), "units must be None or a list of unit names"),
    ]
    for kw, what in cases:
        kw = dict(dict(images=img), **kw)
        with pytest.raises(ValueError, match=f"rd_report: .*{what}"):
            rd_report(qnn, **kw)
        with pytest.raises(ValueError, match=f"rd_report: .*{what}"):
            qnn.rd_report(**kw)
    assert flags == [(m.use_weight_quant, m.use_act_quant) for m in qnn.modules() if hasattr(m, "use_weight_quant")]


def test_rd_report_on_the_cpu_fails_loudly_and_restores_the_flags():
    """well-formed arguments on a CPU model: the first forward raises (there is no CPU path), and the flags come back"""
    from quantization import BaseQuantBlock, QuantModule
    qnn = _toy("cheng")
    mods = [m for m in qnn.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    for k, m in enumerate(mods):
        m.use_weight_quant, m.use_act_quant = k % 2 == 0, k % 3 == 0
    before = [(m.use_weight_quant, m.use_act_quant, m.trained) for m in mods]
    with pytest.raises(RuntimeError):
        qnn.rd_report(torch.rand(1, 3, 64, 64))
    assert before == [(m.use_weight_quant, m.use_act_quant, m.trained) for m in mods]


def test_quant_state_puts_back_what_it_found_whatever_the_block_did():
    """`utils.quant_state` on mixed flags: restored after a normal exit and after an exception, to the recorded pairs and not to a state
    the block switched to (through `set`, one flag or both, or through the modules' own `set_quant_state`)"""
    from quantization import BaseQuantBlock, QuantModule
    from quantization.utils import quant_state
    qnn = _toy("cheng")
    mods = [m for m in qnn.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    for k, m in enumerate(mods):
        m.use_weight_quant, m.use_act_quant = k % 2 == 0, k % 3 == 0
    before = [(m.use_weight_quant, m.use_act_quant) for m in mods]
    assert len(set(before)) == 4                                         # (every combination is among them)

    def flags():
        return [(m.use_weight_quant, m.use_act_quant) for m in mods]
    with quant_state(qnn) as state:                                      # nothing given: nothing set
        assert state.mods == mods and flags() == before
    assert flags() == before
    with quant_state(qnn, True, False) as state:
        assert flags() == [(True, False)] * len(mods)
        state.set(False, True)
        assert flags() == [(False, True)] * len(mods)
        state.set(weight=True)                                           # one flag: the other stays
        assert flags() == [(True, True)] * len(mods)
    assert flags() == before
    with pytest.raises(KeyError, match="inside"):
        with quant_state(qnn, weight=True):
            assert flags() == [(True, a) for _, a in before]
            qnn.set_quant_state(False, False)
            raise KeyError("inside")
    assert flags() == before
    unit = mods[1]                                                       # a sub-tree: the rest of the model is not its business
    inside = [m for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    with quant_state(unit, True, True) as state:
        assert state.mods == inside
        assert [f for m, f in zip(mods, flags()) if m not in inside] == [f for m, f in zip(mods, before) if m not in inside]
    assert flags() == before


def test_held_attrs_puts_back_what_it_found_whatever_the_block_did():
    """`utils.held_attrs` on two plain objects: a present attribute gets its identical object back, an absent one is absent again --
    after a normal exit and after an exception, and when the block itself replaced, set or deleted the attribute"""
    from quantization.utils import held_attrs

    class Thing:
        pass
    a, b = Thing(), Thing()
    grid, stats = [1.0, 2.0], {"n": 3}
    a.delta, a.act_stats = grid, stats                                   # b has neither; `other` is not held
    a.other = b.other = "kept"
    fields = ("delta", "act_stats")

    def check():
        assert a.delta is grid and a.act_stats is stats and vars(a) == {"delta": grid, "act_stats": stats, "other": a.other}
        assert vars(b) == {"other": b.other}
    with held_attrs([a, b], fields):                                     # nothing touched
        pass
    check()
    with held_attrs([a, b], fields):                                     # replaced by an equal copy; set where absent
        a.delta, a.act_stats = list(grid), dict(stats)
        b.delta, b.act_stats = [0.5], {}
        a.other = b.other = "written"                                    # (a field that is not held stays as the block left it)
    check()
    assert a.other == "written"
    with held_attrs([a, b], fields):                                     # deleted, and set then deleted
        del a.delta, a.act_stats
        b.delta = [0.5]
        del b.delta
    check()
    with pytest.raises(KeyError, match="inside"):
        with held_attrs([a, b], fields):
            a.delta, b.act_stats = None, {}
            del a.act_stats
            raise KeyError("inside")
    check()


def test_product_still_never_imports_the_oracle():
    for base, _, files in os.walk(os.path.join(ROOT, "rdo-ptq_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(base, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, re.M), f"{f} imports the oracle"
    for f in ("hipops/ops.py", "quantization/export.py", "quantization/reports.py", "quantization/widths.py", "quantization/quant_model.py"):
        assert "oracle" not in open(os.path.join(ROOT, "rdo-ptq_amd", f)).read()
