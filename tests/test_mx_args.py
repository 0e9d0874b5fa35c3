"""CPU checks of the MX block formats: the float64 reference (tests/mx_reference.py) against hand-worked blocks of every format, its
idempotence and the exactness of its wq in float32, include/rdo_ptq_mx.h against `MX_FORMATS` and the built library, the refusals of the
C entries (RDO_EINVAL without touching a device) and of `ops.mx_fakequant` / `ops.mx_dequant` (ValueError before any pointer is taken),
`MXQuantizer`'s fields, and `QuantModel.set_weight_format` with the refusals that go with it, on the toy models built on the CPU (fields
only: no kernel runs)."""
import ctypes as C
import os
import re

import pytest
import torch

import mx_reference as R
from test_rd_report_args import _toy

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _block(values):
    return torch.tensor([list(values) + [0.0] * (R.BLOCK - len(values))], dtype=torch.float32)


# ----------------------------------------------------------------------------- the reference
# per format: the leading values of one block (the rest zeros; amax puts E at 0), what they become, their codes.  In the order: a
# value just under the next power of two that rounds up and saturates, a tie that goes down to the even mantissa, a tie that goes up
# to it, a subnormal, a subnormal tie (up to even), half the smallest subnormal (a tie, down to zero), a value that flushes to zero, a
# negative normal
WORKED = {
    "mxfp6_e2m3": ((7.9, 4.25, 4.75, 0.3, 0.1875, 0.0625, 0.06, -1.3), (7.5, 4.0, 5.0, 0.25, 0.25, 0.0, 0.0, -1.25),
                   (31, 24, 26, 2, 2, 0, 0, 32 | 10)),
    "mxfp6_e3m2": ((31.0, 18.0, 22.0, 0.15, 0.09375, 0.03125, 0.03, -3.0), (28.0, 16.0, 24.0, 0.125, 0.125, 0.0, 0.0, -3.0),
                   (31, 28, 30, 2, 2, 0, 0, 32 | 18)),
    "mxfp8_e4m3": ((500.0, 272.0, 336.0, 0.005, 1.5 * 2.0 ** -9, 2.0 ** -10, 0.0009, -1.3),
                   (448.0, 256.0, 320.0, 3 * 2.0 ** -9, 2.0 ** -8, 0.0, 0.0, -1.25), (126, 120, 122, 3, 2, 0, 0, 128 | 58)),
    "mxfp8_e5m2": ((63000.0, 36864.0, 45056.0, 4e-5, 1.5 * 2.0 ** -16, 2.0 ** -17, 7e-6, -1.3),
                   (57344.0, 32768.0, 49152.0, 3 * 2.0 ** -16, 2.0 ** -15, 0.0, 0.0, -1.25), (123, 120, 122, 3, 2, 0, 0, 128 | 61)),
}


def test_reference_reproduces_the_worked_mxfp4_block():
    got = R.quantize(_block((6, 5, 0.75, 0.25, -0.26, 3.5, 2.5, 1e-3)), "mxfp4")
    assert got["wq"][0, :9].tolist() == [6, 4, 1, 0, -0.5, 4, 2, 0, 0] and got["scales"].tolist() == [[127]]
    assert got["codes"][0, :9].tolist() == [7, 6, 2, 0, 8 | 1, 6, 4, 0, 0] and not got["wq"][0, 9:].any()
    # 7.9: amax just under the next power of two, the top element saturates
    assert R.quantize(_block((7.9, -7.9)), "mxfp4")["wq"][0, :2].tolist() == [6.0, -6.0]


@pytest.mark.parametrize("fmt", list(WORKED))
def test_reference_reproduces_one_hand_worked_block_per_format(fmt):
    values, want, codes = WORKED[fmt]
    got = R.quantize(_block(values), fmt)
    assert got["scales"].tolist() == [[127]]
    assert got["wq"][0, :8].tolist() == list(want)
    assert got["codes"][0, :8].tolist() == list(codes)
    # the same block 2^-40 times as large: the scale code moves by 40, the element codes stay
    small = R.quantize(_block(values) * 2.0 ** -40, fmt)
    assert small["scales"].tolist() == [[87]] and torch.equal(small["codes"], got["codes"])
    assert _same_bits(small["wq"], got["wq"] * 2.0 ** -40)


@pytest.mark.parametrize("fmt", R.NAMES)
def test_reference_is_idempotent_and_exact_in_float32(fmt):
    g = torch.Generator().manual_seed(11)
    w = torch.distributions.StudentT(3.0).sample((6, 100)) * 0.01
    w = torch.cat([w, torch.randn(6, 100, generator=g) * torch.pow(2.0, torch.arange(-149, 121, 45, dtype=torch.float32))[:, None]])
    w[0, :32] = 0.0
    w[1, 5] = -0.0
    first = R.quantize(w, fmt)                                            # (asserts inside that wq survives the trip through float32)
    again = R.quantize(first["wq"], fmt)
    assert _same_bits(first["wq"], again["wq"]) and torch.equal(first["codes"], again["codes"])
    assert _same_bits(R.dequantize(first["codes"], first["scales"], fmt), first["wq"])
    assert torch.signbit(first["wq"][1, 5]) and first["wq"][1, 5] == 0 and int(first["codes"][1, 5]) == 1 << (R.element_bits(fmt) - 1)
    assert first["scales"][0, 0] == 0 and not first["wq"][0, :32].any()
    assert first["scales"].shape == (12, 4) and int(first["scales"].max()) <= 254
    assert bool((first["err"] <= first["energy"]).all()) and again["err"].tolist() == [0.0] * 12
    bits = R.element_bits(fmt)
    assert int(first["codes"].max()) < 2 ** bits
    if fmt == "mxfp8_e4m3":
        assert not bool(((first["codes"] & 0x7F) == 0x7F).any())         # the NaN pattern is never produced
    if fmt == "mxfp8_e5m2":
        assert not bool(((first["codes"] & 0x7F) >= 0x7C).any())         # nor infinities


def test_reference_marks_a_block_that_is_not_finite():
    w = torch.ones(2, 70)
    w[0, 33], w[1, 69] = float("nan"), float("-inf")
    got = R.quantize(w, "mxfp6_e3m2")
    assert got["scales"].tolist() == [[127 - 4, 255, 127 - 4], [127 - 4, 127 - 4, 255]]
    assert bool(got["wq"][0, 32:64].isnan().all()) and bool(got["wq"][1, 64:].isnan().all())
    assert bool((got["wq"][0, :32] == 1).all()) and bool((got["wq"][1, :64] == 1).all())


# ----------------------------------------------------------------------------- the header, the exports
def test_header_ids_and_bits_match_the_host_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mx.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MX) >= {"rdo_mx_fakequant", "rdo_mx_dequant", "rdo_mx_format_bits"}
    assert '#include "rdo_ptq_hip.h"' in hdr
    assert int(re.search(r"^#define RDO_MX_BLOCK (\d+)", hdr, re.M).group(1)) == L.MX_BLOCK == R.BLOCK
    ids = {n: int(v) for n, v in re.findall(r"^#define RDO_MX_(FP[0-9A-Z_]+) (\d+)", hdr, re.M)}
    assert ids == {"FP4": 0, "FP6_E2M3": 1, "FP6_E3M2": 2, "FP8_E4M3": 3, "FP8_E5M2": 4}
    assert int(re.search(r"^#define RDO_MX_FORMATS (\d+)", hdr, re.M).group(1)) == len(L.MX_FORMATS) == 5
    assert list(L.MX_FORMATS) == list(R.NAMES)
    h = L.lib()
    for name, (fid, bits) in L.MX_FORMATS.items():
        assert ids["FP" + name[4:].upper()] == fid == R.FORMATS[name][0]
        assert h.rdo_mx_format_bits(fid) == bits == R.element_bits(name)
        row = re.search(rf"^ \*   {fid}   {name} +(\d)/(\d)/(\d) +(\d+) +(\d+) ", hdr, re.M)          # the table of the header's comment
        assert row and tuple(int(v) for v in row.groups()) == (1,) + R.FORMATS[name][1:5]
    assert [h.rdo_mx_format_bits(i) for i in (-1, 5, 255)] == [0, 0, 0]
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_BIAS, L.EXPORTS_BITS, L.EXPORTS_PACK, L.EXPORTS_SUBPEL, L.EXPORTS_ACTBITS, L.EXPORTS_ATTNQ)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert len(L.EXPORTS) == 124


def test_c_entries_refuse_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    odd = C.c_void_p(C.addressof(buf) + 2)
    names = ["w", "rows", "inner", "format", "wq", "scales", "codes", "err", "energy", "ws"]

    def call(**kw):
        a = dict(w=p, rows=3, inner=40, format=0, wq=p, scales=p, codes=p, err=p, energy=p, ws=p)
        a.update(kw)
        return h.rdo_mx_fakequant(*[a[n] for n in names], None)
    none = dict(wq=None, scales=None, codes=None, err=None, energy=None)
    bad = [dict(rows=0), dict(rows=-3), dict(inner=0), dict(inner=-40), dict(format=-1), dict(format=5), dict(format=255), none,
           dict(w=None), dict(w=odd), dict(wq=odd), dict(ws=None), dict(none, err=p, ws=None), dict(err=C.c_void_p(C.addressof(buf) + 4)),
           dict(rows=2 ** 31 - 1, inner=2 ** 40)]
    for kw in bad:
        assert call(**kw) == RDO_EINVAL, kw
        assert b"rdo_mx_fakequant" in h.rdo_last_error(), kw
    ws = h.rdo_mx_fakequant_workspace
    assert [ws(*a) for a in ((0, 40), (-1, 40), (3, 0), (3, -5), (2 ** 31 - 1, 2 ** 40))] == [0] * 5
    assert ws(3, 40) == 3 * 2 * 16 and ws(1, 1) == 16 and ws(65536, 192) == 65536 * 6 * 16
    names = ["codes", "scales", "rows", "inner", "format", "w"]

    def deq(**kw):
        a = dict(codes=p, scales=p, rows=3, inner=40, format=0, w=p)
        a.update(kw)
        return h.rdo_mx_dequant(*[a[n] for n in names], None)
    for kw in (dict(codes=None), dict(scales=None), dict(w=None), dict(rows=0), dict(inner=0), dict(format=5), dict(format=-1), dict(w=odd)):
        assert deq(**kw) == RDO_EINVAL, kw
        assert b"rdo_mx_dequant" in h.rdo_last_error(), kw


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


def test_mx_fakequant_refuses_malformed_operands(no_library):
    ops = no_library
    w = _t(3, 40)
    cases = [
        ((w.double(), "mxfp4"), {}, "w_rows must be an fp32 tensor"),
        ((None, "mxfp4"), {}, "w_rows must be an fp32 tensor"),
        ((w.to(torch.uint8), "mxfp4"), {}, "w_rows must be an fp32 tensor"),
        ((_t(120), "mxfp4"), {}, "rank 2"),
        ((_t(3, 4, 10), "mxfp4"), {}, "rank 2"),
        ((_t(0, 40), "mxfp4"), {}, "empty"),
        ((_t(3, 80)[:, ::2], "mxfp4"), {}, "contiguous"),
        ((_t(40, 3).t(), "mxfp4"), {}, "contiguous"),
        ((w, "mxfp5"), {}, "unknown MX format 'mxfp5'; the formats are \\['mxfp4', 'mxfp6_e2m3', 'mxfp6_e3m2', 'mxfp8_e4m3', 'mxfp8_e5m2'\\]"),
        ((w, 0), {}, "unknown MX format 0"),
        ((w, None), {}, "unknown MX format None"),
        ((w, "int"), {}, "unknown MX format 'int'"),
        ((w, "mxfp4"), {"want": ()}, "want must hold at least one"),
        ((w, "mxfp4"), {"want": []}, "want must hold at least one"),
        ((w, "mxfp4"), {"want": "wq"}, "want must be a sequence"),
        ((w, "mxfp4"), {"want": None}, "want must be a sequence"),
        ((w, "mxfp4"), {"want": ("wq", "delta")}, "only distinct names out of"),
        ((w, "mxfp4"), {"want": ("wq", "wq")}, "only distinct names out of"),
        ((w, "mxfp4"), {"want": ("codes",), "wq_out": w}, "wq_out is given but 'wq' is not wanted"),
        ((w, "mxfp4"), {"wq_out": _t(3, 41)}, "wq_out must be a contiguous fp32 \\[3, 40\\]"),
        ((w, "mxfp4"), {"wq_out": _t(3, 40).double()}, "wq_out must be a contiguous fp32"),
        ((w, "mxfp4"), {"wq_out": torch.zeros(3, 40, device="meta")}, "wq_out must be a contiguous fp32"),
        ((torch.zeros(2 ** 20, 2 ** 30, device="meta"), "mxfp4"), {}, "2\\^40 blocks"),
        ((w, "mxfp4"), {}, "no CPU path"),
        ((w, "mxfp8_e5m2"), {"want": ("err", "energy", "codes", "scales", "wq"), "wq_out": w}, "no CPU path"),
    ]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=f"mx_fakequant: .*{what}"):
            ops.mx_fakequant(*args, **kw)


def test_mx_dequant_refuses_malformed_operands(no_library):
    ops = no_library
    c, s = _t(3, 40, dtype=torch.uint8), _t(3, 2, dtype=torch.uint8)
    cases = [
        ((c.float(), s, 40, "mxfp4"), "codes must be an uint8 tensor"),
        ((None, s, 40, "mxfp4"), "codes must be an uint8 tensor"),
        ((_t(120, dtype=torch.uint8), s, 40, "mxfp4"), "rank 2"),
        ((_t(3, 80, dtype=torch.uint8)[:, ::2], s, 40, "mxfp4"), "contiguous"),
        ((c, s, 40, "fp4"), "unknown MX format 'fp4'; the formats are"),
        ((c, s, 41, "mxfp4"), "codes is \\(3, 40\\); inner is 41"),
        ((c, s, 0, "mxfp4"), "inner must be a whole number >= 1"),
        ((c, s, 40.0, "mxfp4"), "inner must be a whole number >= 1"),
        ((c, _t(3, 1, dtype=torch.uint8), 40, "mxfp4"), "scales must be a contiguous uint8 \\[3, 2\\]"),
        ((c, s.float(), 40, "mxfp4"), "scales must be a contiguous uint8 \\[3, 2\\]"),
        ((c, torch.zeros(3, 2, dtype=torch.uint8, device="meta"), 40, "mxfp4"), "scales must be a contiguous uint8 \\[3, 2\\]"),
        ((c, s, 40, "mxfp4"), "no CPU path"),
    ]
    for args, what in cases:
        with pytest.raises(ValueError, match=f"mx_dequant: .*{what}"):
            ops.mx_dequant(*args)


# ----------------------------------------------------------------------------- MXQuantizer
def test_quantiser_carries_what_the_module_reads():
    from quantization.mx import MX_FORMATS, MXQuantizer
    assert MX_FORMATS == R.NAMES
    for fmt in R.NAMES:
        q = MXQuantizer(fmt)
        bits = R.element_bits(fmt)
        assert (q.fmt, q.tconv, q.inited, q.n_bits, q.n_levels, q.delta, q.zero_point) == (fmt, False, True, bits, 2 ** bits, None, None)
        assert q.size_bits(torch.zeros(8, 5, 3, 3)) == R.size_bits(8, 45, fmt)
        assert q.size_bits(torch.zeros(7, 40)) == R.size_bits(7, 40, fmt) and q.size_bits(torch.zeros(40)) == R.size_bits(1, 40, fmt)
        assert q.size_bits(torch.zeros(7, 64)) == 7 * 64 * bits + 8 * 14
        assert MXQuantizer(fmt, tconv=True).size_bits(torch.zeros(5, 8, 3, 3)) == R.size_bits(8, 45, fmt)
        with pytest.raises(NotImplementedError, match=f"MXQuantizer\\({fmt}\\): MX activations are not built"):
            q(torch.zeros(2, 3), True)
        with pytest.raises(NotImplementedError, match="MX activations are not built"):
            q(torch.zeros(2, 3), act=True, site=1)
        with pytest.raises(ValueError, match="mx_fakequant: .*no CPU path"):
            q(torch.zeros(2, 3))
    for bad in ("mxfp5", "int", 4, None):
        with pytest.raises(ValueError, match="MXQuantizer: unknown MX format .*the formats are"):
            MXQuantizer(bad)


# ----------------------------------------------------------------------------- set_weight_format and the refusals around it
def _weighted(qnn):
    from quantization import QuantModule
    return [(n, m) for n, m in qnn.named_modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def _fields(qnn):
    return [(n, id(m.weight_quantizer), type(m.weight_quantizer).__name__, "int_weight_quantizer" in m._modules, m.use_weight_quant, m.trained)
            for n, m in _weighted(qnn)]


def test_set_weight_format_refuses_before_anything_is_written():
    qnn = _toy("cheng")
    before = _fields(qnn)
    names = list(qnn.units())
    cases = [
        (None, "formats must be one of \\['mxfp4', 'mxfp6_e2m3', 'mxfp6_e3m2', 'mxfp8_e4m3', 'mxfp8_e5m2', 'int'\\] or a mapping"),
        ("mxfp5", "formats must be one of"),
        (4, "formats must be one of"),
        (["mxfp4"], "formats must be one of"),
        ({"g_a.99": "mxfp4"}, "unknown unit name\\(s\\) \\['g_a.99'\\]"),
        ({names[0]: "mxfp4", "model.g_a.0": "mxfp4"}, "unknown unit name"),
        ({names[0]: "mxfp4", names[1]: "fp4"}, f"the format of unit '{re.escape(names[1])}' must be one of"),
        ({names[0]: "mxfp4", names[-1]: 6}, "must be one of"),
        ({names[0]: None}, "must be one of"),
    ]
    for formats, what in cases:
        with pytest.raises(ValueError, match=f"set_weight_format: .*{what}"):
            qnn.set_weight_format(formats)
        assert before == _fields(qnn)
    # a trained module in the LAST named unit: the first one is not written either
    from quantization.export import weighted_modules
    last = weighted_modules(qnn.units()[names[-1]])[-1]
    for formats in ("mxfp6_e2m3", {names[0]: "mxfp4", names[-1]: "int"}):
        last.trained = True
        with pytest.raises(ValueError, match=f"set_weight_format: unit '{re.escape(names[-1])}' holds a trained module"):
            qnn.set_weight_format(formats)
        last.trained = False
        assert before == _fields(qnn)


@pytest.mark.parametrize("arch", ["cheng", "lu2022"])
def test_set_weight_format_swaps_and_restores_the_quantiser_objects(arch):
    """fields only: no kernel runs, so the CPU-built toy models do"""
    from quantization.export import weighted_modules
    from quantization.mx import MXQuantizer
    qnn = _toy(arch)
    units = qnn.units()
    names = list(units)
    before = _fields(qnn)
    first = {n: [m.weight_quantizer for m in weighted_modules(u)] for n, u in units.items()}
    for m in (m for u in units.values() for m in weighted_modules(u)):
        m._pack_memo = {"q": "stale"}
    qnn.set_weight_format({names[0]: "mxfp4", names[2]: "mxfp8_e4m3"})
    for n, u in units.items():
        for m, q0 in zip(weighted_modules(u), first[n]):
            q = m.weight_quantizer
            if n in (names[0], names[2]):
                assert isinstance(q, MXQuantizer) and q.fmt == ("mxfp4" if n == names[0] else "mxfp8_e4m3") and q.tconv == m.if_tconv
                assert m.int_weight_quantizer is q0 and m._pack_memo == {}
            else:
                assert q is q0 and "int_weight_quantizer" not in m._modules and m._pack_memo == {"q": "stale"}
    bits = qnn.weight_bits()                                               # element bits only
    assert set(bits[names[0]]["bits"].values()) == {4} and set(bits[names[1]]["bits"].values()) == {8}
    qnn.set_weight_format("mxfp6_e3m2")                                    # one name for every unit; the kept quantiser stays the first one
    for n, u in units.items():
        for m, q0 in zip(weighted_modules(u), first[n]):
            assert m.weight_quantizer.fmt == "mxfp6_e3m2" and m.int_weight_quantizer is q0
    qnn.set_weight_format({names[1]: "int"})
    assert [m.weight_quantizer for m in weighted_modules(units[names[1]])] == first[names[1]]
    qnn.set_weight_format("int")                                           # also over units that hold no MX quantiser any more
    assert before == _fields(qnn)
    qnn.set_weight_format("int")
    assert before == _fields(qnn)


def test_refusals_where_an_mx_quantiser_cannot_be_served(tmp_path, monkeypatch):
    from quantization import block_reconstruction, layer_reconstruction, BaseQuantBlock
    from quantization import utils
    from quantization.export import integer_state
    from quantization.recon import reconstruct
    qnn = _toy("cheng")
    units = qnn.units()
    name = "g_a.1"
    assert isinstance(units[name], BaseQuantBlock) and not isinstance(units["g_a.6"], BaseQuantBlock)
    qnn.set_weight_format({name: "mxfp4", "g_a.6": "mxfp6_e2m3"})

    def boom(*a, **k):
        raise AssertionError("a cache was built")
    monkeypatch.setattr(utils, "save_inp_oup_data", boom)
    cali = torch.rand(2, 3, 64, 64)
    for call in (lambda: reconstruct(qnn, units[name], "1", cali), lambda: block_reconstruction(qnn, units[name], "1", cali),
                 lambda: layer_reconstruction(qnn, units["g_a.6"], "6", cali)):
        with pytest.raises(NotImplementedError, match="reconstruct: module '[16].*' holds an MXQuantizer \\(mxfp.*learned rounding on MX grids is not built"):
            call()
    with pytest.raises(ValueError, match="integer_state: module 'model.g_a.1.* holds an MXQuantizer \\(mxfp4\\)"):
        integer_state(qnn)
    path = os.path.join(tmp_path, "toy.rdopack")
    with pytest.raises(ValueError, match="save_packed: module 'model.g_a.1.* holds an MXQuantizer \\(mxfp4\\): a packed MX container is not built"):
        qnn.save_packed(path)
    assert os.listdir(tmp_path) == []
    qnn.set_weight_format("int")
    assert integer_state(qnn) == {}                                        # (no quantiser is initialised on the CPU model)


def test_format_report_refuses_bad_arguments_before_any_gpu_work(monkeypatch):
    from hipops import _lib as L
    from quantization import QuantModel
    from quantization.export import format_report, weighted_modules
    qnn = _toy("cheng")
    before = _fields(qnn)

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(QuantModel, "forward", boom)
    img = torch.rand(2, 3, 64, 128)
    cases = [
        (dict(images=torch.rand(3, 64, 64)), "images must be \\[n, 3, H, W\\]"),
        (dict(images=torch.rand(2, 3, 64, 96)), "multiples of 64"),
        (dict(lmbda=0.0), "lmbda must be a positive finite number"),
        (dict(batch=0), "batch must be an integer >= 1"),
        (dict(units=["g_a.0", "g_a.99"]), "unknown unit name\\(s\\) \\['g_a.99'\\]"),
        (dict(formats=()), "formats must hold at least one name"),
        (dict(formats="mxfp4"), "formats must be a sequence"),
        (dict(formats=None), "formats must be a sequence"),
        (dict(formats=("mxfp4", "int")), "unknown MX format 'int'; the formats are"),
        (dict(formats=("mxfp4", 6)), "unknown MX format 6"),
        (dict(formats=("mxfp4", "mxfp4")), "distinct"),
    ]
    for kw, what in cases:
        kw = dict(dict(images=img), **kw)
        with pytest.raises(ValueError, match=f"format_report: .*{what}"):
            format_report(qnn, **kw)
        with pytest.raises(ValueError, match=f"format_report: .*{what}"):
            qnn.format_report(**kw)
    m = weighted_modules(qnn.units()["g_a.0"])[-1]
    m.trained = True
    with pytest.raises(ValueError, match="format_report: unit 'g_a.0' holds a trained module"):
        qnn.format_report(img)
    m.trained = False
    monkeypatch.undo()
    # the argument checks are passed: scoring the weights is the first GPU work, and on a CPU model it refuses; everything is put back
    with pytest.raises(ValueError, match="mx_fakequant: .*no CPU path"):
        qnn.format_report(img, units=["g_a.1"])
    assert before == _fields(qnn)
