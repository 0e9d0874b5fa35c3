"""MX block formats on the GPU: `ops.mx_fakequant` / `ops.mx_dequant` (csrc/mx_quant.hip) bit for bit against the float64 reference
(tests/mx_reference.py) on heavy-tailed rows and on crafted blocks, the float64 sums, round trips and aliasing, blocks that are not
finite; `MXQuantizer` on the four weight layouts and inside a QuantModule; `QuantModel.set_weight_format` and the refusals around it;
`format_report` against `rd_report`, the arithmetic of its size columns, the reference's error sums, and the state it leaves behind.

The allowed difference of the float64 sums is derived, nothing in it is measured: the kernel and the reference add the SAME exact terms
((double)d * (double)d holds the 48-bit product of two fp32 values), all non-negative, in different orders, so two orders differ by less
than inner 2^-52 of the sum per row (tests/test_gpu_bit_alloc.py derives it)."""
import functools
import os

import pytest
import torch

import mx_reference as R
from test_gpu_rd_report import LMBDA, _cheng, _same_report

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 31), (3, 32), (3, 33), (2, 27), (4, 1728), (2, 8193), (257, 64)]
ALL = ("wq", "scales", "codes", "err", "energy")


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _student(rows, inner):
    """heavy-tailed rows: Student-t(3) x 0.01, seeded (left unchanged by every test)"""
    torch.manual_seed(1000 * rows + inner)
    return (torch.distributions.StudentT(3.0).sample((rows, inner)) * 0.01).float().contiguous()


@functools.lru_cache(maxsize=None)
def _crafted(fmt):
    """a matrix [rows, 103] (three whole blocks and one of seven elements a row) whose blocks hold: only zeros; an amax that is an exact
    power of two; an amax just under the next power of two, so that the top element saturates; every multiple of half a step at every
    binade of the format, subnormal ties included, at E = 0, E = -120 and under the clamp E = -127; elements 2^-20 x amax; -0.0; fp32
    subnormals only; amax = 3e38"""
    _, eb, M, bias, emax, vmax = R.FORMATS[fmt]
    g = torch.Generator().manual_seed(7)
    blocks = [torch.zeros(32)]
    b = (torch.rand(32, generator=g) - 0.5) * 0.2
    b[5] = 0.125
    blocks.append(b)
    b = (torch.rand(32, generator=g) - 0.5) * 8
    b[9], b[10] = 7.9, -7.9
    blocks.append(b)
    b = (torch.rand(32, generator=g) - 0.5) * 8
    b[31] = -torch.nextafter(torch.tensor(8.0), torch.tensor(0.0))
    blocks.append(b)
    vals = [k * 2.0 ** (e - 1) for e in range(1 - bias - M - 3, emax + 2) for k in range(2 ** (M + 2) + 1)]
    t = torch.tensor(vals, dtype=torch.float64)
    t = torch.cat([t, -t])
    t = torch.cat([t, torch.zeros((-t.numel()) % 31, dtype=torch.float64)]).reshape(-1, 31)
    t = torch.cat([t, torch.full((t.shape[0], 1), 2.0 ** emax * 1.99, dtype=torch.float64)], 1)      # every block's amax: E = 0
    for scale in (1.0, 2.0 ** -120, 2.0 ** -140):
        blocks += list((t * scale).float())
    b = torch.full((32,), 3.0 * 2.0 ** -20)
    b[::2] *= -1
    b[17] = 3.0
    blocks.append(b)
    b = (torch.rand(32, generator=g) - 0.5) * 2
    b[::3] = -0.0
    blocks.append(b)
    blocks.append(torch.full((32,), -0.0))
    blocks.append((torch.arange(32, dtype=torch.float64) * 2.0 ** -149).float())                      # amax = 31 x 2^-149
    b = ((torch.rand(32, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** -126).float()
    b[3] = 0.75 * 2.0 ** -126
    blocks.append(b)
    b = (torch.rand(32, generator=g) - 0.5) * 1e38
    b[0], b[1], b[2], b[3], b[4] = 3e38, -2.5e38, 1e30, 1.0, -3e38
    blocks.append(b)
    blocks += [torch.zeros(32)] * ((-len(blocks)) % 4)
    rows = [torch.cat([blocks[i], blocks[i + 1], blocks[i + 2], blocks[i + 3][:7]]) for i in range(0, len(blocks), 4)]
    # the fourth block of every row is cut to seven elements: the same blocks again, rotated by one, so that each is whole somewhere
    rows += [torch.cat([blocks[i + 3], blocks[i], blocks[i + 1], blocks[i + 2][:7]]) for i in range(0, len(blocks), 4)]
    w = torch.stack(rows).contiguous()
    assert w.shape[1] == 103 and bool(torch.isfinite(w).all())
    return w


INPUTS = [("student",) + s for s in SHAPES] + [("crafted",)]


@functools.lru_cache(maxsize=None)
def _case(fmt, kind, *shape):
    """(w on the CPU, w on the GPU, the reference's outputs): computed once, shared, left unchanged"""
    w = _student(*shape) if kind == "student" else _crafted(fmt)
    return w, w.cuda(), R.quantize(w, fmt)


def _ids(v):
    return "x".join(str(s) for s in v) if isinstance(v, tuple) else None


@pytest.mark.parametrize("inp", INPUTS, ids=_ids)
@pytest.mark.parametrize("fmt", R.NAMES)
def test_outputs_equal_the_reference_bit_for_bit(fmt, inp):
    from hipops import ops
    w, wg, ref = _case(fmt, *inp)
    rows, inner = w.shape
    out = ops.mx_fakequant(wg, fmt, want=ALL)
    assert list(out) == list(ALL)
    assert out["wq"].dtype == torch.float32 and out["scales"].dtype == out["codes"].dtype == torch.uint8
    assert out["scales"].shape == (rows, R.blocks(inner)) and out["codes"].shape == out["wq"].shape == (rows, inner)
    assert _same_bits(out["wq"].cpu(), ref["wq"])
    assert torch.equal(out["scales"].cpu(), ref["scales"])
    assert torch.equal(out["codes"].cpu(), ref["codes"])
    assert _same_bits(wg.cpu(), w)                                                  # the operand is not written
    if inp[0] == "crafted":
        assert 0 in ref["scales"] and 127 in ref["scales"] and int(ref["scales"].max()) == 127 + 127 - R.FORMATS[fmt][4]
        if fmt == "mxfp4":
            sat = w.abs() == torch.tensor(7.9)
            assert bool((ref["wq"][sat].abs() == 6.0).all()) and int(sat.sum()) >= 2
    # each output alone and the default: the same bits
    for name in ALL:
        assert _same_bits(ops.mx_fakequant(wg, fmt, want=(name,))[name], out[name]), name
    assert _same_bits(ops.mx_fakequant(wg, fmt)["wq"], out["wq"])


@pytest.mark.parametrize("inp", INPUTS, ids=_ids)
@pytest.mark.parametrize("fmt", R.NAMES)
def test_sums_stay_within_the_derived_bound_and_repeat_bit_for_bit(fmt, inp):
    from hipops import ops
    w, wg, ref = _case(fmt, *inp)
    inner = w.shape[1]
    out = ops.mx_fakequant(wg, fmt, want=("err", "energy"))
    assert out["err"].dtype == out["energy"].dtype == torch.float64 and out["err"].shape == (w.shape[0],) and out["err"].is_cuda
    for name in ("err", "energy"):
        got, want = out[name].cpu(), ref[name]
        bound = inner * 2.0 ** -52 * want
        worst = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
        print(f"{fmt} {inp} {name}: largest share of the derived bound {worst:.3f}")
        assert bool(((got - want).abs() <= bound).all()), name
    # the same bits again, also behind a poisoned workspace
    assert ops._workspaces("mx_fakequant")
    for ws in ops._workspaces("mx_fakequant"):
        ws.fill_(float("nan"))
    again = ops.mx_fakequant(wg, fmt, want=("err", "energy"))
    assert _same_bits(again["err"], out["err"]) and _same_bits(again["energy"], out["energy"])


@pytest.mark.parametrize("inp", INPUTS, ids=_ids)
@pytest.mark.parametrize("fmt", R.NAMES)
def test_round_trips_and_aliasing(fmt, inp):
    from hipops import ops
    w, wg, ref = _case(fmt, *inp)
    rows, inner = w.shape
    out = ops.mx_fakequant(wg, fmt, want=("wq", "scales", "codes"))
    assert _same_bits(ops.mx_dequant(out["codes"], out["scales"], inner, fmt), out["wq"])
    assert _same_bits(R.dequantize(ref["codes"], ref["scales"], fmt), ref["wq"])
    twice = ops.mx_fakequant(out["wq"], fmt, want=("wq", "err"))
    assert _same_bits(twice["wq"], out["wq"]) and not bool(twice["err"].any())
    # in place
    buf = wg.clone()
    got = ops.mx_fakequant(buf, fmt, want=("wq", "err"), wq_out=buf)
    assert got["wq"] is buf and _same_bits(buf, out["wq"])
    assert _same_bits(got["err"], ops.mx_fakequant(wg, fmt, want=("err",))["err"])
    # an operand that starts one float into its buffer
    store = torch.full((rows * inner + 3,), float("nan"), device="cuda")
    view = store[1:1 + rows * inner].view(rows, inner)
    view.copy_(wg)
    assert view.data_ptr() == store.data_ptr() + 4 and view.is_contiguous()
    shifted = ops.mx_fakequant(view, fmt, want=("wq", "scales", "codes"))
    assert all(_same_bits(shifted[k], out[k]) for k in shifted)
    dst = torch.full((rows * inner + 3,), float("nan"), device="cuda")
    ops.mx_fakequant(view, fmt, wq_out=dst[1:1 + rows * inner].view(rows, inner))
    assert _same_bits(dst[1:-2].view(rows, inner), out["wq"]) and bool(dst[0].isnan()) and bool(dst[-2:].isnan().all())


@pytest.mark.parametrize("fmt", R.NAMES)
def test_a_block_that_is_not_finite_is_marked_and_the_others_are_untouched(fmt):
    from hipops import ops
    w = _student(3, 100).clone()
    w[0, 40], w[1, 99], w[2, 0], w[2, 70] = float("nan"), float("inf"), float("-inf"), float("nan")
    ref = R.quantize(w, fmt)
    out = ops.mx_fakequant(w.cuda(), fmt, want=("wq", "scales", "codes"))
    scales, wq, codes = out["scales"].cpu(), out["wq"].cpu(), out["codes"].cpu()
    assert torch.equal(scales, ref["scales"])
    bad = scales == 255
    assert bad.tolist() == [[False, True, False, False], [False, False, False, True], [True, False, True, False]]
    bad_el = bad.repeat_interleave(32, dim=1)[:, :100]
    assert bool(wq[bad_el].isnan().all()) and bool(ref["wq"][bad_el].isnan().all()) and not bool(wq[~bad_el].isnan().any())
    assert _same_bits(wq[~bad_el], ref["wq"][~bad_el]) and torch.equal(codes[~bad_el], ref["codes"][~bad_el])
    back = ops.mx_dequant(out["codes"], out["scales"], 100, fmt).cpu()
    assert bool(back[bad_el].isnan().all()) and _same_bits(back[~bad_el], wq[~bad_el])


def test_wrappers_refuse_on_the_device_what_they_refuse_on_the_host():
    from hipops import ops
    w = torch.zeros(3, 40, device="cuda")
    for args, kw, what in [((w, "mxfp5"), {}, "unknown MX format"), ((w, "mxfp4"), {"want": ()}, "want must hold at least one"),
                           ((w[:, ::2], "mxfp4"), {}, "contiguous"), ((w, "mxfp4"), {"wq_out": torch.zeros(3, 40)}, "wq_out must be")]:
        with pytest.raises(ValueError, match=f"mx_fakequant: .*{what}"):
            ops.mx_fakequant(*args, **kw)
    with pytest.raises(ValueError, match="mx_dequant: .*scales must be a contiguous uint8"):
        ops.mx_dequant(torch.zeros(3, 40, dtype=torch.uint8, device="cuda"), torch.zeros(3, 2, dtype=torch.uint8), 40, "mxfp4")


# ----------------------------------------------------------------------------- the quantiser
def _reference_weight(w, fmt, tconv=False):
    """the reference applied to to_rows of a weight, back in the weight's logical shape, on the CPU -> (wq, err sum, energy sum)"""
    from quantization.quantizer import from_rows, to_rows
    wr = to_rows(w.detach().cpu(), tconv)
    ref = R.quantize(wr.reshape(wr.shape[0], -1).contiguous(), fmt)
    return from_rows(ref["wq"].reshape(wr.shape), w, tconv).contiguous(), float(ref["err"].sum()), float(ref["energy"].sum())


@pytest.mark.parametrize("fmt", R.NAMES)
def test_quantiser_equals_the_reference_on_every_weight_layout(fmt):
    from quantization.mx import MXQuantizer
    torch.manual_seed(3)
    for shape, tconv in (((8, 5, 3, 3), False), ((5, 8, 3, 3), True), ((7, 40), False), ((40,), False)):
        w = (torch.distributions.StudentT(3.0).sample(shape) * 0.01).float().cuda()
        q = MXQuantizer(fmt, tconv=tconv)
        got = q(w)
        assert got.shape == w.shape and _same_bits(got.cpu().contiguous(), _reference_weight(w, fmt, tconv)[0]), (shape, tconv)
        err, energy = q.weight_cost(w)
        rows = 1 if len(shape) == 1 else 8 if len(shape) == 4 else 7
        assert err.shape == energy.shape == (rows,)
        assert q.size_bits(w) == R.size_bits(rows, w.numel() // rows, fmt)
    with pytest.raises(NotImplementedError, match="MX activations are not built"):
        q(w, True)


@pytest.fixture(scope="module")
def cheng():
    """the toy Cheng2020 (N = 8, four 64^2 images, every quantiser initialised at W8); every test leaves it as it found it"""
    return _cheng()


def _weighted(unit):
    from quantization import QuantModule
    return [m for m in unit.modules() if isinstance(m, QuantModule) and m.org_weight is not None]


@pytest.mark.parametrize("fmt", R.NAMES)
def test_module_in_quant_state_equals_the_fp_module_on_the_reference_weight(cheng, fmt):
    """both run the same kernels on the same weight bits"""
    from quantization.mx import MXQuantizer
    qnn, _ = cheng
    mods = _weighted(qnn)
    picked = [next(m for m in mods if m.kind == "conv" and m.weight[0].numel() % 32), next(m for m in mods if m.kind == "gdn")]
    torch.manual_seed(5)
    for m in picked:
        cin = m.weight.shape[1]
        x = torch.randn(2, cin, 8, 8, device="cuda")
        held = (m.weight_quantizer, m.org_weight, m.use_weight_quant, m.use_act_quant)
        try:
            m.weight_quantizer = MXQuantizer(fmt, tconv=m.if_tconv)
            m.set_quant_state(True, False)
            m.drop_weight_pack()
            with torch.no_grad():
                yq = m(x).contiguous().clone()
            m.set_quant_state(False, False)
            m.org_weight = _reference_weight(m.weight, fmt, m.if_tconv)[0].cuda()
            m.drop_weight_pack()
            with torch.no_grad():
                yf = m(x).contiguous().clone()
            assert torch.equal(m.bias.detach(), m.org_bias)
        finally:
            m.weight_quantizer, m.org_weight, m.use_weight_quant, m.use_act_quant = held
            m.drop_weight_pack()
        assert _same_bits(yq, yf), m.kind
        with torch.no_grad():
            m.set_quant_state(False, False)
            plain = m(x).contiguous().clone()
            m.use_weight_quant, m.use_act_quant = held[2:]
        assert not _same_bits(plain, yq) or fmt.startswith("mxfp8")                # the format shows in the output


# ----------------------------------------------------------------------------- the model
def _forward(qnn, x):
    with torch.no_grad():
        out = qnn(x)
    return [out["x_hat"].contiguous().clone()] + [v.contiguous().clone() for v in out["likelihoods"].values()]


def _quantisers(qnn):
    return [(id(m.weight_quantizer), type(m.weight_quantizer).__name__, "int_weight_quantizer" in m._modules) for m in _weighted(qnn)]


def test_set_weight_format_and_back(cheng, tmp_path):
    from quantization import block_reconstruction
    from quantization.export import integer_state
    from quantization.mx import MXQuantizer
    qnn, cali = cheng
    units = qnn.units()
    names = list(units)
    flags = [(m.use_weight_quant, m.use_act_quant) for m in qnn.modules() if hasattr(m, "use_weight_quant")]
    qnn.set_quant_state(True, False)
    try:
        before, out0 = _quantisers(qnn), _forward(qnn, cali[:2])
        qnn.set_weight_format("mxfp4")                                              # one name for every unit
        assert all(isinstance(m.weight_quantizer, MXQuantizer) and m.weight_quantizer.fmt == "mxfp4" for m in _weighted(qnn))
        out4 = _forward(qnn, cali[:2])
        assert not _same_bits(out4[0], out0[0])
        qnn.set_weight_format({names[0]: "mxfp8_e4m3", names[1]: "int"})            # a mapping; the other units keep theirs
        assert {m.weight_quantizer.fmt for m in _weighted(units[names[0]])} == {"mxfp8_e4m3"}
        assert not any(isinstance(m.weight_quantizer, MXQuantizer) for m in _weighted(units[names[1]]))
        assert all(m.weight_quantizer.fmt == "mxfp4" for n in names[2:] for m in _weighted(units[n]))
        # the forward is the fp model's on the reference weights: one unit checked end to end
        qnn.set_weight_format("int")
        qnn.set_weight_format({names[0]: "mxfp6_e2m3"})
        out6 = _forward(qnn, cali[:2])
        qnn.set_weight_format("int")
        held = [(m, m.org_weight) for m in _weighted(units[names[0]])]
        try:
            units[names[0]].set_quant_state(False, False)
            for m, _ in held:
                m.org_weight = _reference_weight(m.weight, "mxfp6_e2m3", m.if_tconv)[0].cuda()
                m.drop_weight_pack()
            assert all(torch.equal(m.bias.detach(), m.org_bias) for m, _ in held)
            by_hand = _forward(qnn, cali[:2])
        finally:
            for m, w0 in held:
                m.org_weight = w0
                m.drop_weight_pack()
            units[names[0]].set_quant_state(True, False)
        assert all(_same_bits(a, b) for a, b in zip(out6, by_hand))
        # 'int' has put the same objects back: the forward gives the bits it gave
        assert _quantisers(qnn) == before
        assert all(_same_bits(a, b) for a, b in zip(_forward(qnn, cali[:2]), out0))
        # a trained unit is refused and nothing is written
        last = _weighted(units[names[-1]])[-1]
        last.trained = True
        try:
            with pytest.raises(ValueError, match="set_weight_format: unit .* holds a trained module"):
                qnn.set_weight_format("mxfp4")
        finally:
            last.trained = False
        assert _quantisers(qnn) == before
        # where an MX quantiser cannot be served
        name = next(n for n in names if len(_weighted(units[n])) > 1)
        qnn.set_weight_format({name: "mxfp6_e3m2"})
        with pytest.raises(NotImplementedError, match="reconstruct: module .* holds an MXQuantizer \\(mxfp6_e3m2\\): learned rounding on MX grids"):
            block_reconstruction(qnn, units[name], name.split(".")[-1], cali, batch_size=2, iters=4)
        with pytest.raises(ValueError, match="integer_state: module .* holds an MXQuantizer"):
            integer_state(qnn)
        with pytest.raises(ValueError, match="save_packed: module .* holds an MXQuantizer .*a packed MX container is not built"):
            qnn.save_packed(os.path.join(tmp_path, "toy.rdopack"))
        assert os.listdir(tmp_path) == []
        assert set(qnn.weight_bits()[name]["bits"].values()) == {6}                 # element bits only
        qnn.set_weight_format("int")
        assert _quantisers(qnn) == before and len(integer_state(qnn)) == len(_weighted(qnn))
        assert all(_same_bits(a, b) for a, b in zip(_forward(qnn, cali[:2]), out0))
    finally:
        qnn.set_weight_format("int")
        for m, (w, a) in zip([m for m in qnn.modules() if hasattr(m, "use_weight_quant")], flags):
            m.use_weight_quant, m.use_act_quant = w, a


# ----------------------------------------------------------------------------- the report
REPORT_UNITS = ["g_a.0", "g_s.0"]
REPORT_FORMATS = ("mxfp4", "mxfp8_e4m3")


def test_format_report_on_the_toy_model(cheng, monkeypatch):
    qnn, cali = cheng
    images = cali[:2]
    units = qnn.units()
    before, state0 = _quantisers(qnn), [(m.use_weight_quant, m.use_act_quant) for m in qnn.modules() if hasattr(m, "use_weight_quant")]
    out0 = _forward(qnn, images)
    rep = qnn.format_report(images, formats=REPORT_FORMATS, lmbda=LMBDA, batch=2, units=REPORT_UNITS)
    assert list(rep) == ["fp", "units", "weights", "formats", "n", "pixels", "lmbda", "batch"]
    assert (rep["formats"], rep["n"], rep["pixels"], rep["lmbda"], rep["batch"]) == (list(REPORT_FORMATS), 2, 2 * 64 * 64, LMBDA, 2)
    assert list(rep["units"]) == list(rep["weights"]) == REPORT_UNITS
    rd = qnn.rd_report(images, lmbda=LMBDA, act_quant=False, batch=2, units=REPORT_UNITS)
    _same_report(rep["fp"], rd["fp"])
    extra = ["bits_per_weight", "size_bits", "weight_err", "weight_sqnr_db"]
    for name in REPORT_UNITS:
        ms = _weighted(units[name])
        count = sum(m.weight.numel() for m in ms)
        assert rep["weights"][name] == count > 0 and list(rep["units"][name]) == list(REPORT_FORMATS)
        for fmt in REPORT_FORMATS:
            row = rep["units"][name][fmt]
            assert sorted(set(row) - set(rd["units"][name])) == extra
            # sizes by hand from the shapes: rows are output channels (a GDN's gamma and a 1-D weight as stored)
            geometry = [(1 if m.weight.dim() == 1 else m.weight.shape[0], m.weight.numel() // (1 if m.weight.dim() == 1 else m.weight.shape[0]))
                        for m in ms]
            assert not any(m.if_tconv for m in ms)
            size = sum(R.size_bits(rows, inner, fmt) for rows, inner in geometry)
            assert row["size_bits"] == size and row["bits_per_weight"] == size / count
            assert row["bits_per_weight"] >= R.element_bits(fmt) + 0.25
            assert (row["bits_per_weight"] == R.element_bits(fmt) + 0.25) == all(inner % 32 == 0 for _, inner in geometry)
            refs = [_reference_weight(m.weight, fmt, m.if_tconv) for m in ms]
            err, energy = sum(r[1] for r in refs), sum(r[2] for r in refs)
            assert row["weight_err"] == pytest.approx(err, rel=1e-12, abs=0) and row["weight_err"] > 0
            assert row["weight_sqnr_db"] == pytest.approx(10.0 * torch.log10(torch.tensor(energy / err, dtype=torch.float64)).item(), rel=1e-12)
            assert row["d_loss"] == row["loss"] - rep["fp"]["loss"]
            print(name, fmt, "bits/weight", row["bits_per_weight"], "weight SQNR", round(row["weight_sqnr_db"], 2), "d_loss", row["d_loss"])
            # the row is rd_report's unit row of the model left in the format
            qnn.set_weight_format({name: fmt})
            try:
                want = qnn.rd_report(images, lmbda=LMBDA, act_quant=False, batch=2, units=[name])["units"][name]
            finally:
                qnn.set_weight_format("int")
            _same_report({k: row[k] for k in want}, dict(want))
        assert rep["units"][name]["mxfp4"]["weight_err"] > rep["units"][name]["mxfp8_e4m3"]["weight_err"]
    # the model is left exactly as found
    assert _quantisers(qnn) == before
    assert state0 == [(m.use_weight_quant, m.use_act_quant) for m in qnn.modules() if hasattr(m, "use_weight_quant")]
    assert all(_same_bits(a, b) for a, b in zip(_forward(qnn, images), out0))
    # a forward raises on the second state (one batch a state: call 2)
    u = units["g_a.1"]
    assert "g_a.1" not in REPORT_UNITS
    calls, real = [0], u.forward

    def failing(*a, **k):
        calls[0] += 1
        if calls[0] == 2:
            raise RuntimeError("planted failure")
        return real(*a, **k)
    monkeypatch.setattr(u, "forward", failing)
    with pytest.raises(RuntimeError, match="planted failure"):
        qnn.format_report(images, formats=REPORT_FORMATS, lmbda=LMBDA, batch=2, units=REPORT_UNITS)
    assert calls[0] == 2
    monkeypatch.undo()
    assert _quantisers(qnn) == before
    assert state0 == [(m.use_weight_quant, m.use_act_quant) for m in qnn.modules() if hasattr(m, "use_weight_quant")]
    assert all(m._pack_memo == {} for n in REPORT_UNITS for m in _weighted(units[n]))
    assert all(_same_bits(a, b) for a, b in zip(_forward(qnn, images), out0))
