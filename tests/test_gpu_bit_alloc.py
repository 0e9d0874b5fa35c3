"""Mixed-precision weight widths on the GPU: `ops.uaq_width_scan` (rdo_uaq_width_scan of csrc/bit_alloc.hip) against the kernels it stands
in for (`uaq_init_minmax`, `uaq_fakequant`) and against a torch-CPU restatement, in both modes, on rows that fit LDS and on split rows;
`QuantModel.bit_report` against `rd_report` (the width-8 row is the same bits), the state it leaves behind, a toy Lu2022 unit; the chain
bit_report -> allocate_bits -> set_weight_bits -> reconstruct -> integer_state -> pickle; two data-parallel ranks.

The allowed difference of the float64 sums is derived, nothing in it is measured: the kernel and the references add the SAME exact terms
((double)d * (double)d holds the 48-bit product of two fp32 values), all non-negative, in different orders.  Any order of a float64 sum
of n non-negative terms is within (n - 1) 2^-53 of the true sum S relatively (to first order), so two orders differ by at most
2 (n - 1) 2^-53 S < inner 2^-52 S per row.  Largest share of that bound the kernel used on an MI355X: 0.006, at (7, 257) (DESIGN.md
section 4)."""
import functools
import math
import os
import pickle
import socket
import sys
from collections import OrderedDict

import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_rd_report import LMBDA, _cheng, _lu2022, _plain, _same_report

pytestmark = pytest.mark.gpu

T = 8192                                                     # RDO_WIDTH_SCAN_LDS_ROW: the longest row one workgroup stages in LDS
SHAPES = [(1, 1), (3, 5), (7, 257), (5, 1600), (2, T + 3), (4, T + 3), (1, 921600)]
WIDTHS = [(2, 3, 4, 8, 16), (8,), (16, 12, 10, 8, 6, 5, 4, 2)]


@functools.lru_cache(maxsize=None)
def _rows(rows, inner):
    """seeded rows whose scales are spread over 2.5 decades; with three rows or more the last three are a row of zeros, an all-positive
    and an all-negative one; the two rows of a two-row matrix are all-positive and all-negative (left unchanged by every test)"""
    g = torch.Generator().manual_seed(1000 * rows + inner % 997)
    w = torch.randn(rows, inner, generator=g)
    scale = torch.pow(10.0, -2.5 * torch.arange(rows, dtype=torch.float32) / max(rows - 1, 1))
    w = w * scale[:, None]
    if rows >= 3:
        w[-3] = 0.0
        w[-2] = w[-2].abs() + 1e-3 * scale[-2]
        w[-1] = -w[-1].abs() - 1e-3 * scale[-1]
    elif rows == 2:
        w[0] = w[0].abs()
        w[1] = -w[1].abs()
    return w.contiguous(), w.cuda().contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _references(wc, wg, width, d, z):
    """float64 [rows] sums of (w - wq)^2 for wq (a) from the existing kernel `ops.uaq_fakequant`, w - wq in fp32 on the device, (b) from a
    torch-CPU restatement of the quantiser's expression -- on the grid (d, z) fp32 [rows] -- and the energy"""
    from hipops import ops
    desc = ops.ada_desc(wg, 2 ** width, conv_layout=False)
    wq = ops.uaq_fakequant(desc, wg, d.contiguous(), z.contiguous())
    by_kernel = ((wg - wq).double() ** 2).sum(1).cpu()
    dc, zc = d.cpu()[:, None], z.cpu()[:, None]
    xq = (torch.clamp(torch.round(wc / dc) + zc, 0, 2 ** width - 1) - zc) * dc
    by_torch = ((wc - xq).double() ** 2).sum(1)
    return by_kernel, by_torch, (wc.double() ** 2).sum(1)


def _within(got, ref, inner, what):
    bound = inner * 2.0 ** -52 * ref
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest share of the derived bound {worst:.3f}")
    assert bool(((got - ref).abs() <= bound).all()), what


@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("rows,inner", SHAPES)
def test_scan_matches_the_kernels_it_stands_in_for(rows, inner, widths):
    from hipops import ops
    wc, wg = _rows(rows, inner)
    K = len(widths)
    d, z, err, energy = ops.uaq_width_scan(wg, widths)
    assert d.shape == z.shape == err.shape == (K, rows) and energy.shape == (rows,)
    assert d.dtype == z.dtype == torch.float32 and err.dtype == energy.dtype == torch.float64 and err.is_cuda
    err_c, en_c = err.cpu(), energy.cpu()
    for k, b in enumerate(widths):
        d0, z0 = ops.uaq_init_minmax(wg, 2 ** b)
        assert _same_bits(d[k], d0) and _same_bits(z[k], z0), b                    # the grids of the min-max init, bit for bit
        by_kernel, by_torch, en = _references(wc, wg, b, d[k], z[k])
        _within(err_c[k], by_kernel, inner, f"min-max {(rows, inner)} width {b} against uaq_fakequant")
        _within(err_c[k], by_torch, inner, f"min-max {(rows, inner)} width {b} against torch on the CPU")
        if k == 0:
            _within(en_c, en, inner, f"energy {(rows, inner)}")
    if rows >= 3:
        assert bool((err_c[:, -3] == 0).all()) and float(en_c[-3]) == 0.0           # the row of zeros
        assert inner < 257 or bool((err_c[:, [-2, -1]] > 0).all())
    if len(widths) > 1 and inner >= 257:                                            # a finer grid costs less, here by far
        order = sorted(range(K), key=lambda k: widths[k])
        live = en_c > 0
        assert bool((err_c[order[0]][live] > err_c[order[-1]][live]).all())
    # the same bits again, also behind a poisoned workspace
    assert ops._workspaces("uaq_width_scan")
    for ws in ops._workspaces("uaq_width_scan"):
        ws.fill_(float("nan"))
    again = ops.uaq_width_scan(wg, widths)
    torch.cuda.synchronize()
    assert all(_same_bits(a, b_) for a, b_ in zip((d, z, err, energy), again))
    # given mode: other grids are copied through bit for bit and scored; the min-max grids given back score to the same bits
    dg, zg = (d * 1.37).contiguous(), (z + 1.0).contiguous()
    d2, z2, err2, en2 = ops.uaq_width_scan(wg, widths, dg, zg)
    assert _same_bits(d2, dg) and _same_bits(z2, zg) and _same_bits(en2, energy)
    assert d2.data_ptr() != dg.data_ptr()
    err2_c = err2.cpu()
    for k, b in enumerate(widths):
        by_kernel, by_torch, _ = _references(wc, wg, b, dg[k], zg[k])
        _within(err2_c[k], by_kernel, inner, f"given {(rows, inner)} width {b} against uaq_fakequant")
        _within(err2_c[k], by_torch, inner, f"given {(rows, inner)} width {b} against torch on the CPU")
    d3, z3, err3, en3 = ops.uaq_width_scan(wg, widths, d, z)
    assert all(_same_bits(a, b_) for a, b_ in zip((d, z, err, energy), (d3, z3, err3, en3)))


def test_scan_refuses_on_the_device_what_it_refuses_on_the_host():
    from hipops import ops
    w = torch.zeros(3, 40, device="cuda")
    for args, kw, what in [((w, (4, 4)), {}, "distinct"), ((w, (4, 17)), {}, "whole number in 2 .. 16"),
                           ((w, (4, 8)), {"delta": torch.zeros(2, 3, device="cuda")}, "given together"),
                           ((w, (4, 8)), {"delta": torch.zeros(2, 3), "zp": torch.zeros(2, 3, device="cuda")}, "delta must be a contiguous fp32"),
                           ((w[:, ::2], (4, 8)), {}, "contiguous")]:
        with pytest.raises(ValueError, match=f"uaq_width_scan: .*{what}"):
            ops.uaq_width_scan(*args, **kw)


# ----------------------------------------------------------------------------- bit_report on the toy Cheng2020
CHENG_UNITS = ["g_a.0", "g_a.6", "g_s.0"]


def _weighted(unit):
    from quantization import QuantModule
    return [m for m in unit.modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def _check_against_rd_report(qnn, cali, names, widths, batch, by_parameters=True):
    """the report of `widths` (8 among them) on `names` -> it; every column the width-8 row shares with rd_report's unit row is the same
    bits (same grids, same kernels), sizes and counts are as counted by hand, the weight columns are a hand sum of the scan"""
    from hipops import ops
    units = qnn.units()
    # what the first weighted module of every chosen unit stands at in each forward of the report
    seen = {name: [] for name in names}
    hooks = []
    for name in names:
        m = _weighted(units[name])[0]
        hooks.append(units[name].register_forward_pre_hook(lambda unit, inp, name=name, m=m: seen[name].append(
            (m.use_weight_quant, m.weight_quantizer.n_bits, m.weight_quantizer.n_levels, m.weight_quantizer.inited))))
    try:
        rep = qnn.bit_report(cali, widths=widths, lmbda=LMBDA, batch=batch, units=names)
    finally:
        for h in hooks:
            h.remove()
    nb = -(-cali.shape[0] // batch)
    order = [u for u in units if u in names]
    for name in names:
        got = seen[name]
        assert len(got) == nb * (1 + len(order) * len(widths)) and not any(g[0] for g in got[:nb])
        states = [(u, b) for u in order for b in widths]
        for i, (u, b) in enumerate(states):
            part = got[nb * (1 + i):nb * (2 + i)]
            assert all(g == (True, b, 2 ** b, True) for g in part) if u == name else not any(g[0] for g in part), (name, u, b)
    rd = qnn.rd_report(cali, lmbda=LMBDA, act_quant=False, batch=batch, units=names)
    n, _, H, W = cali.shape
    assert list(rep) == ["fp", "units", "weights", "widths", "n", "pixels", "lmbda", "batch"]
    assert (rep["widths"], rep["n"], rep["pixels"], rep["lmbda"], rep["batch"]) == (list(widths), n, n * H * W, LMBDA, batch)
    assert list(rep["units"]) == list(rep["weights"]) == [u for u in units if u in names]
    _same_report(rep["fp"], rd["fp"])
    for name in names:
        table, want = rep["units"][name], rd["units"][name]
        assert list(table) == list(widths)
        shared = OrderedDict((k, table[8][k]) for k in want)
        _same_report(shared, want)                                                  # rel = 0: the same bits
        assert sorted(set(table[8]) - set(want)) == ["size_bits", "weight_err", "weight_sqnr_db"]
        # by hand: the weights of the unit are the parameters named 'weight' of its QuantModules (a GDN's gamma is one)
        count = sum(math.prod(m.weight.shape) for m in _weighted(units[name]))
        if by_parameters:
            assert count == sum(p.numel() for pn, p in units[name].named_parameters() if pn.split(".")[-1] == "weight")
        assert rep["weights"][name] == count > 0
        err, energy, terms = [0.0] * len(widths), 0.0, 0
        for m in _weighted(units[name]):
            wr = m.weight_quantizer._rows(m.weight.detach())
            _, _, e, en = ops.uaq_width_scan(wr.reshape(wr.shape[0], -1), widths)
            for k in range(len(widths)):
                err[k] += sum(float(v) for v in e[k].cpu())
            energy += sum(float(v) for v in en.cpu())
            terms += wr.shape[0]
        for k, b in enumerate(widths):
            row = table[b]
            assert row["size_bits"] == b * count
            assert abs(row["weight_err"] - err[k]) <= terms * 2.0 ** -52 * err[k] and row["weight_err"] > 0
            assert row["weight_sqnr_db"] == pytest.approx(10.0 * math.log10(energy / err[k]), rel=1e-12)
            assert all(f in row for f in ("bits", "bits_total", "sse", "bpp", "mse", "psnr_db", "loss", "d_bits", "d_loss"))
            assert row["d_loss"] == row["loss"] - rep["fp"]["loss"] and math.isfinite(row["d_loss"])
        lo, hi = min(widths), max(widths)
        assert table[lo]["weight_err"] > table[hi]["weight_err"] and table[lo]["weight_sqnr_db"] < table[hi]["weight_sqnr_db"]
        if name.startswith("g_s"):           # behind the latents' rounding the width shows in x_hat (in front of it the rounding may absorb it)
            assert table[lo]["sse"] != table[hi]["sse"]
    return rep


@pytest.fixture(scope="module")
def cheng_table():
    """the toy Cheng2020 (N = 8, four 64^2 images, every quantiser initialised at W8) and its table at widths (3, 8) on three units"""
    qnn, cali = _cheng()
    rep = _check_against_rd_report(qnn, cali, CHENG_UNITS, (3, 8), 2)
    return qnn, cali, rep


def test_width_8_row_is_the_rd_report_row_on_toy_cheng2020(cheng_table):
    qnn, cali, rep = cheng_table
    for name, table in rep["units"].items():
        print(name, {b: (round(r["weight_sqnr_db"], 2), r["d_loss"]) for b, r in table.items()})
    assert all(n in qnn.units() for n in CHENG_UNITS)


def _snapshot(qnn):
    from quantization import BaseQuantBlock, QuantModule
    out = []
    for name, m in qnn.named_modules():
        if not isinstance(m, (QuantModule, BaseQuantBlock)):
            continue
        row = {"name": name, "flags": (m.use_weight_quant, m.use_act_quant, m.trained)}
        if isinstance(m, QuantModule) and m.org_weight is not None:
            q = m.weight_quantizer
            row.update(q=id(q), n_bits=q.n_bits, n_levels=q.n_levels, inited=q.inited, delta_id=id(q.delta), zp_id=id(q.zero_point),
                       delta=None if q.delta is None else q.delta.clone(), zp=None if q.zero_point is None else q.zero_point.clone(),
                       wstate=m._weight_state())
        out.append(row)
    return out


def _same_snapshot(x, y):
    assert len(x) == len(y) > 0
    for r, s in zip(x, y):
        assert sorted(r) == sorted(s)
        for k in r:
            if torch.is_tensor(r[k]):
                assert torch.is_tensor(s[k]) and _same_bits(r[k], s[k]), (r["name"], k)
            else:
                assert r[k] == s[k], (r["name"], k)


def test_the_model_is_left_as_it_was_found(monkeypatch):
    qnn, cali = _cheng()
    units = qnn.units()
    qnn.set_quant_state(False, False)
    for k, u in enumerate(units.values()):                                          # mixed flags
        u.set_quant_state(k % 2 == 0, k % 3 == 0)
    units["g_s.0"].set_quant_state(False, True)
    cold = _weighted(units["g_s.0"])[0].weight_quantizer                            # a quantiser that has never run
    cold.inited, cold.delta, cold.zero_point = False, None, None
    units["g_a.0"].set_quant_state(True, False)
    units["g_a.6"].set_quant_state(True, False)
    for m in _weighted(units["g_a.6"]):                                             # a unit that stands at another width
        m.weight_quantizer.bitwidth_refactor(6)
        m.weight_quantizer.inited = False
    before = _snapshot(qnn)
    assert {r["flags"][:2] for r in before} >= {(True, False), (False, True), (False, False)}
    with torch.no_grad():
        out0 = qnn(cali[:2])
    before = _snapshot(qnn)                                                         # (g_a.6 has initialised its 6-bit scale now)
    assert not cold.inited and any(r.get("n_bits") == 6 and r["inited"] for r in before)
    qnn.bit_report(cali, widths=(3, 8), lmbda=LMBDA, batch=2, units=CHENG_UNITS)
    _same_snapshot(before, _snapshot(qnn))
    with torch.no_grad():
        out1 = qnn(cali[:2])
    assert _same_bits(out0["x_hat"], out1["x_hat"]) and all(_same_bits(out0["likelihoods"][k], out1["likelihoods"][k]) for k in out0["likelihoods"])
    _same_snapshot(before, _snapshot(qnn))
    # the forward raises half-way: the first batch of the third state (the two batches of 'fp' and of (g_a.0, 3) are calls 1 .. 4)
    u = units["g_a.1"]
    assert "g_a.1" not in CHENG_UNITS and CHENG_UNITS[0] == "g_a.0"
    calls, real = [0], u.forward

    def failing(*a, **k):
        calls[0] += 1
        if calls[0] == 5:
            raise RuntimeError("planted failure")
        return real(*a, **k)
    monkeypatch.setattr(u, "forward", failing)
    with pytest.raises(RuntimeError, match="planted failure"):
        qnn.bit_report(cali, widths=(3, 8), lmbda=LMBDA, batch=2, units=CHENG_UNITS)
    assert calls[0] == 5
    monkeypatch.undo()
    _same_snapshot(before, _snapshot(qnn))
    with torch.no_grad():
        out2 = qnn(cali[:2])
    assert _same_bits(out0["x_hat"], out2["x_hat"])


def test_other_scale_methods_go_through_the_scan_in_given_mode():
    """a symmetric 'max' quantiser and an 'mse' one: their own `init_quantization_scale` after `bitwidth_refactor(b)` gives the grids,
    the width-8 row is still rd_report's, and the quantisers are put back as found"""
    qnn, cali = _cheng()
    name = "g_a.6"
    m, = _weighted(qnn.units()[name])
    rows = {}
    for sym, method in ((True, "max"), (False, "mse")):
        q = m.weight_quantizer
        q.sym, q.scale_method, q.inited, q.delta, q.zero_point = sym, method, False, None, None
        m.drop_weight_pack()
        rep = qnn.bit_report(cali, widths=(4, 8), lmbda=LMBDA, batch=2, units=[name])
        assert (q.n_bits, q.n_levels, q.inited, q.delta, q.zero_point) == (8, 256, False, None, None)
        rd = qnn.rd_report(cali, lmbda=LMBDA, act_quant=False, batch=2, units=[name])   # (initialises the scale its own way)
        assert q.inited
        _same_report(OrderedDict((k, rep["units"][name][8][k]) for k in rd["units"][name]), rd["units"][name])
        rows[method] = rep["units"][name]
    assert rows["max"][4]["weight_err"] != rows["mse"][4]["weight_err"]


def test_one_unit_of_toy_lu2022_with_linear_and_layernorm_weights():
    qnn, cali = _lu2022()
    name = "g_a1"
    kinds = {m.kind for m in _weighted(qnn.units()[name])}
    assert {"linear", "layernorm"} <= kinds
    before = _snapshot(qnn)
    _check_against_rd_report(qnn, cali, [name], (4, 8), 2, by_parameters=False)
    _same_snapshot(before, _snapshot(qnn))


# ----------------------------------------------------------------------------- end to end
def test_allocation_is_applied_calibrated_exported_and_pickled(cheng_table):
    from test_gpu_unit_report import _toy
    from quantization import BaseQuantBlock, block_reconstruction, layer_reconstruction
    from quantization.export import allocate_bits, dequantize, integer_state
    _, _, rep = cheng_table
    alloc = allocate_bits(rep, avg_bits=5.5)
    total_w = sum(rep["weights"].values())
    assert alloc["budget_bits"] == math.floor(5.5 * total_w) and alloc["size_bits"] <= alloc["budget_bits"]
    assert set(alloc["bits"].values()) <= {3, 8} and 3 in alloc["bits"].values()
    assert alloc["size_bits"] == sum(alloc["bits"][n] * rep["weights"][n] for n in rep["weights"])
    qnn, cali, _, kwargs = _toy()                                                   # a fresh model: the table's one stays as it is
    qnn.set_weight_bits(alloc["bits"])
    units = qnn.units()
    got = qnn.weight_bits()
    for n, b in alloc["bits"].items():
        assert set(got[n]["bits"].values()) == {b} and got[n]["weights"] == rep["weights"][n] and got[n]["size_bits"] == b * rep["weights"][n]
    others = sum(got[n]["weights"] for n in units if n not in alloc["bits"])
    assert got["total"]["size_bits"] == alloc["size_bits"] + 8 * others and got["total"]["weights"] == total_w + others
    assert got["total"]["avg_bits"] == got["total"]["size_bits"] / got["total"]["weights"]
    name = next(n for n, b in alloc["bits"].items() if b < 8)
    u, b = units[name], alloc["bits"][name]
    torch.manual_seed(1005)
    (block_reconstruction if isinstance(u, BaseQuantBlock) else layer_reconstruction)(qnn, u, name.split(".")[-1], **kwargs)
    assert kwargs["iters"] == 20
    mods = dict(qnn.named_modules())
    state = integer_state(qnn)
    mine = ["model." + name + ("." + mn if mn else "") for mn in got[name]["bits"]]
    assert mine and all(k in state for k in mine)
    for key in mine:
        entry, m = state[key], mods[key]
        assert m.trained and entry["n_bits"] == b and entry["levels"].dtype == torch.uint8
        assert 0 <= int(entry["levels"].min()) and int(entry["levels"].max()) <= 2 ** b - 1
        m.set_quant_state(True, False)
        used = m.weight_quantizer(m.weight).detach().cpu()                          # the hard-rounded weight the module uses
        assert _same_bits(dequantize(entry).reshape(used.shape).contiguous(), used.contiguous()), key
    for key, entry in state.items():                                                # every other module: round to nearest at its own width
        if key not in mine:
            assert int(entry["levels"].max()) <= 2 ** entry["n_bits"] - 1
    assert qnn.weight_bits() == got                                                 # calibration does not move a width
    with pytest.raises(ValueError, match=f"set_weight_bits: unit '{name}' holds a trained module"):
        qnn.set_weight_bits({name: 8})
    back = pickle.loads(pickle.dumps(qnn))
    assert back.weight_bits() == got


# ----------------------------------------------------------------------------- two ranks on one GPU
DP_UNITS = ["g_a.0", "g_s.7.0"]


def _dp_rank(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "rdo-ptq_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        qnn, cali = _cheng()
        rep = qnn.bit_report(cali[:3], widths=(3, 8), lmbda=LMBDA, batch=1, units=DP_UNITS)
        out_q.put((rank, _plain(rep)))
        dist.barrier()
    except BaseException as e:          # the parent must not wait out its queue timeout for a rank that failed
        out_q.put(("error", f"rank {rank}: {e!r}"))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_return_the_table_of_one():
    """Two processes on cuda:0 over gloo on three images (rank 0: images 0 and 2, rank 1: image 1), batch 1: both return the same table,
    'n' and 'pixels' are global, and the sums are the single process's to 1e-12 relative (the per-image fp32 values are the same; only
    the float64 addition order differs); the weight columns do not depend on the images and are the same bits"""
    qnn, cali = _cheng()
    want = qnn.bit_report(cali[:3], widths=(3, 8), lmbda=LMBDA, batch=1, units=DP_UNITS)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(2):
            rk, val = q.get(timeout=180)
            assert rk != "error", val
            got[rk] = _plain(val, back=True)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    _same_report(got[0], got[1])
    assert got[0]["n"] == 3 and got[0]["pixels"] == 3 * 64 * 64 and got[0]["batch"] == 1 and got[0]["widths"] == [3, 8]
    _same_report(got[0]["fp"], want["fp"], rel=1e-12)
    assert got[0]["weights"] == want["weights"] and list(got[0]["units"]) == DP_UNITS
    for name in DP_UNITS:
        for b in (3, 8):
            _same_report(got[0]["units"][name][b], want["units"][name][b], rel=1e-12)
            row = got[0]["units"][name][b]
            assert row["bits_total"] == pytest.approx(float(sum(v.sum() for v in row["bits"].values())), rel=1e-12)
            for f in ("size_bits", "weight_err", "weight_sqnr_db"):
                assert got[0]["units"][name][b][f] == want["units"][name][b][f]
