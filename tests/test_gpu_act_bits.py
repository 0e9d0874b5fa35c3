"""Activation widths per unit on the GPU: `ops.actquant_width_scan` (rdo_actquant_width_scan of csrc/actquant.hip) against the restatement
of tests/act_width_reference.py and against the quantisers it stands in for (`actquant_static`, `actquant_perchannel`); the quantiser
hook `act_scan`; `QuantModel.act_bit_report` against passes done by hand and hand sums of the scan, the state it leaves behind;
`act_width_report` against hand sums of one pass and against `act_report`; the chain act_bit_report -> allocate_act_bits ->
set_act_bits -> reconstruct -> activation_state -> pickle -> save_packed -> load_packed; a Swin unit of the toy Lu2022; two data-parallel
ranks.

The bound of the kernel checks is derived, not measured: the kernel and the restatement add the same non-negative fp32 terms, the kernel
in fp32 in serial chains of at most 1024 terms plus the folds' trees, the restatement in float64: (1024 + 20) * 2^-24 = 6.2e-5 < 1e-4
relative, the bar of the score kernel's test (the same skeleton).  Largest relative error measured on an MI355X: 5.7e-7, on the long
chain (3.5e-7 on the shapes of the list)."""
import math
import os
import pickle
import socket
import sys
from collections import OrderedDict

import pytest
import torch
import torch.multiprocessing as mp

from act_width_reference import rel_err, width_scan_ref
from test_gpu_actquant_auto import _heavy, _unaligned
from test_gpu_rd_report import LMBDA, _cheng, _lu2022, _mark_trained, _plain, _same_report

pytestmark = pytest.mark.gpu

SHAPES = [(16384, 192), (35, 1280), (561, 3), (1, 6), (300000, 1)]
WIDTHS = [(8,), (2, 3, 4, 6, 8, 10, 12, 16)]
RDO_EINVAL = -22


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _clipping_range(x):
    """one grid per channel that cuts different shares off the two ends of the observed range"""
    lo, hi = x.amin(0), x.amax(0)
    w = hi - lo
    return torch.cat([lo + 0.1 * w, hi - 0.3 * w]).float().contiguous()


def _raw_scan(x, rng, widths, energy=True):
    """the C entry itself, on a workspace of its own -> (rc, err [C, K], energy [C] or None)"""
    import ctypes as C
    from hipops import _lib as L
    from hipops import ops
    Cc, K = x.shape[-1], len(widths)
    ws = torch.full((max(int(L.lib().rdo_actquant_width_scan_workspace(Cc, K)), 1),), float("nan"), device="cuda")
    err = torch.full((Cc, K), float("nan"), device="cuda")
    en = torch.full((Cc,), float("nan"), device="cuda") if energy else None
    rc = L.lib().rdo_actquant_width_scan(ops._ptr(x), x.numel() // Cc, Cc, ops._ptr(rng), (C.c_int32 * max(K, 1))(*widths), K, ops._ptr(err),
                                         ops._ptr(en), ops._ptr(ws), ops._stream())
    return rc, err, en


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("widths", WIDTHS)
@pytest.mark.parametrize("npix,C", SHAPES)
def test_scan_matches_the_restatement(npix, C, widths):
    """err and energy within 1e-4 relative of the restatement; the same bits from a second launch behind a poisoned workspace; the same
    err with energy null; behind an unaligned base pointer (4-byte accesses); at K = 1 the error of `ops.actquant_static` itself; on the
    tensor's own min | max the error of `ops.actquant_perchannel`'s output at every width (what lets one kernel serve both modes)."""
    from hipops import ops
    x = _heavy(npix, C)
    rng = _clipping_range(x)
    K = len(widths)
    ref_err, ref_energy = width_scan_ref(x, rng, widths)
    if npix > 1:                                                                    # (the range does clip, at both ends)
        assert bool((x < rng[:C]).any()) and bool((x > rng[C:]).any())
    xc, rc = x.cuda(), rng.cuda()
    err, energy = ops.actquant_width_scan(xc, rc, widths)
    assert err.shape == (C, K) and energy.shape == (C,) and err.dtype == energy.dtype == torch.float32 and err.is_cuda
    worst = max(rel_err(err.cpu().double(), ref_err), rel_err(energy.cpu().double(), ref_energy))
    print(f"width scan npix={npix} C={C} widths={widths}: largest relative error {worst:.3e}")
    assert worst <= 1e-4
    if K > 1 and npix > 1:                                                          # a finer grid on the same range costs less
        order = sorted(range(K), key=lambda k: widths[k])
        total = ref_err.sum(0)
        assert all(float(total[a]) > float(total[b]) for a, b in zip(order, order[1:]))
    # outputs are written, not added to; a fixed reduction order: the same bits again, also behind a poisoned workspace
    assert ops._workspaces("actquant_width_scan")
    for ws in ops._workspaces("actquant_width_scan"):
        ws.fill_(float("nan"))
    err2, energy2 = ops.actquant_width_scan(xc, rc, widths)
    assert _same_bits(err, err2) and _same_bits(energy, energy2)
    code, err3, energy3 = _raw_scan(xc, rc, widths)
    assert code == 0 and _same_bits(err, err3) and _same_bits(energy, energy3)
    code, err4, none = _raw_scan(xc, rc, widths, energy=False)                      # the nullable output does not change err
    assert code == 0 and none is None and _same_bits(err, err4)
    # an unaligned base pointer
    xu = _unaligned(xc)
    err5, energy5 = ops.actquant_width_scan(xu, rc, widths)
    assert max(rel_err(err5.cpu().double(), ref_err), rel_err(energy5.cpu().double(), ref_energy)) <= 1e-4
    if C % 4:
        assert _same_bits(err, err5) and _same_bits(energy, energy5)               # (one channel per thread either way)
    if K == 1:
        y = ops.actquant_static(xc, rc, n_bits=widths[0])
        same = ((xc - y).double() ** 2).sum(0).cpu()
        assert rel_err(err[:, 0].cpu().double(), same) <= 1e-4
    # the dynamic claim: on the tensor's own min | max, the grid of the dynamic quantiser
    own = torch.cat([xc.amin(0), xc.amax(0)]).contiguous()
    err_own, _ = ops.actquant_width_scan(xc, own, widths)
    for k, b in enumerate(widths):
        y = ops.actquant_perchannel(xc, n_bits=b)
        assert _same_bits(y, ops.actquant_static(xc, own, n_bits=b))
        same = ((xc - y).double() ** 2).sum(0).cpu()
        assert rel_err(err_own[:, k].cpu().double(), same) <= 1e-4, b


def test_long_chains_are_closed():
    """More than 1024 pixels per thread (one channel: all 256 lanes of all 256 workgroups walk the pixels, 1100 each): the running sums
    are closed every 1024 terms.  The restatement is evaluated by torch on the device (288 MB in fp32 and its temporaries)."""
    from hipops import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    npix = 256 * 256 * 1100
    x = (torch.rand(npix, 1, generator=g, device="cuda") ** 2).contiguous()
    rng = torch.tensor([0.09, 0.81], device="cuda")
    widths = (4, 8, 12)
    ref_err, ref_energy = width_scan_ref(x, rng, widths)
    err, energy = ops.actquant_width_scan(x, rng, widths)
    worst = max(rel_err(err.cpu().double(), ref_err), rel_err(energy.cpu().double(), ref_energy))
    print(f"width scan {npix} x 1: largest relative error {worst:.3e}")
    assert worst <= 1e-4


def test_scan_refuses_on_the_device_what_it_refuses_on_the_host():
    from hipops import _lib as L
    from hipops import ops
    x, r = torch.zeros(35, 6, device="cuda"), torch.zeros(12, device="cuda")
    for args, what in [((x, r, (4, 4)), "distinct"), ((x, r, (4, 17)), "whole number in 2 .. 16"), ((x, r, ()), "1 .. 8 entries"),
                       ((x, r, tuple(range(2, 11))), "1 .. 8 entries"), ((x[:, ::2], r, (4, 8)), "contiguous"),
                       ((x, r.cpu(), (4, 8)), "rng must be a contiguous fp32 \\[12\\] on cuda:0"),
                       ((x, torch.zeros(10, device="cuda"), (4, 8)), "rng must be a contiguous fp32 \\[12\\]"),
                       ((x.double(), r, (4, 8)), "x must be an fp32 tensor"), ((x.cpu(), r.cpu(), (4, 8)), "no CPU path")]:
        with pytest.raises(ValueError, match=f"actquant_width_scan: .*{what}"):
            ops.actquant_width_scan(*args)
    # the C entry, on device pointers: refused before any launch (the outputs keep their NaNs)
    for widths in ((4, 4), (4, 17), (1,), tuple(range(2, 11)), ()):
        code, err, en = _raw_scan(x, r, widths)
        torch.cuda.synchronize()
        assert code == RDO_EINVAL and b"rdo_actquant_width_scan" in L.lib().rdo_last_error()
        assert bool(torch.isnan(err).all()) and bool(torch.isnan(en).all())


# ----------------------------------------------------------------------------- the hook
@pytest.mark.parametrize("mode", ["dynamic", "static"])
def test_hook_adds_the_scan_and_returns_the_same_bits(mode):
    """three sites of one quantiser (NCHW, tokens, channels-last probabilities), two calls each: with a scan open the outputs are the same
    bits, and the closed sums are a hand sum of `ops.actquant_width_scan` over the same inputs on the grid each call quantises on"""
    from hipops import ops
    from quantization.quantizer import UniformAffineQuantizer, _act_rows
    g = torch.Generator().manual_seed(3)
    widths = (3, 6, 11)
    sites = {0: ((2, 6, 5, 7), False), 1: ((3, 11, 8), False), 2: ((2, 4, 4, 3), True)}
    calls = [(s, (torch.randn(shape, generator=g) ** 3).cuda(), cl) for _ in range(2) for s, (shape, cl) in sites.items()]
    q = UniformAffineQuantizer(act=True, dynamic_bits=6, act_mode=mode)
    if mode == "static":
        with pytest.raises(RuntimeError, match="act_scan: the static quantiser is not frozen"):
            q.act_scan(widths)
        q.act_observe()
        for s, x, cl in calls:
            q(x, True, site=s, channels_last=cl)
        q.act_freeze()
        q.act_range = {s: (r * 0.6).contiguous() for s, r in q.act_range.items()}    # (so that values are clipped)
        assert q.act_frozen()
    plain = [q(x, True, site=s, channels_last=cl) for s, x, cl in calls]
    q.act_scan(widths)
    scanned = [q(x, True, site=s, channels_last=cl) for s, x, cl in calls]
    sums = q.act_scan_close()
    assert all(_same_bits(a, b) and a.shape == x.shape for a, b, (_, x, _) in zip(plain, scanned, calls))
    assert sorted(sums) == [0, 1, 2] and q.act_scan_widths is None and q.act_scan_sums == {} and q.dynamic_bits == 6
    for s, (shape, cl) in sites.items():
        C = shape[-1] if (cl or len(shape) == 3) else shape[1]
        err = torch.zeros(len(widths), C, dtype=torch.float64, device="cuda")
        energy, n = torch.zeros(C, dtype=torch.float64, device="cuda"), 0
        for s2, x, _ in calls:
            if s2 != s:
                continue
            xr, _ = _act_rows(x, cl)
            flat = xr.reshape(-1, C)
            rng = q.act_range[s] if mode == "static" else torch.cat([flat.amin(0), flat.amax(0)]).contiguous()
            e, en = ops.actquant_width_scan(xr, rng, widths)
            err += e.t().double()
            energy += en.double()
            n += flat.shape[0]
        got = sums[s]
        assert got["err"].dtype == torch.float64 and got["err"].is_cuda and got["n"] == n
        assert torch.equal(got["err"], err) and torch.equal(got["energy"], energy) and float(err.sum()) > 0
    # closed: a further call adds nothing
    assert _same_bits(q(calls[0][1], True, site=0), plain[0]) and q.act_scan_close() == {}


# ----------------------------------------------------------------------------- act_bit_report on the toy Cheng2020
CHENG_UNITS = ["g_a.0", "g_a.6", "g_s.0"]


def _calibrated(**extra):
    """the toy Cheng2020 of the activation-quantiser tests (N = 8, four 64^2 images), the three units calibrated W8A8 for 6 iterations"""
    from test_gpu_actquant_hist_mse import _toy
    from quantization import BaseQuantBlock, block_reconstruction, layer_reconstruction
    qnn, cali, _, kwargs, _, _ = _toy(**extra)
    assert kwargs["iters"] == 6 and kwargs["act_quant"] is True
    units = qnn.units()
    for k, name in enumerate(CHENG_UNITS):
        u = units[name]
        torch.manual_seed(1005 + k)
        (block_reconstruction if isinstance(u, BaseQuantBlock) else layer_reconstruction)(qnn, u, name.split(".")[-1], **kwargs)
        assert u.trained
    qnn.eval()
    qnn.set_quant_state(True, True)
    return qnn, cali, kwargs


@pytest.fixture(scope="module")
def dynamic_model():
    qnn, cali, _ = _calibrated()
    return qnn, cali


@pytest.fixture(scope="module")
def static_model():
    qnn, cali, _ = _calibrated(act_mode="static", act_range="max", act_report=True)
    assert qnn.units()["g_a.6"].act_quantizer.act_frozen() and len(qnn.act_ranges()) >= 6
    return qnn, cali


def _applied(root, prefix=""):
    """(name, quantiser) of every activation quantiser under `root` that a forward with act_quant=True applies, by the rule itself"""
    from quantization import BaseQuantBlock, QuantModule
    out, seen = [], set()
    for n, m in root.named_modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)) and m.trained and not getattr(m, "disable_act_quant", False) \
                and id(m.act_quantizer) not in seen:
            seen.add(id(m.act_quantizer))
            out.append((f"{prefix}{n}{'.' if n else ''}act_quantizer", m.act_quantizer))
    return out


class _Tap:
    """forward pre-hooks on quantisers: every call's (name, dynamic_bits, scan widths, input, site, channels_last), in call order"""

    def __init__(self, named):
        self.calls = []
        self.hooks = [q.register_forward_pre_hook(lambda mod, args, kwargs, name=name: self.calls.append(
            (name, mod.dynamic_bits, getattr(mod, "act_scan_widths", None), args[0].detach().clone(), kwargs.get("site", 0),
             kwargs.get("channels_last", False))), with_kwargs=True) for name, q in named]

    def remove(self):
        for h in self.hooks:
            h.remove()


def _hand_scan(quants, calls, widths):
    """what the hooks of `quants` (name -> quantiser) add over `calls`, by hand: site name -> (err float64 [K, C], energy float64 [C], n),
    each call scanned by `ops.actquant_width_scan` on the grid it quantises on; in order of the quantisers, then of the sites"""
    from hipops import ops
    from quantization.quantizer import _act_rows
    out = OrderedDict()
    for name, q in quants.items():
        mine = [c for c in calls if c[0] == name]
        for site in sorted({c[4] for c in mine}):
            tot = None
            for _, _, _, x, s, cl in mine:
                if s != site:
                    continue
                xr, _ = _act_rows(x, cl)
                C = xr.shape[-1]
                flat = xr.reshape(-1, C)
                rng = q.act_range[site].detach() if q.act_mode == "static" else torch.cat([flat.amin(0), flat.amax(0)]).contiguous()
                e, en = ops.actquant_width_scan(xr, rng, widths)
                if tot is None:
                    tot = [torch.zeros(len(widths), C, dtype=torch.float64, device="cuda"), torch.zeros(C, dtype=torch.float64, device="cuda"), 0]
                tot[0] += e.t().double()
                tot[1] += en.double()
                tot[2] += flat.shape[0]
            out[name if site == 0 else f"{name}#{site}"] = tuple(tot)
    return out


def _hand_row(qnn, images, batch, lmbda, fp=None):
    """an `rd_report` row of the state the model is in, by hand: the model batch for batch, each likelihood tensor once through
    `ops.neg_log2_channel_sums` and the squared error through `ops.sq_diff_sum_ordered`, added in float64 on the device"""
    from hipops import ops
    acc, sse = OrderedDict(), torch.zeros(1, dtype=torch.float64, device="cuda")
    with torch.no_grad():
        for i in range(0, images.shape[0], batch):
            x = images[i:i + batch].contiguous()
            out = qnn(x)
            for k, lik in out["likelihoods"].items():
                s = ops.neg_log2_channel_sums(lik).double()
                acc[k] = acc[k] + s if k in acc else s
            sse += ops.sq_diff_sum_ordered(out["x_hat"].contiguous(), x, 1.0, clamp01=True).double()
    n, _, H, W = images.shape
    P = n * H * W
    bits = OrderedDict((k, a.cpu()) for k, a in acc.items())
    total = float(sum(b.sum() for b in bits.values()))
    mse = float(sse) / (3 * P)
    r = OrderedDict(bits=bits, bits_total=total, sse=float(sse), bpp=total / P, mse=mse, psnr_db=float("inf") if mse == 0 else -10.0 * math.log10(mse))
    r["loss"] = r["bpp"] + lmbda * 255.0 ** 2 * mse
    if fp is not None:
        r["d_bits"] = OrderedDict((k, r["bits"][k] - fp["bits"][k]) for k in r["bits"])
        for f in ("bpp", "mse", "psnr_db", "loss"):
            r["d_" + f] = r[f] - fp[f]
    return r


def _check_bit_report(qnn, cali, names, widths, batch, want_batch, own=8):
    """the table of `widths` (the model's own width among them) on `names` -> it.  Checked: what every quantiser of the chosen units
    stands at in every forward; the row at the model's own width against passes done by hand (the shared columns: the same bits);
    elements and sizes counted from the hooked calls; act_err and act_sqnr_db against hand sums of the scan; their order in the width."""
    from quantization import BaseQuantBlock, QuantModule
    from quantization.utils import quant_state
    units = qnn.units()
    order = [u for u in units if u in names]
    quants = {name: OrderedDict(_applied(units[name])) for name in order}
    assert all(quants.values())
    tap = _Tap([(f"{name}/{qn}", q) for name in order for qn, q in quants[name].items()])
    try:
        rep = qnn.act_bit_report(cali, widths=widths, lmbda=LMBDA, weight_quant=False, batch=batch, units=names)
    finally:
        tap.remove()
    n, _, H, W = cali.shape
    assert list(rep) == ["fp", "units", "elements", "skipped", "widths", "n", "pixels", "lmbda", "weight_quant", "batch"]
    assert (rep["widths"], rep["n"], rep["pixels"], rep["lmbda"], rep["weight_quant"], rep["batch"], rep["skipped"]) == \
        (list(widths), n, n * H * W, LMBDA, False, want_batch, OrderedDict())
    assert list(rep["units"]) == list(rep["elements"]) == order
    # every hooked call belongs to its unit's own states, in order, at that state's width and scanning at it alone
    at = 0
    per_state = {}
    for name in order:
        mine = [c for c in tap.calls if c[0].startswith(name + "/")]
        assert all(a is b for a, b in zip(tap.calls[at:at + len(mine)], mine))       # (the states run unit after unit)
        at += len(mine)
        assert len(mine) % len(widths) == 0 and mine
        k = len(mine) // len(widths)
        for j, b in enumerate(widths):
            part = mine[j * k:(j + 1) * k]
            assert all(c[1] == b and c[2] == [b] for c in part), (name, b)
            per_state[(name, b)] = part
    assert at == len(tap.calls)
    with quant_state(qnn):
        qnn.set_quant_state(False, False)
        fp = _hand_row(qnn, cali, want_batch, LMBDA)
        _same_report(rep["fp"], fp)
        for name in order:
            qnn.set_quant_state(False, False)
            for m in units[name].modules():                                         # the unit and every wrapper nested in it
                if isinstance(m, (QuantModule, BaseQuantBlock)):
                    m.set_quant_state(False, True)
            want = _hand_row(qnn, cali, want_batch, LMBDA, fp)
            table = rep["units"][name]
            assert list(table) == list(widths)
            _same_report(OrderedDict((k, table[own][k]) for k in want), want)           # rel = 0: the same bits
            assert sorted(set(table[own]) - set(want)) == ["act_err", "act_sqnr_db", "size_bits"]
    for name in order:
        table = rep["units"][name]
        values = {b: sum(c[3].numel() for c in per_state[(name, b)]) for b in widths}
        assert len(set(values.values())) == 1 and values[own] % n == 0
        elements = values[own] // n
        assert rep["elements"][name] == elements > 0 and isinstance(rep["elements"][name], int)
        for b in widths:
            row = table[b]
            calls = [(c[0].split("/", 1)[1],) + c[1:] for c in per_state[(name, b)]]
            hand = _hand_scan(quants[name], calls, [b])
            err = float(sum(float(e.sum()) for e, _, _ in hand.values()))
            energy = float(sum(float(en.sum()) for _, en, _ in hand.values()))
            assert sum(cnt * en.numel() for _, en, cnt in hand.values()) == elements * n
            assert row["size_bits"] == b * elements and isinstance(row["size_bits"], int)
            assert row["act_err"] == pytest.approx(err, rel=1e-12, abs=0) and row["act_err"] > 0
            assert row["act_sqnr_db"] == pytest.approx(10.0 * math.log10(energy / err), rel=1e-12)
            assert row["d_loss"] == row["loss"] - rep["fp"]["loss"] and math.isfinite(row["d_loss"])
        rising = sorted(widths)
        assert all(table[a]["act_err"] > table[b]["act_err"] and table[a]["act_sqnr_db"] < table[b]["act_sqnr_db"]
                   for a, b in zip(rising, rising[1:])), name
    return rep


@pytest.fixture(scope="module")
def static_table(static_model):
    qnn, cali = static_model
    return _check_bit_report(qnn, cali, CHENG_UNITS, (4, 6, 8), 4, 4)


def test_table_on_frozen_static_ranges_keeps_the_batch(static_table):
    for name, table in static_table["units"].items():
        print(name, static_table["elements"][name], {b: (round(r["act_sqnr_db"], 2), r["d_loss"]) for b, r in table.items()})
    assert static_table["batch"] == 4


def test_table_on_dynamic_grids_runs_image_by_image(dynamic_model):
    qnn, cali = dynamic_model
    rep = _check_bit_report(qnn, cali, CHENG_UNITS, (4, 8), 4, 1)
    assert rep["batch"] == 1
    # units=None: the units in which nothing is applied are listed, with the reason, and have no row
    full = qnn.act_bit_report(cali[:1], widths=(8,), lmbda=LMBDA, batch=1)
    assert list(full["units"]) == CHENG_UNITS == list(full["elements"])
    assert list(full["skipped"]) == [u for u in qnn.units() if u not in CHENG_UNITS]
    assert all("no activation quantiser of the unit is applied" in why for why in full["skipped"].values())
    assert full["elements"] == rep["elements"]
    with pytest.raises(ValueError, match="act_bit_report: unit 'g_a.1': no activation quantiser of the unit is applied"):
        qnn.act_bit_report(cali, units=["g_a.0", "g_a.1"])
    # weight_quant=True: the unit's row is rd_report's with act_quant=True, the same bits
    both = qnn.act_bit_report(cali, widths=(8,), lmbda=LMBDA, weight_quant=True, batch=4, units=["g_s.0"])
    rd = qnn.rd_report(cali, lmbda=LMBDA, act_quant=True, batch=4, units=["g_s.0"])
    assert both["weight_quant"] is True and both["batch"] == rd["batch"] == 1
    _same_report(OrderedDict((k, both["units"]["g_s.0"][8][k]) for k in rd["units"]["g_s.0"]), rd["units"]["g_s.0"])


def _state(qnn):
    from quantization import BaseQuantBlock, QuantModule
    out = []
    for name, m in qnn.named_modules():
        if not isinstance(m, (QuantModule, BaseQuantBlock)):
            continue
        q = m.act_quantizer
        out.append({"name": name, "flags": (m.use_weight_quant, m.use_act_quant, m.trained), "q": id(q), "bits": q.dynamic_bits,
                    "mode": q.act_mode, "phase": q.act_phase, "stats_id": id(q.act_stats), "stats": sorted(q.act_stats),
                    "scan": (q.act_scan_widths, sorted(q.act_scan_sums)), "range_ids": {s: id(r) for s, r in q.act_range.items()},
                    "ranges": {s: r.clone() for s, r in q.act_range.items()}})
    return out


def _same_state(x, y):
    assert len(x) == len(y) > 0
    for r, s in zip(x, y):
        assert sorted(r) == sorted(s)
        for k in r:
            if k == "ranges":
                assert sorted(r[k]) == sorted(s[k]) and all(_same_bits(r[k][i], s[k][i]) for i in r[k]), (r["name"], k)
            else:
                assert r[k] == s[k], (r["name"], k)


def test_the_model_is_left_as_it_was_found(static_model, monkeypatch):
    qnn, cali = static_model
    units = qnn.units()
    try:
        qnn.set_quant_state(False, False)
        for k, u in enumerate(units.values()):                                      # mixed flags
            u.set_quant_state(k % 2 == 0, k % 3 == 0)
        units["g_a.6"].act_quantizer.dynamic_bits = 5                               # a unit that stands at another width
        before = _state(qnn)
        assert {r["flags"][:2] for r in before} >= {(True, False), (False, True), (False, False), (True, True)}
        assert any(r["stats"] for r in before) and any(r["ranges"] for r in before) and any(r["bits"] == 5 for r in before)
        with torch.no_grad():
            out0 = qnn(cali[:2])
        qnn.act_bit_report(cali, widths=(3, 8), lmbda=LMBDA, batch=4, units=CHENG_UNITS)
        _same_state(before, _state(qnn))
        with torch.no_grad():
            out1 = qnn(cali[:2])
        assert _same_bits(out0["x_hat"], out1["x_hat"]) and all(_same_bits(out0["likelihoods"][k], out1["likelihoods"][k]) for k in out0["likelihoods"])
        qnn.act_width_report(cali, widths=(3, 8), batch=4)
        _same_state(before, _state(qnn))
        # the forward raises half-way: batch 4 makes one call per state; call 3 is the state (g_a.0, 8), g_a.0's quantisers at 8 and
        # scanning, behind g_a.0 in the forward
        u = units["g_a.1"]
        for report, fail_at in ((lambda: qnn.act_bit_report(cali, widths=(3, 8), lmbda=LMBDA, batch=4, units=CHENG_UNITS), 3),
                                (lambda: qnn.act_width_report(cali, widths=(3, 8), batch=4), 1)):
            calls, real = [0], u.forward
            seen = []

            def failing(*a, calls=calls, real=real, fail_at=fail_at, seen=seen, **k):
                calls[0] += 1
                if calls[0] == fail_at:
                    seen.append([q.act_scan_widths for _, q in _applied(units["g_a.0"])])
                    raise RuntimeError("planted failure")
                return real(*a, **k)
            monkeypatch.setattr(u, "forward", failing)
            with pytest.raises(RuntimeError, match="planted failure"):
                report()
            assert calls[0] == fail_at and seen and all(w is not None for w in seen[0])      # (the scans were open when it failed)
            monkeypatch.undo()
            _same_state(before, _state(qnn))
        with torch.no_grad():
            out2 = qnn(cali[:2])
        assert _same_bits(out0["x_hat"], out2["x_hat"])
    finally:
        units["g_a.6"].act_quantizer.dynamic_bits = 8
        qnn.set_quant_state(True, True)


# ----------------------------------------------------------------------------- act_width_report
def _check_width_report(qnn, cali, widths, batch, want_batch):
    named = _applied(qnn)
    unit_of = {}
    for uname, u in qnn.units().items():
        for qn, _ in _applied(u, prefix=f"model.{uname}."):
            unit_of[qn] = uname
    tap = _Tap(named)
    try:
        rep = qnn.act_width_report(cali, widths=widths, batch=batch)
    finally:
        tap.remove()
    assert list(rep) == ["sites", "widths", "n", "batch"] and (rep["widths"], rep["n"], rep["batch"]) == (list(widths), cali.shape[0], want_batch)
    nb = -(-cali.shape[0] // want_batch)
    assert all(c[2] == list(widths) for c in tap.calls) and len(tap.calls) % nb == 0 and tap.calls
    hand = _hand_scan(OrderedDict(named), tap.calls, widths)
    assert list(rep["sites"]) == list(hand)
    for site, (err, energy, n) in hand.items():
        row, q = rep["sites"][site], dict(named)[site.split("#")[0]]
        assert (row["unit"], row["mode"], row["n_bits"], row["channels"], row["n"]) == \
            (unit_of[site.split("#")[0]], q.act_mode, q.dynamic_bits, energy.numel(), n)
        assert row["err"].dtype == torch.float64 and row["err"].device.type == "cpu" and row["err"].shape == (len(widths), energy.numel())
        assert torch.equal(row["err"], err.cpu()) and torch.equal(row["energy"], energy.cpu())
        e, en = err.cpu(), energy.cpu()
        want = torch.where(e == 0, torch.full_like(e, float("inf")), 10.0 * torch.log10(en.unsqueeze(0) / e))
        assert torch.equal(row["sqnr_db"], want)
        assert torch.equal(row["total"]["err"], e.sum(1)) and row["total"]["energy"] == float(en.sum())
        assert torch.allclose(row["total"]["sqnr_db"], 10.0 * torch.log10(en.sum() / e.sum(1)), rtol=1e-12, atol=0)
        rising = sorted(range(len(widths)), key=lambda k: widths[k])
        assert all(float(e[a].sum()) > float(e[b].sum()) for a, b in zip(rising, rising[1:])), site
    return rep


def test_width_report_is_the_hand_sum_of_one_pass(static_model, dynamic_model):
    qnn, cali = static_model
    rep = _check_width_report(qnn, cali, (4, 6, 8), 4, 4)
    assert list(rep["sites"]) == list(qnn.act_ranges())                             # the site names of act_ranges
    assert any("#" in s for s in rep["sites"]) and {r["unit"] for r in rep["sites"].values()} == set(CHENG_UNITS)
    # the column at the model's own width against act_report: the statistics the calibration recorded on each unit's cached inputs.
    # The first unit's cached inputs are the images themselves, as here, so its sites compare as recorded; a later unit's cache was
    # taken with the untrained units in front of it in full precision, so its statistics are taken again (`report_act_ranges`, the
    # scoring kernel) on the inputs the unit has in this pass
    from quantization.unit_passes import report_act_ranges
    units = qnn.units()
    recorded = qnn.act_report()
    assert list(recorded) == list(rep["sites"])
    inputs = {}
    hooks = [units[n].register_forward_pre_hook(lambda mod, args, n=n: inputs.__setitem__(n, args[0].detach().clone())) for n in CHENG_UNITS[1:]]
    try:
        qnn.set_quant_state(True, True)
        with torch.no_grad():
            qnn(cali)
    finally:
        for h in hooks:
            h.remove()
    held = {id(q): q.act_stats for _, q in qnn.act_quantizers()}
    try:
        for _, q in qnn.act_quantizers():
            q.act_stats = dict(q.act_stats)                                         # (the recorded statistics stay as the calibration left them)
        for n in CHENG_UNITS[1:]:
            report_act_ranges(units[n], inputs[n], batch=4)
        again = qnn.act_report()
    finally:
        for _, q in qnn.act_quantizers():
            q.act_stats = held[id(q)]
        qnn.set_quant_state(True, True)
    k = rep["widths"].index(8)
    for site, row in rep["sites"].items():
        src = recorded if row["unit"] == CHENG_UNITS[0] else again
        assert src[site]["n"] == row["n"] and src[site]["n_bits"] == 8
        worst = max(rel_err(row["err"][k], src[site]["err"].double()), rel_err(row["energy"], src[site]["energy"].double()))
        print(f"{site}: against act_report, largest relative difference {worst:.3e}")
        assert worst <= 1e-4
    qnn_d, cali_d = dynamic_model
    rep_d = _check_width_report(qnn_d, cali_d, (8, 4), 4, 1)
    assert rep_d["batch"] == 1 and {r["mode"] for r in rep_d["sites"].values()} == {"dynamic"} and len(rep_d["sites"]) == len(rep["sites"])


# ----------------------------------------------------------------------------- the flow
def test_allocation_is_applied_calibrated_exported_pickled_and_packed(static_table, tmp_path):
    from test_gpu_actquant_hist_mse import _toy
    from test_gpu_packed import _forward, _same_outputs, _scramble
    from quantization import BaseQuantBlock, block_reconstruction, layer_reconstruction
    from quantization.export import activation_state, allocate_act_bits
    rep = static_table
    alloc = allocate_act_bits(rep, avg_bits=6)
    total = sum(rep["elements"].values())
    assert alloc["budget_bits"] == 6 * total and alloc["size_bits"] <= alloc["budget_bits"]
    assert set(alloc["bits"].values()) <= {4, 6, 8} and min(alloc["bits"].values()) < 8 and list(alloc["bits"]) == CHENG_UNITS
    assert alloc["size_bits"] == sum(alloc["bits"][n] * rep["elements"][n] for n in CHENG_UNITS)
    qnn, cali, _, kwargs, _, _ = _toy(act_mode="static", act_range="max")          # a fresh model: the table's one stays as it is
    qnn.set_act_bits(alloc["bits"])
    units = qnn.units()
    got = qnn.act_bits()
    for n in units:
        assert set(got[n]["bits"].values()) == {alloc["bits"].get(n, 8)} and got[n]["applied"] == []
    # calibration at the widths: every call of a unit's quantisers during its loop and its range passes sees the unit's own width
    for k, name in enumerate(CHENG_UNITS):
        u = units[name]
        tap = _Tap([(f"{name}/{qn}", m.act_quantizer) for qn, m in u.named_modules() if hasattr(m, "act_quantizer")])
        torch.manual_seed(1005 + k)
        try:
            (block_reconstruction if isinstance(u, BaseQuantBlock) else layer_reconstruction)(qnn, u, name.split(".")[-1], **kwargs)
        finally:
            tap.remove()
        assert tap.calls and {c[1] for c in tap.calls} == {alloc["bits"][name]}, name
    qnn.eval()
    after = qnn.act_bits()
    assert {n: r["bits"] for n, r in after.items()} == {n: r["bits"] for n, r in got.items()}       # calibration does not move a width
    assert all(after[n]["applied"] for n in CHENG_UNITS) and not any(after[n]["applied"] for n in units if n not in CHENG_UNITS)
    ranges, state = qnn.act_ranges(), activation_state(qnn)
    assert list(ranges) == list(state) and len(state) >= 6
    for site, (lo, hi, n_bits) in ranges.items():
        unit = next(n for n in CHENG_UNITS if site.startswith(f"model.{n}."))
        assert n_bits == state[site]["n_bits"] == alloc["bits"][unit], site
    # allowed after calibration: the ranges stay, recorded statistics of the named units go
    x = cali[:2]
    want = _forward(qnn, x, (True, True))
    low = next(n for n in CHENG_UNITS if alloc["bits"][n] < 8)
    qnn.set_act_bits({low: 8})
    moved = qnn.act_ranges()
    assert set(qnn.act_bits()[low]["bits"].values()) == {8} and list(moved) == list(ranges)
    assert all(_same_bits(moved[s][0], ranges[s][0]) and _same_bits(moved[s][1], ranges[s][1]) for s in ranges)
    assert all(moved[s][2] == (8 if s.startswith(f"model.{low}.") else ranges[s][2]) for s in ranges)
    qnn.set_act_bits({low: alloc["bits"][low]})
    assert _same_outputs(want, _forward(qnn, x, (True, True)))
    # pickle and the packed checkpoint carry the widths; the loaded model computes the saved model's bits
    back = pickle.loads(pickle.dumps(qnn))
    assert back.act_bits() == qnn.act_bits() and _same_outputs(want, _forward(back, x, (True, True)))
    path = str(tmp_path / "act_bits.rdopack")
    qnn.save_packed(path)
    fresh, _, _, _, _, _ = _toy()
    _scramble(fresh)
    fresh.load_packed(path)
    loaded = activation_state(fresh)
    assert list(loaded) == list(state)
    for site in state:
        assert loaded[site]["n_bits"] == state[site]["n_bits"] and _same_bits(loaded[site]["lo"], state[site]["lo"])
        assert _same_bits(loaded[site]["hi"], state[site]["hi"])
    assert {n: fresh.act_bits()[n]["bits"] for n in CHENG_UNITS} == {n: after[n]["bits"] for n in CHENG_UNITS}
    assert _same_outputs(want, _forward(fresh, x, (True, True)))


# ----------------------------------------------------------------------------- a Swin unit
def test_one_swin_unit_of_toy_lu2022_counts_both_attention_sites():
    """the first RSTB of the toy Lu2022, marked trained, on dynamic grids: the probabilities [B_, N, N, heads] (site 0) and attn @ v
    (site 1) of every window attention are quantised, scanned and counted"""
    from quantization.quant_block import QuantRSTB, QuantWindowAttention
    qnn, cali = _lu2022()
    name = "g_a1"
    u = qnn.units()[name]
    assert isinstance(u, QuantRSTB)
    _mark_trained(u)
    attns = [(n, m) for n, m in u.named_modules() if isinstance(m, QuantWindowAttention)]
    assert attns
    tap = _Tap([(n, m.act_quantizer) for n, m in attns])
    try:
        rep = _check_bit_report(qnn, cali, [name], (4, 8), 2, 1)
    finally:
        tap.remove()
    n = cali.shape[0]
    mine = [c for c in tap.calls if c[2] == [8]]                                    # the state at width 8 (scanning: not the hand pass)
    for an, m in attns:
        sites = {s: [c for c in mine if c[0] == an and c[4] == s] for s in (0, 1)}
        assert len(sites[0]) == len(sites[1]) == n                                  # one call per image and site at each width
        assert all(c[5] and c[3].dim() == 4 and c[3].shape[-1] == m.num_heads and c[3].shape[1] == c[3].shape[2] for c in sites[0])
        assert all(not c[5] and c[3].shape[-1] == m.dim for c in sites[1])
    attention = sum(c[3].numel() for c in mine) // n
    assert 0 < attention < rep["elements"][name]


# ----------------------------------------------------------------------------- two ranks on one GPU
DP_UNITS = ["g_a.0", "g_s.7.0"]


def _dp_model():
    qnn, cali = _cheng()
    for n in DP_UNITS:
        _mark_trained(qnn.units()[n])
    qnn.units()["g_s.7.0"].disable_act_quant = False                                # (whatever the output rule made of it: applied here)
    return qnn, cali


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
        qnn, cali = _dp_model()
        rep = qnn.act_bit_report(cali[:3], widths=(4, 8), lmbda=LMBDA, batch=1, units=DP_UNITS)
        wide = qnn.act_width_report(cali[:3], widths=(4, 8), batch=1)
        out_q.put((rank, _plain(rep), _plain(wide)))
        dist.barrier()
    except BaseException as e:          # the parent must not wait out its queue timeout for a rank that failed
        out_q.put(("error", f"rank {rank}: {e!r}", None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_return_the_table_of_one():
    """Two processes on cuda:0 over gloo on three images (rank 0: images 0 and 2, rank 1: image 1), batch 1 (dynamic grids): both return
    the same tables, 'n' and 'pixels' are global, and the sums are the single process's to 1e-12 relative (the per-image fp32 values
    are the same; only the float64 addition order differs); the counts are the same whole numbers"""
    qnn, cali = _dp_model()
    want = qnn.act_bit_report(cali[:3], widths=(4, 8), lmbda=LMBDA, batch=1, units=DP_UNITS)
    want_wide = qnn.act_width_report(cali[:3], widths=(4, 8), batch=1)
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
        got, wide = {}, {}
        for _ in range(2):
            rk, val, w = q.get(timeout=180)
            assert rk != "error", val
            got[rk], wide[rk] = _plain(val, back=True), _plain(w, back=True)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    _same_report(got[0], got[1])
    _same_report(wide[0], wide[1])
    assert got[0]["n"] == 3 and got[0]["pixels"] == 3 * 64 * 64 and got[0]["batch"] == 1 and got[0]["widths"] == [4, 8]
    _same_report(got[0]["fp"], want["fp"], rel=1e-12)
    assert got[0]["elements"] == want["elements"] and list(got[0]["units"]) == DP_UNITS and got[0]["skipped"] == want["skipped"] == {}
    for name in DP_UNITS:
        for b in (4, 8):
            _same_report(got[0]["units"][name][b], want["units"][name][b], rel=1e-12)
            assert got[0]["units"][name][b]["size_bits"] == want["units"][name][b]["size_bits"] == b * want["elements"][name]
    assert wide[0]["n"] == 3 and list(wide[0]["sites"]) == list(want_wide["sites"]) and wide[0]["sites"]
    for site, row in want_wide["sites"].items():
        mine = wide[0]["sites"][site]
        assert (mine["n"], mine["channels"], mine["unit"], mine["mode"], mine["n_bits"]) == \
            (row["n"], row["channels"], row["unit"], row["mode"], row["n_bits"])
        for f in ("err", "energy"):
            assert bool(((mine[f] - row[f]).abs() <= 1e-12 * row[f].abs()).all()), (site, f)
