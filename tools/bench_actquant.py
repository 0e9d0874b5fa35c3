#!/usr/bin/env python3
"""Dynamic against static per-channel activation quantisation on one MI355X, on the shapes the product meets (NHWC fp32).

Kernel part: device-event timing after warm-up, the two quantisers ALTERNATING in one process (dynamic round, static round, ...; the
median round is reported), µs per call and GB/s against algorithmic bytes -- static 8 B per element (one read, one write), dynamic 12
(two reads, one write).  The static call does a strict subset of the dynamic call's work: a shape on which it is slower is flagged.
The range search (one read, ten candidates) and the range scoring of act_range='auto' and act_report (one read, K = 1 and K = 4 arbitrary
grids with their clipped counts and the energy) are timed next to them; with --bwd also the backward of the static quantiser (two reads, one
write: 12 B per element), whose share of the static forward's GB/s on the same tensor is reported; with --hist the per-channel histogram
pass of act_range='percentile' and 'hist_mse' (one read, 1024 integer bins per channel) and their C-sized selections (the percentile
cut and the exhaustive histogram-MSE search), in the same alternating windows as the search pass they stand in for; with --pair the
pair moments of the per-unit output error report (two reads: 8 B per element), in the same windows as the K = 1 score.

Learning part (--learn): wall time of `recon.learn_act_ranges` on one Cheng2020 block unit at N = 192 (a ResidualBlock on 32^2 inputs, what
g_a[5] sees for 256^2 crops), after a short warm-up run, device synchronised at both ends.

Flow part (--flow): the cache-building wall (`args.timing`, `cache_s`) of a W8A8 calibration schedule of a toy Cheng2020 (N = 8, 64^2
crops) in both modes -- dynamic grids build every unit's caches image by image, static ones in batches; with --hist also the range
fixing wall (`act_s`) of the static flow under act_range='l2' against 'percentile' and 'hist_mse'.

    python tools/bench_actquant.py [--reps 1000] [--rounds 7] [--bwd] [--hist] [--pair] [--learn] [--flow] [--images 32] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

SHAPES = [(4, 128, 128, 192), (4, 64, 64, 192), (4, 16, 16, 192), (1, 32, 48, 192), (1, 512, 768, 3)]


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def bench_kernels(reps, rounds, n_bits=8, bwd=False, hist=False, pair=False):
    from hipops import ops
    L = ops.L
    rows = []
    for shape in SHAPES:
        g = torch.Generator().manual_seed(sum(shape))
        x = (torch.randn(*shape, generator=g) * 3).cuda()
        C, n = shape[-1], x.numel()
        out = torch.empty_like(x)
        ws = torch.empty(int(L.lib().rdo_actquant_workspace(C)), device="cuda")
        sws = torch.empty(int(L.lib().rdo_actquant_search_workspace(C)), device="cuda")
        rng = ops.act_range_init(C, "cuda")
        ops.actquant_observe(x, rng, n_bits=n_bits)
        err = torch.zeros(C, ops.ACT_SEARCH_CANDIDATES, device="cuda")
        # the grids 'auto' would score: the observed range and three shrunk ones (what they are does not change the work per element)
        cand4 = torch.stack([rng * s for s in (1.0, 0.9, 0.8, 0.7)]).contiguous()
        cand1 = cand4[1:2].contiguous()
        cws = torch.empty(int(L.lib().rdo_actquant_score_workspace(C, ops.ACT_SCORE_MAX)), device="cuda")
        cerr = {k: torch.zeros(C, k, device="cuda") for k in (1, 4)}
        cclip = {k: torch.zeros(C, k, 2, dtype=torch.int32, device="cuda") for k in (1, 4)}
        cen = torch.zeros(C, device="cuda")

        def score_call(cand):
            k = cand.shape[0]
            cclip[k].zero_()                                       # (32-bit counts: every call starts empty; a C-sized memset)
            ops.actquant_score(x, cand, cerr[k], cclip[k], cen, n_bits=n_bits, ws=cws)
        calls = {
            "dynamic": lambda: ops.actquant_perchannel(x, out=out, ws=ws, n_bits=n_bits),
            "static": lambda: ops.actquant_static(x, rng, out=out, n_bits=n_bits),
            "search": lambda: ops.actquant_search(x, rng, err, n_bits=n_bits, ws=sws),
            "score1": lambda: score_call(cand1),
            "score4": lambda: score_call(cand4),
        }
        if bwd:
            gx = torch.randn(*shape, generator=g).cuda()
            dx, dr = torch.empty_like(x), torch.zeros(2 * C, device="cuda")
            bws = torch.empty(int(L.lib().rdo_actquant_static_bwd_workspace(C)), device="cuda")
            calls["bwd"] = lambda: ops.actquant_static_bwd(x, gx, rng, dr, dx=dx, n_bits=n_bits, ws=bws)
        if hist:
            hh = ops.act_hist_init(C, "cuda")
            sel = [None]

            def hist_call():
                ops.actquant_hist(x, rng, hh)

            def select_call():
                sel[0] = ops.act_percentile_select(hh, rng, 1e-4)

            def select_mse_call():
                sel[0] = ops.act_hist_mse_select(hh, rng, n_bits)
            calls["hist"], calls["select"], calls["select_mse"] = hist_call, select_call, select_mse_call
        if pair:
            y = (x + 0.01 * torch.randn(*shape, generator=g).cuda()).contiguous()
            pout = torch.zeros(3, C, device="cuda")
            calls["pair"] = lambda: ops.pair_moments(x, y, out=pout)
        r = reps
        for fn in calls.values():                              # warm-up: code objects, caches
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(rounds):                                # alternate within one process
            for k, fn in calls.items():
                if k == "hist":
                    hh.zero_()                                     # (the counters are 32-bit: every window starts empty)
                t[k].append(_time_us(fn, r))
        assert torch.equal(ops.actquant_static(x, rng, n_bits=n_bits), ops.actquant_perchannel(x, n_bits=n_bits))
        med = {k: statistics.median(v) for k, v in t.items()}
        row = dict(shape=list(shape), elements=n, reps=r, rounds=rounds,
                   dynamic_us=round(med["dynamic"], 2), static_us=round(med["static"], 2), search_us=round(med["search"], 2),
                   dynamic_spread_us=[round(min(t["dynamic"]), 2), round(max(t["dynamic"]), 2)],
                   static_spread_us=[round(min(t["static"]), 2), round(max(t["static"]), 2)],
                   dynamic_gbs=round(12.0 * n / med["dynamic"] / 1e3, 1), static_gbs=round(8.0 * n / med["static"] / 1e3, 1),
                   search_gbs=round(4.0 * n / med["search"] / 1e3, 1),
                   score1_us=round(med["score1"], 2), score4_us=round(med["score4"], 2),
                   score4_spread_us=[round(min(t["score4"]), 2), round(max(t["score4"]), 2)],
                   score1_gbs=round(4.0 * n / med["score1"] / 1e3, 1), score4_gbs=round(4.0 * n / med["score4"] / 1e3, 1),
                   score4_over_search=round(med["score4"] / med["search"], 2),
                   speedup=round(med["dynamic"] / med["static"], 2), static_slower=bool(med["static"] > med["dynamic"]))
        if bwd:
            bwd_gbs = 12.0 * n / med["bwd"] / 1e3
            row.update(bwd_us=round(med["bwd"], 2), bwd_spread_us=[round(min(t["bwd"]), 2), round(max(t["bwd"]), 2)], bwd_gbs=round(bwd_gbs, 1),
                       bwd_share_of_static_gbs=round(bwd_gbs / (8.0 * n / med["static"] / 1e3), 2))
        if hist:
            assert int(hh.sum()) == r * n and bool((hh.sum(1) == r * (n // C)).all())     # the last window's counts: nothing lost
            row.update(hist_us=round(med["hist"], 2), hist_spread_us=[round(min(t["hist"]), 2), round(max(t["hist"]), 2)],
                       hist_gbs=round(4.0 * n / med["hist"] / 1e3, 1), select_us=round(med["select"], 2),
                       select_mse_us=round(med["select_mse"], 2),
                       select_mse_spread_us=[round(min(t["select_mse"]), 2), round(max(t["select_mse"]), 2)],
                       hist_over_search=round(med["hist"] / med["search"], 2))
        if pair:
            row.update(pair_us=round(med["pair"], 2), pair_spread_us=[round(min(t["pair"]), 2), round(max(t["pair"]), 2)],
                       pair_gbs=round(8.0 * n / med["pair"] / 1e3, 1), pair_over_score1=round(med["pair"] / med["score1"], 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_learn(iters=100, images=64, batch=32, n=192, side=32, bits=8):
    """`learn_act_ranges` on a ResidualBlock unit (N = 192, three quantisation points), seconds per `iters` steps and per 500."""
    import lic
    from quantization import BaseQuantBlock, QuantModule
    from quantization.quant_block import QuantRB
    from quantization.recon import calibrate_act_ranges, learn_act_ranges
    torch.manual_seed(1005)
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False, "dynamic_bits": bits, "act_mode": "static"}
    unit = QuantRB(lic.ResidualBlock(n, n), wq, aq).cuda().eval()
    x = torch.randn(images, n, side, side, generator=torch.Generator().manual_seed(3)).cuda()
    unit.set_quant_state(False, False)
    with torch.no_grad():
        out_fp = unit(x).clone()
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.trained = True
    rows = []
    for rep in range(3):
        calibrate_act_ranges(unit, x, "l2", batch=batch, keep_obs=True)
        learn_act_ranges(unit, x, out_fp, 10, 1e-3, batch, seed=1)              # warm-up: code objects, weight packs, allocator
        calibrate_act_ranges(unit, x, "l2", batch=batch, keep_obs=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        learn_act_ranges(unit, x, out_fp, iters, 1e-3, batch, seed=1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rows.append(dict(unit=f"ResidualBlock N={n}", inputs=[images, n, side, side], batch=batch, iters=iters, wall_s=round(dt, 4),
                         ms_per_iter=round(1e3 * dt / iters, 3), s_per_500=round(dt / iters * 500, 3)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_flow(images, iters=6, hist=False):
    """cache_s of every unit of the toy W8A8 schedule, dynamic then static (then dynamic and static again: the spread); with `hist`
    then the static flow with act_range='l2', 'percentile' and 'hist_mse', twice each: their act_s."""
    import torch.nn as nn
    import lic
    from quantization import BaseQuantBlock, QuantModel, QuantModule, block_reconstruction, layer_reconstruction

    def run(mode, act_range="max"):
        torch.manual_seed(1005)
        model = lic.Cheng2020Anchor(N=8).cuda().eval()
        g = torch.Generator().manual_seed(13)
        cali = torch.rand(images, 3, 64, 64, generator=g).cuda()
        wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
        aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
        qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq, is_cheng=True).cuda().eval()
        qnn.set_first_last_layer_to_8bit()
        qnn.disable_network_output_quantization()
        qnn.set_quant_state(True, False)
        with torch.no_grad():
            qnn(cali[:2])
        timing = []
        args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Cheng2020", act_mode=mode, act_range=act_range, timing=timing)
        kw = dict(cali_data=cali, batch_size=2, iters=iters, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2), warmup=0.2,
                  act_quant=True, opt_mode="mse", config=None, args=args)
        qnn.set_quant_state(True, True)

        def walk(m: nn.Module):
            for name, c in m.named_children():
                if isinstance(c, QuantModule):
                    layer_reconstruction(qnn, c, name, **kw)
                elif isinstance(c, BaseQuantBlock):
                    block_reconstruction(qnn, c, name, **kw)
                else:
                    walk(c)
        walk(qnn)
        return dict(mode=mode, act_range=act_range, images=images, units=len(timing), cache_s=round(sum(t["cache_s"] for t in timing), 4),
                    act_s=round(sum(t.get("act_s", 0.0) for t in timing), 4), loop_s=round(sum(t["loop_s"] for t in timing), 4))
    rows = []
    for mode in ("dynamic", "static", "dynamic", "static"):
        rows.append(run(mode))
        print(json.dumps(rows[-1]), flush=True)
    for how in (("l2", "percentile", "hist_mse") * 2 if hist else ()):
        rows.append(run("static", how))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=1000, help="calls per timed window (7-33 us each: windows of 7 ms and more)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bwd", action="store_true", help="also time the backward of the static quantiser")
    ap.add_argument("--hist", action="store_true", help="also time the histogram pass and the selections of act_range='percentile' and 'hist_mse'; "
                    "with --flow also act_s of the toy flow under 'l2' against 'percentile' and 'hist_mse'")
    ap.add_argument("--pair", action="store_true", help="also time ops.pair_moments (the per-unit output error report) beside the K = 1 score")
    ap.add_argument("--learn", action="store_true", help="time learn_act_ranges on one N = 192 block unit")
    ap.add_argument("--flow", action="store_true")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_actquant needs a GPU: there is no CPU path to time")
    res = {"kernels": bench_kernels(a.reps, a.rounds, bwd=a.bwd, hist=a.hist, pair=a.pair)}
    slow = [r["shape"] for r in res["kernels"] if r["static_slower"]]
    if slow:
        print(f"DEFECT: static slower than dynamic on {slow}", flush=True)
    if a.learn:
        res["learn"] = bench_learn()
    if a.flow:
        res["flow"] = bench_flow(a.images, hist=a.hist)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 1 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
