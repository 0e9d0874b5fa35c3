#!/usr/bin/env python3
"""The fused AdaRound step on an MX grid (`ops.mx_round_step`; mx_step_kernel + mx_wd_transpose_kernel of csrc/mx_round.hip) on one
MI355X, next to the integer-grid step it mirrors (`ops.adaround_step`: the flat form of csrc/adaround.hip with its dgrad launch, no
planes) on the same tensors in the same process, alternating: the two weights of the flagship codec's blocks, 192x3x3x192 and
192x1x1x192, at the gradient-slab counts the engine uses for them on a 128 x 128 feature map at batch 4 (`ops.wgrad_nsplit`; --nsplit
overrides).  The MX step reads one more fp32 stream per element (lo, gap against w) and does no per-row look-ups and no division.

Each call is recorded once into a plan and replayed `reps` times as a graph, so the window holds kernels and not the host's enqueue
rate; device events around the replay after a warm-up replay; the median window of `rounds` is reported with the spread, and
`ratio` = MX step / integer-grid step of the same row.  The byte count of a step is 4 B x numel x (nsplit + 9): the slabs, five streams
read (lo / gap or w, alpha, m, v) and four written (alpha, m, v, wq), wq read again and wd written by the second launch.

    python tools/bench_mx_round.py [--reps 200] [--rounds 7] [--nsplit N] [--format mxfp4] [--json out.json] [--log profiles/mx_round_step_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

SHAPES = ((192, 3, 3, 192), (192, 1, 1, 192))
X_SHAPE = (4, 128, 128, 192)      # the activations whose weight gradient the slabs hold: decides the slab count
ROUND_WEIGHT = 0.01


def _time_us(plan, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    plan.run(reps, graph=True)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def run(reps, rounds, fmt, nsplit):
    from hipops import ops
    from hipops.plan import Plan
    g = torch.Generator().manual_seed(1005)
    iters = 8
    sched = ops.make_sched(iters, 0.0, (20, 2), 1e-3, "cuda")
    it = torch.full((1,), 3, dtype=torch.int32, device="cuda")              # a row with the rounding term on; the step never moves it
    out = []
    for w4 in SHAPES:
        rows, kh = w4[0], w4[1]
        ns = nsplit or ops.wgrad_nsplit(X_SHAPE, w4, 1, kh // 2)
        w = (torch.randn(w4, generator=g) * (2.0 / (w4[1] * w4[2] * w4[3])) ** 0.5).cuda().contiguous()
        slabs = (1e-3 * torch.randn((ns,) + w4, generator=g)).cuda()
        log = torch.zeros(iters, 32, device="cuda")
        d = ops.ada_desc(w)
        # integer grid
        delta, zp = ops.uaq_init_minmax(w.reshape(rows, -1), 256)
        st_i = dict(alpha=ops.adaround_init_alpha(d, w, delta), m=torch.zeros_like(w), v=torch.zeros_like(w), wq=torch.empty_like(w),
                    wd=torch.empty_like(w))
        # MX grid
        lo, gap = ops.mx_neighbours(w.reshape(rows, -1), fmt)
        lo, gap = lo.reshape(w4), gap.reshape(w4)
        st_m = dict(alpha=ops.mx_round_init_alpha(w, lo, gap), m=torch.zeros_like(w), v=torch.zeros_like(w), wq=torch.empty_like(w),
                    wd=torch.empty_like(w))
        plans = {"int8": Plan(), fmt: Plan()}
        with plans["int8"].record():
            ops.adaround_step(d, w, delta, zp, slabs, 1.0, ROUND_WEIGHT, sched, it, st_i["alpha"], st_i["m"], st_i["v"], st_i["wq"], st_i["wd"], log)
        with plans[fmt].record():
            ops.mx_round_step(d, lo, gap, slabs, 1.0, ROUND_WEIGHT, sched, it, st_m["alpha"], st_m["m"], st_m["v"], st_m["wq"], st_m["wd"], log)
        for p in plans.values():                                   # warm-up: code objects, the graph of `reps` replays
            p.prepare(reps)
            p.run(reps, graph=True)
        torch.cuda.synchronize()
        if not (bool(torch.isfinite(st_i["wq"]).all()) and bool(torch.isfinite(st_m["wq"]).all())):
            raise SystemExit(f"{w4}: a step left a non-finite weight")
        t = {k: [] for k in plans}
        for _ in range(rounds):                                    # alternate within one process
            for k, p in plans.items():
                t[k].append(_time_us(p, reps))
        base = statistics.median(t["int8"])
        for k, v in t.items():
            us = statistics.median(v)
            out.append(dict(weight="x".join(str(s) for s in w4), nsplit=int(ns), grid=k, us=round(us, 2), spread_us=[round(min(v), 2), round(max(v), 2)],
                            ratio=round(us / base, 3), gbytes_per_s=round(4.0 * w.numel() * (ns + 9) / us / 1e3, 1), reps=reps, rounds=rounds,
                            pinned_share=round(float((gap == 0).float().mean()), 4) if k != "int8" else None))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200, help="replays per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--nsplit", type=int, default=0, help="gradient slabs (default: what ops.wgrad_nsplit gives for the shape)")
    ap.add_argument("--format", default="mxfp4")
    ap.add_argument("--json", default=None)
    ap.add_argument("--log", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_round needs a GPU: there is no CPU path to time")
    rows = run(a.reps, a.rounds, a.format, a.nsplit)
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    if a.log:
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
