#!/usr/bin/env python3
"""The batched AdaRound step on MX grids (`ops.mx_round_step_batch`: mx_step_batch_kernel + mx_dgrad_batch_kernel of
csrc/mx_round_batch.hip, two launches) on one MI355X, next to the per-tensor sequence it replaces on the same tensors in the same
process, alternating: per weight `ops.mx_round_step` (step + transpose launch) and one split launch per plane buffer, then one
`ops.iter_advance`.  Three weight sets: the 192-channel 3x3 conv of a layer unit, the three convs of a residual block (1x1 192 -> 96,
3x3 96 -> 96, 1x1 96 -> 192) and a 192 x 192 GDN gamma.  Convs carry fp16 planes of wq and wd, the gamma the Linear planes of itself
and of its transpose; gradient-slab counts are those of `ops.wgrad_nsplit` on a 128 x 128 map at batch 4 (--nsplit overrides).

Each sequence is recorded once into a plan and replayed `reps` times as a graph, so a window holds kernels and not the host's enqueue
rate; device events around the replay after a warm-up replay; the median window of `rounds` is reported with the spread, and `ratio`
= batched / per-tensor of the same set.  Both sequences read the iteration counter at a fixed row and advance a spare word, so a replay
never walks off the schedule table.

    python tools/bench_mx_round_batch.py [--reps 200] [--rounds 7] [--nsplit N] [--format mxfp4] [--json out.json] [--log profiles/mx_round_batch_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

SETS = {"layer 3x3 192": [(192, 3, 3, 192)], "block 1x1 96 / 3x3 96 / 1x1 192": [(96, 1, 1, 192), (96, 3, 3, 96), (192, 1, 1, 96)],
        "gamma 192": [(192, 192)]}
ROUND_WEIGHT = 0.01
REPARAM = (2.0 ** -18, 2.0 ** -36)


def _time_us(plan, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    plan.run(reps, graph=True)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def _items(shapes, fmt, nsplit, g):
    """two copies of the state of one weight set: one for each sequence"""
    from hipops import ops
    pair = ([], [])
    for shape in shapes:
        gamma = len(shape) == 2
        w4 = (shape[0], 1, 1, shape[1]) if gamma else shape
        ns = nsplit or ops.wgrad_nsplit((4, 128, 128, w4[3]), w4, 1, w4[1] // 2)
        w = (torch.randn(shape, generator=g) * (2.0 / (w4[1] * w4[2] * w4[3])) ** 0.5)
        w = (w.abs() + REPARAM[0] if gamma else w).cuda().contiguous()
        slabs = (1e-3 * torch.randn((ns,) + tuple(shape), generator=g)).cuda()
        lo, gap = ops.mx_neighbours(w.reshape(shape[0], -1), fmt)
        lo, gap = lo.reshape(shape), gap.reshape(shape)
        scale = ops.pow2_scale(float(torch.maximum(lo.abs(), (lo + gap).abs()).max()))
        for items in pair:
            it = dict(d=ops.ada_desc(w, reparam=REPARAM if gamma else None), lo=lo, gap=gap, slabs=slabs, alpha=ops.mx_round_init_alpha(w, lo, gap),
                      m=torch.zeros_like(w), v=torch.zeros_like(w), wq=torch.empty_like(w), wd=torch.empty_like(w), w4=w4)
            planes = lambda: ops.H2(torch.empty((2,) + tuple(shape), device="cuda", dtype=torch.int16), scale)
            it.update(dict(lin_fwd=planes(), lin_bwd=planes()) if gamma else dict(wq_planes=planes(), wd_planes=planes()))
            items.append(it)
    return pair


def _per_tensor(items, sched, it, spare, log):
    from hipops import ops
    for t in items:
        ops.mx_round_step(t["d"], t["lo"], t["gap"], t["slabs"], 1.0, ROUND_WEIGHT, sched, it, t["alpha"], t["m"], t["v"], t["wq"], t["wd"], log)
        co, kh, kw, ci = t["w4"]
        wq4, wd4 = t["wq"].reshape(co, kh, kw, ci), t["wd"].reshape(ci, kh, kw, co)
        if "wq_planes" in t:
            ops.split_h2_conv(wq4, planes=t["wq_planes"])
            ops.split_h2_conv(wd4, planes=t["wd_planes"])
        else:
            ops.split_h2_linear(wq4, planes=t["lin_fwd"])
            ops.split_h2_linear(wd4, planes=t["lin_bwd"])
    ops.iter_advance(spare)


def run(reps, rounds, fmt, nsplit):
    from hipops import ops
    from hipops.plan import Plan
    g = torch.Generator().manual_seed(1005)
    iters = 8
    sched = ops.make_sched(iters, 0.0, (20, 2), 1e-3, "cuda")
    it = torch.full((1,), 3, dtype=torch.int32, device="cuda")              # a row with the rounding term on; neither sequence moves it
    spare = torch.zeros(1, dtype=torch.int32, device="cuda")                # the word both sequences advance
    out = []
    for name, shapes in SETS.items():
        per, bat = _items(shapes, fmt, nsplit, g)
        log = torch.zeros(iters, 32, device="cuda")
        plans = {"per-tensor": Plan(), "batched": Plan()}
        with plans["per-tensor"].record():
            _per_tensor(per, sched, it, spare, log)
        with plans["batched"].record():
            ops.mx_round_step_batch([{k: v for k, v in t.items() if k != "w4"} for t in bat], 1.0, ROUND_WEIGHT, sched, it, log, advance_iter=spare)
        launches = {"per-tensor": 4 * len(shapes) + 1, "batched": 2}        # step, transpose and two splits a tensor, the counter | step, dgrad
        for p in plans.values():                                   # warm-up: code objects, the graph of `reps` replays
            p.prepare(reps)
            p.run(reps, graph=True)
        torch.cuda.synchronize()
        same = all(torch.equal(a[k].t if isinstance(a[k], ops.H2) else a[k], b[k].t if isinstance(b[k], ops.H2) else b[k])
                   for a, b in zip(per, bat) for k in a if k not in ("d", "w4"))
        if not same:
            raise SystemExit(f"{name}: the two sequences left different state after the same number of steps")
        t = {k: [] for k in plans}
        for _ in range(rounds):                                    # alternate within one process
            for k, p in plans.items():
                t[k].append(_time_us(p, reps))
        base = statistics.median(t["per-tensor"])
        for k, v in t.items():
            us = statistics.median(v)
            out.append(dict(set=name, format=fmt, nsplit=[int(x["slabs"].shape[0]) for x in per], path=k, us=round(us, 2),
                            spread_us=[round(min(v), 2), round(max(v), 2)], ratio=round(us / base, 3), launches=launches[k], reps=reps, rounds=rounds))
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
        raise SystemExit("bench_mx_round_batch needs a GPU: there is no CPU path to time")
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
