#!/usr/bin/env python3
"""The one-launch MX residual unit (`ops.mx_residual_unit`; csrc/mx_resunit.hip) on one MI355X where the attention blocks of
Cheng2020-attn sit: B = 4, 16 x 16 and 64 x 64 pixels, N = 128 and 192, mxfp4 and mxfp8_e4m3 for activations and weights alike.  Per
shape and format, from one process, alternating:
  composition       the un-fused sequence the launch is bit for bit: mx_quant_pack, mx_gemm (packed output, ReLU), mx_conv2d (3x3, packed
                    output, ReLU), mx_gemm, add, relu -- six launches through `ops`.  (A switched-off model runs eleven: it does not chain
                    the convs through packed outputs.)
  mx_residual_unit  `ops.mx_residual_unit` (one launch)
Each is timed twice.  `issue='eager'`: `reps` calls through `ops` from Python -- what a model's forward pays, the host's enqueue of six
launches against one included.  `issue='graph'`: the same calls recorded once into a plan and replayed `reps` times as a graph, so a
window holds kernels and not the host's enqueue -- what the kernels themselves take.
A first measurement and a record, not a bar: what is to be seen is on which side of the composition the one launch falls, by more than
the spread between windows of one call.

Device-event timing around `reps` calls after warm-up (2 000 by default: a window of 0.1 s and more), `rounds` alternating windows; the
median window is reported with its spread.  Before timing, the launch's output is compared with the composition's on the timed shape
(`bits_equal`), or the run stops.

    python tools/bench_mx_resunit.py [--reps 2000] [--rounds 5] [--json out.json] [--log profiles/mx_resunit_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

BATCH = 4
SIDES = (16, 64)
WIDTHS = (128, 192)
FORMATS = ("mxfp4", "mxfp8_e4m3")


def _time_us(fn, reps):
    """fn: a callable, called `reps` times, or a plan, replayed `reps` times as a graph"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if callable(fn):
        for _ in range(reps):
            fn()
    else:
        fn.run(reps, graph=True)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def run(reps, rounds):
    from hipops import ops
    from hipops.plan import Plan
    g = torch.Generator().manual_seed(1006)
    out = []
    for N in WIDTHS:
        Nh = N // 2
        W1, W2, W3 = ((torch.randn(n, k, generator=g) * k ** -0.5).cuda() for n, k in ((Nh, N), (Nh, 9 * Nh), (N, Nh)))
        b1, b2, b3 = ((0.1 * torch.randn(n, generator=g)).cuda() for n in (Nh, Nh, N))
        for side in SIDES:
            shape = (BATCH, side, side)
            x = (torch.randn(BATCH * side * side, N, generator=g) ** 3 * 0.3).cuda().contiguous()
            for fmt in FORMATS:
                w1, w2, w3 = (ops.mx_quant_pack(w, fmt) for w in (W1, W2, W3))

                def composition(keep=None):
                    xp = ops.mx_quant_pack(x, fmt)
                    h1 = ops.mx_gemm(xp, w1, b1, out_fmt=fmt, act="relu")
                    h2 = ops.mx_conv2d(h1, w2, shape, 3, 1, 1, b2, out_fmt=fmt, act="relu")
                    br = ops.mx_gemm(h2, w3, b3)
                    s = ops.add(x, br)
                    y = ops.relu(s)
                    if keep is not None:                               # a plan replays into the tensors of its recording
                        keep.keep(xp.packed, xp.scales, h1.packed, h1.scales, h2.packed, h2.scales, br, s, y)
                    return y

                def one(keep=None):
                    y = ops.mx_residual_unit(x, shape, w1, b1, w2, b2, w3, b3, fmt)
                    if keep is not None:
                        keep.keep(y)
                    return y

                if not torch.equal(one(), composition()):
                    raise SystemExit(f"N {N} {side} x {side} {fmt}: mx_residual_unit's output is not the composition's")
                calls = {("composition", "eager"): composition, ("mx_residual_unit", "eager"): one}
                for what, fn in (("composition", composition), ("mx_residual_unit", one)):
                    plan = Plan()
                    with plan.record():
                        fn(plan)
                    plan.prepare(reps)
                    calls[(what, "graph")] = plan
                for fn in calls.values():                              # warm-up: code objects, the allocator's blocks, the graphs
                    if callable(fn):
                        for _ in range(3):
                            fn()
                    else:
                        fn.run(reps, graph=True)
                torch.cuda.synchronize()
                t = {key: [] for key in calls}
                for _ in range(rounds):                                # alternate within one process
                    for key, fn in calls.items():
                        t[key].append(_time_us(fn, reps))
                med = {k: statistics.median(v) for k, v in t.items()}
                for (what, issue), v in t.items():
                    row = dict(shape=f"resunit{N}@{BATCH}x{side}x{side}", B=BATCH, H=side, W=side, N=N, format=fmt, call=what, issue=issue,
                               us=round(med[(what, issue)], 2), spread_us=[round(min(v), 2), round(max(v), 2)],
                               of_composition=round(med[(what, issue)] / med[("composition", issue)], 3), reps=reps, rounds=rounds,
                               bits_equal=True)
                    out.append(row)
                    print(json.dumps(row), flush=True)
                del calls
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=2000, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--log", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_resunit needs a GPU: there is no CPU path to time")
    rows = run(a.reps, a.rounds)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
