#!/usr/bin/env python3
"""The activation width scan (`ops.actquant_width_scan`; aqw_partial_kernel of csrc/actquant.hip) on one MI355X: ONE scan of K = 8 widths
against the EIGHT K = 1 launches of the scoring kernel (`ops.actquant_score`, one per width, on the same grid) that measure the same
eight error sums, on a 16 384 x 192 activation (a 128 x 128 feature map of 192 channels), all in one process and alternating.  Next to
them a K = 1 scan, a K = 3 scan (the default widths of the reports) and a device-to-device copy of the tensor (one read and one write of
the same bytes).  A record, not a bar.

Device-event timing after warm-up; the median window is reported, with the spread.  The scan and the eight launches are compared on
their results first (1e-4 relative: two fp32 summations of the same terms).

    python tools/bench_act_width_scan.py [--reps 500] [--rounds 7] [--json out.json] [--log profiles/act_width_scan_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

NPIX, CHANNELS = 16384, 192
WIDTHS = (2, 3, 4, 6, 8, 10, 12, 16)


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def run(reps, rounds):
    from hipops import ops
    g = torch.Generator().manual_seed(1005)
    x = (torch.randn(NPIX, CHANNELS, generator=g) ** 3).cuda().contiguous()
    lo, hi = x.amin(0), x.amax(0)
    rng = torch.cat([lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo)]).contiguous()
    cand = rng.reshape(1, -1).contiguous()
    err1 = [torch.zeros(CHANNELS, 1, device="cuda") for _ in WIDTHS]
    dst = torch.empty_like(x)

    def eight_scores():
        for e, b in zip(err1, WIDTHS):
            ops.actquant_score(x, cand, e, n_bits=b)

    # the same sums, first
    scan, _ = ops.actquant_width_scan(x, rng, WIDTHS)
    eight_scores()
    ref = torch.cat(err1, dim=1)
    worst = float(((scan - ref).abs() / ref).max())
    if not worst <= 1e-4:
        raise SystemExit(f"the scan and the eight score launches differ by {worst:.3e} relative")
    calls = {"copy_d2d": lambda: dst.copy_(x), "scan_k8": lambda: ops.actquant_width_scan(x, rng, WIDTHS), "score_k1_x8": eight_scores,
             "scan_k1": lambda: ops.actquant_width_scan(x, rng, (8,)), "scan_k3": lambda: ops.actquant_width_scan(x, rng, (4, 6, 8)),
             "score_k1": lambda: ops.actquant_score(x, cand, err1[0], n_bits=8)}
    for fn in calls.values():                                      # warm-up: code objects, the workspaces, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in calls}
    for _ in range(rounds):                                        # alternate within one process
        for name, fn in calls.items():
            t[name].append(_time_us(fn, reps))
    row = dict(npix=NPIX, channels=CHANNELS, widths=list(WIDTHS), mbytes=round(4e-6 * NPIX * CHANNELS, 2), reps=reps, rounds=rounds,
               largest_relative_difference=worst)
    for name, v in t.items():
        row[f"{name}_us"] = round(statistics.median(v), 2)
        row[f"{name}_spread_us"] = [round(min(v), 2), round(max(v), 2)]
    row["scan_k8_bytes_per_us"] = round(4.0 * NPIX * CHANNELS / row["scan_k8_us"], 1)           # the one read of x over the call's time
    row["speedup"] = round(row["score_k1_x8_us"] / row["scan_k8_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=500, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--log", default=None, help="append the result line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_act_width_scan needs a GPU: there is no CPU path to time")
    out = run(a.reps, a.rounds)
    line = json.dumps(out)
    print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.log:
        with open(a.log, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
