#!/usr/bin/env python3
"""The MX window attention (`ops.mx_window_attention`; csrc/mx_attn.hip) on one MI355X against the fp32 attention core it stands in for
(`ops.window_attention`; csrc/swin.hip), at the Lu2022 shape B = 4, 128 x 128, C = 192, window 8: 4 and 8 heads (head dims 48 and 24),
shift 0 and 4, mxfp4 and mxfp8_e4m3 for Q / K / V and the probabilities alike.  Per geometry and format, from one process, alternating:
  fp32_attention   `ops.window_attention` (one launch; fp32 MFMA, no quantisation)
  mx_attention     `ops.mx_window_attention` (one launch; three quantisation phases, both products on the block-scaled instruction)
The two do NOT compute the same thing -- the MX core rounds Q, K, P and V -- so nothing is compared but time; the figure printed beside it
is the largest |difference| of the two outputs over the largest |fp32 output|, for the record.  A first measurement and a record, not a bar.

Device-event timing around `reps` calls after warm-up, `rounds` alternating windows; the median window is reported with its spread.

    python tools/bench_mx_attn.py [--reps 20] [--rounds 7] [--json out.json] [--log profiles/mx_attn_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

B, HW, C, WINDOW = 4, 128, 192, 8
HEADS = (4, 8)
SHIFTS = (0, 4)
FORMATS = ("mxfp4", "mxfp8_e4m3")


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
    qkv = torch.randn(B, HW, HW, 3 * C, generator=g).cuda().contiguous()
    out = []
    for heads in HEADS:
        bias = (2 * torch.randn(heads, WINDOW ** 2, WINDOW ** 2, generator=g)).cuda().contiguous()
        for shift in SHIFTS:
            d = ops.attn_desc(B, HW, HW, C, heads, WINDOW, shift)
            o32, omx = torch.empty(B, HW, HW, C, device="cuda"), torch.empty(B, HW, HW, C, device="cuda")
            for fmt in FORMATS:
                calls = {"fp32_attention": lambda: ops.window_attention(d, qkv, bias, out=o32),
                         "mx_attention": lambda: ops.mx_window_attention(d, qkv, bias, fmt, out=omx)}
                for fn in calls.values():                              # warm-up: code objects, the occupancy query
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                apart = float((omx - o32).abs().max() / o32.abs().max())
                t = {key: [] for key in calls}
                for _ in range(rounds):                                # alternate within one process
                    for key, fn in calls.items():
                        t[key].append(_time_us(fn, reps))
                med = {k: statistics.median(v) for k, v in t.items()}
                for what, v in t.items():
                    row = dict(shape=f"attn{B}x{HW}x{HW}x{C}", heads=heads, hd=C // heads, window=WINDOW, shift=shift, format=fmt, call=what,
                               us=round(med[what], 2), spread_us=[round(min(v), 2), round(max(v), 2)],
                               of_fp32=round(med[what] / med["fp32_attention"], 3), max_abs_apart_of_max=round(apart, 4), reps=reps, rounds=rounds)
                    out.append(row)
                    print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--log", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_attn needs a GPU: there is no CPU path to time")
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
