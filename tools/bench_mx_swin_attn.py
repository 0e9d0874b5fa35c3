#!/usr/bin/env python3
"""The one-launch attention half of an MX Swin block (`ops.mx_swin_attn`; csrc/mx_swin_attn.hip) on one MI355X against the five launches
it replaces, at the Lu2022 width: B = 4, a 128 x 128 map, C = 192, 8 heads of 24, window 8, shift 0 and 4, mxfp8_e4m3 and mxfp4 for
activations and weights alike.  Per shift and format, from one process, alternating:
  five_launches   `ops.mx_layer_norm_pack`, `ops.mx_gemm` (qkv), `ops.mx_window_attention`, `ops.mx_quant_pack`, `ops.mx_gemm` (proj): what a
                  block switched with swin=True, attention=True runs up to the attention branch a (its residual add is inside the MLP launch)
  mx_swin_attn    `ops.mx_swin_attn` (one launch, x + a)
A first measurement and a record, not a bar: no ratio is promised.

Device-event timing around `reps` calls after warm-up, `rounds` alternating windows; the median window is reported with its spread.
Before timing, x + a of the five launches (`ops.add`) is compared with the launch's output on the timed shape: they must be equal
(`bits_equal`), or the run stops.

    python tools/bench_mx_swin_attn.py [--reps 20] [--rounds 7] [--json out.json] [--log profiles/mx_swin_attn_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

B, H, W, C, HEADS, WINDOW = 4, 128, 128, 192, 8, 8
SHIFTS = (0, 4)
FORMATS = ("mxfp8_e4m3", "mxfp4")


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
    rows, N = B * H * W, WINDOW * WINDOW
    x = (torch.randn(rows, C, generator=g) ** 3 * 0.3).cuda().contiguous()
    lw, lb = (1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    bqkv, bproj = (0.1 * torch.randn(3 * C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    Wqkv, Wproj = (torch.randn(3 * C, C, generator=g) * C ** -0.5).cuda(), (torch.randn(C, C, generator=g) * C ** -0.5).cuda()
    bias = (2 * torch.randn(HEADS, N, N, generator=g)).cuda()
    out = []
    for shift in SHIFTS:
        d = ops.attn_desc(B, H, W, C, HEADS, WINDOW, shift)
        for fmt in FORMATS:
            wqkv, wproj = ops.mx_quant_pack(Wqkv, fmt), ops.mx_quant_pack(Wproj, fmt)

            def five_launches():
                qkv = ops.mx_gemm(ops.mx_layer_norm_pack(x, None, lw, lb, fmt), wqkv, bqkv)
                o = ops.mx_window_attention(d, qkv.view(B, H, W, 3 * C), bias, fmt)
                return ops.mx_gemm(ops.mx_quant_pack(o.view(rows, C), fmt), wproj, bproj)

            fused = lambda: ops.mx_swin_attn(d, x, lw, lb, wqkv, bqkv, wproj, bproj, bias, fmt)
            if not torch.equal(fused(), ops.add(x, five_launches())):
                raise SystemExit(f"shift {shift} {fmt}: mx_swin_attn's output is not x + the five launches'")
            calls = {"five_launches": five_launches, "mx_swin_attn": fused}
            for fn in calls.values():                                  # warm-up: code objects, the allocator's blocks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {key: [] for key in calls}
            for _ in range(rounds):                                    # alternate within one process
                for key, fn in calls.items():
                    t[key].append(_time_us(fn, reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            for what, v in t.items():
                row = dict(shape=f"swin_attn{C}h{HEADS}w{WINDOW}s{shift}@{B}x{H}x{W}", shift=shift, format=fmt, call=what, us=round(med[what], 2),
                           spread_us=[round(min(v), 2), round(max(v), 2)], of_five_launches=round(med[what] / med["five_launches"], 3),
                           reps=reps, rounds=rounds, bits_equal=True)
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
        raise SystemExit("bench_mx_swin_attn needs a GPU: there is no CPU path to time")
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
