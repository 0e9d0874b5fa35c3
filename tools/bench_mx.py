#!/usr/bin/env python3
"""The MX quantise kernel (`ops.mx_fakequant`; mx_fakequant_kernel of csrc/mx_quant.hip) on one MI355X: a call's time on two weight-row
matrices of the flagship codec ([192, 1728]: a 3x3 192 -> 192 conv; [768, 640]) and on an activation-shaped operand ([65536, 192]: the
pixels of a 256 x 256 feature map of 192 channels), in each of the five formats, with 'wq' only (written into a buffer made once) and
with all five outputs, all in one process and alternating.  Next to them a device-to-device copy of the operand (one read and one
write of the same bytes).  A record, not a bar: nobody has tuned this kernel.

Device-event timing around `reps` calls of the wrapper after warm-up (so a small operand measures the host's enqueue rate, not the
kernel); the median window is reported, with the spread.  The byte floor is 4 B read + 4 B written per element (+ 1 B with the codes)
at the 6.3 TB/s a copy achieves; `floor_share` = floor / time.  The 'wq' of every format is compared with the
all-outputs call and with `ops.mx_dequant` of its codes first (bit for bit).

    python tools/bench_mx.py [--reps 300] [--rounds 7] [--json out.json] [--log profiles/mx_quant_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

SHAPES = ((192, 1728), (768, 640), (65536, 192))
ALL = ("wq", "scales", "codes", "err", "energy")
HBM_BYTES_PER_US = 6.3e6          # achievable HBM: what a device-to-device copy reaches


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def floor_us(rows, inner, codes):
    return rows * inner * (9.0 if codes else 8.0) / HBM_BYTES_PER_US


def run(reps, rounds):
    from hipops import _lib as L
    from hipops import ops
    g = torch.Generator().manual_seed(1005)
    out = []
    for rows, inner in SHAPES:
        w = (torch.randn(rows, inner, generator=g) ** 3 * 0.01).cuda().contiguous()
        dst, copy = torch.empty_like(w), torch.empty_like(w)
        calls = {("copy_d2d", "-"): lambda: copy.copy_(w)}
        for fmt in L.MX_FORMATS:
            full = ops.mx_fakequant(w, fmt, want=ALL)
            same = torch.equal(ops.mx_fakequant(w, fmt, wq_out=dst)["wq"].view(torch.int32), full["wq"].view(torch.int32)) and \
                torch.equal(ops.mx_dequant(full["codes"], full["scales"], inner, fmt).view(torch.int32), full["wq"].view(torch.int32))
            if not same:
                raise SystemExit(f"{fmt} on {(rows, inner)}: the calls do not give the same wq")
            calls[fmt, "wq"] = lambda fmt=fmt: ops.mx_fakequant(w, fmt, wq_out=dst)
            calls[fmt, "all"] = lambda fmt=fmt: ops.mx_fakequant(w, fmt, want=ALL)
        for fn in calls.values():                                  # warm-up: code objects, the workspace, the allocator's blocks
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {key: [] for key in calls}
        for _ in range(rounds):                                    # alternate within one process
            for key, fn in calls.items():
                t[key].append(_time_us(fn, reps))
        for (fmt, mode), v in t.items():
            row = dict(rows=rows, inner=inner, format=fmt, outputs=mode, us=round(statistics.median(v), 2),
                       spread_us=[round(min(v), 2), round(max(v), 2)], reps=reps, rounds=rounds)
            row["floor_us"] = round(floor_us(rows, inner, mode == "all"), 2)
            row["floor_share"] = round(row["floor_us"] / row["us"], 3)
            out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=300, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--log", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx needs a GPU: there is no CPU path to time")
    rows = run(a.reps, a.rounds)
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
