#!/usr/bin/env python3
"""The per-channel rate sums of the RD report (`ops.neg_log2_channel_sums`, rdo_neg_log2_channel_sums of csrc/entropy.hip) on one
MI355X, on likelihood tensors of the sizes the coders return, stored NCHW and channels-last, next to the torch expression
`(-torch.log2(lik)).sum((0, 2, 3))` on the same box.

Device-event timing after warm-up, the kernel and the torch expression ALTERNATING in one process (kernel window, torch window, ...; the
median window is reported): µs per call, bytes / µs against the algorithmic bytes (one read: 4 B per element) and the share of the
6.3 TB/s a copy achieves (the achievable HBM rate of DESIGN.md section 5).  The latents are small: expect the launch latency of the
call's two launches, not the bandwidth, to set the time.

    python tools/bench_rate_channels.py [--reps 1000] [--rounds 7] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

SHAPES = [(8, 192, 16, 16), (8, 192, 4, 4), (1, 320, 48, 32)]
ACHIEVABLE_HBM_BYTES_PER_US = 6.3e6


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def bench(reps, rounds):
    from hipops import ops
    rows = []
    for shape in SHAPES:
        g = torch.Generator().manual_seed(sum(shape))
        nchw = torch.exp(torch.rand(*shape, generator=g) * -20.0).clamp(1e-9, 1.0).cuda().contiguous()
        for layout, lik in (("nchw", nchw), ("channels_last", nchw.contiguous(memory_format=torch.channels_last))):
            out = torch.empty(shape[1], device="cuda")
            calls = {"kernel": lambda: ops.neg_log2_channel_sums(lik, out=out), "torch": lambda: (-torch.log2(lik)).sum((0, 2, 3))}
            for fn in calls.values():                              # warm-up: code objects, caches
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in calls}
            for _ in range(rounds):                                # alternate within one process
                for k, fn in calls.items():
                    t[k].append(_time_us(fn, reps))
            want = calls["torch"]()
            torch.testing.assert_close(ops.neg_log2_channel_sums(lik), want, rtol=1e-4, atol=1e-3)
            med = {k: statistics.median(v) for k, v in t.items()}
            nbytes = 4.0 * lik.numel()
            row = dict(shape=list(shape), layout=layout, elements=lik.numel(), reps=reps, rounds=rounds)
            for k in calls:
                rate = nbytes / med[k]
                row.update({f"{k}_us": round(med[k], 2), f"{k}_spread_us": [round(min(t[k]), 2), round(max(t[k]), 2)],
                            f"{k}_bytes_per_us": round(rate, 1), f"{k}_share_of_achievable_hbm": round(rate / ACHIEVABLE_HBM_BYTES_PER_US, 4)})
            row["torch_over_kernel"] = round(med["torch"] / med["kernel"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=1000, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rate_channels needs a GPU: there is no CPU path to time")
    rows = bench(a.reps, a.rounds)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rate_channels": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
