#!/usr/bin/env python3
"""The tap sums of the bias correction (`ops.tap_sums`, rdo_tap_sums of csrc/bias_correct.hip) on one MI355X, next to
`ops.pair_moments` (rdo_pair_moments of csrc/actquant.hip) on the SAME tensor (pair_moments reads it twice: against a second tensor
of the same size), on layer inputs of the sizes calibration meets.

Device-event timing after warm-up, the two kernels ALTERNATING in one process (tap_sums window, pair_moments window, ...; the median
window is reported): µs per call, bytes read per µs (tap_sums: 4 B per element once; pair_moments: two tensors) and the ratio of the
two rates.  The aim is the same achieved bytes per second; one input stream keeps half as many loads in flight per lane as
pair_moments' two, so 0.7 x is accepted on the aligned shapes of 32 MB and more.

    python tools/bench_tap_sums.py [--reps 200] [--rounds 7] [--only INDEX] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

# (shape, k, stride, pad)
SHAPES = [((32, 128, 128, 192), 3, 1, 1), ((4, 128, 128, 192), 3, 1, 1), ((32, 256, 256, 3), 3, 2, 1), ((65536, 192), 1, 1, 0),
          ((32, 16, 16, 320), 5, 1, 2)]


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def bench(reps, rounds, only=None):
    from hipops import ops
    rows = []
    for shape, k, s, p in (SHAPES if only is None else [SHAPES[only]]):
        g = torch.Generator(device="cuda").manual_seed(sum(shape))
        x = torch.randn(*shape, generator=g, device="cuda")
        y = x + 0.01 * torch.randn(*shape, generator=g, device="cuda")
        hw = None if x.dim() != 4 else (ops.tap_out_size(shape[1], k, s, p), ops.tap_out_size(shape[2], k, s, p))
        tout = torch.zeros(k * k, shape[-1], device="cuda")
        pout = torch.zeros(3, shape[-1], device="cuda")
        calls = {"tap_sums": lambda: ops.tap_sums(x, k, s, p, hw, out=tout), "pair_moments": lambda: ops.pair_moments(x, y, out=pout)}
        for fn in calls.values():                                  # warm-up: code objects, workspaces, caches
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in calls}
        for _ in range(rounds):                                    # alternate within one process
            for name, fn in calls.items():
                t[name].append(_time_us(fn, reps))
        med = {name: statistics.median(v) for name, v in t.items()}
        nbytes = {"tap_sums": 4.0 * x.numel(), "pair_moments": 8.0 * x.numel()}
        row = dict(shape=list(shape), k=k, stride=s, pad=p, mbytes=round(4.0 * x.numel() / 2 ** 20, 1), vector_path=shape[-1] % 4 == 0,
                   reps=reps, rounds=rounds)
        for name in calls:
            row.update({f"{name}_us": round(med[name], 2), f"{name}_spread_us": [round(min(t[name]), 2), round(max(t[name]), 2)],
                        f"{name}_bytes_per_us": round(nbytes[name] / med[name], 1)})
        row["rate_ratio"] = round(row["tap_sums_bytes_per_us"] / row["pair_moments_bytes_per_us"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run (under a kernel trace: one shape per process)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tap_sums needs a GPU: there is no CPU path to time")
    rows = bench(a.reps, a.rounds, a.only)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"tap_sums": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
