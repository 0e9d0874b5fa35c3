#!/usr/bin/env python3
"""The packed-output MX convolution (`ops.mx_conv2d(..., out_fmt=, act=)`; csrc/mx_chain.hip) on one MI355X against the three launches it
replaces -- `ops.mx_conv2d` -> `ops.lrelu` -> `ops.mx_quant_pack` --, on the shapes of tools/bench_mx_conv.py at batch 4: 3x3 192 -> 192
stride 1 at 128^2 and at 64^2, 5x5 192 -> 192 stride 2 on a 128^2 input, with mxfp4 x mxfp4 and mxfp8_e4m3 x mxfp8_e4m3 (the output in
the activations' format).  Per shape and format: the packed launch, the three launches in sequence and each of the three alone, and
the conv1 -> conv2 pair (a second 3x3 stride-1 192 -> 192 on the first's output) chained -- packed launch, fp32 conv -- and un-chained
-- the three launches, fp32 conv --, all from one process, alternating.  Before timing, the packed launch's bytes are compared with the
three launches': a difference stops the run.

Device-event timing around `reps` calls after warm-up; 7 alternating windows, the median is reported with the spread.

    python tools/bench_mx_chain.py [--reps 20] [--rounds 7] [--log profiles/mx_chain_bench.log]"""
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
SHAPES = (("cheng.3x3@128", 128, 192, 192, 3, 1, 1), ("cheng.3x3@64", 64, 192, 192, 3, 1, 1), ("5x5s2@128", 128, 192, 192, 5, 2, 2))
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
    out = []
    for name, S, C, N, k, stride, pad in SHAPES:
        B, H, W = BATCH, S, S
        So = (S + 2 * pad - k) // stride + 1
        x = (torch.randn(B * H * W, C, generator=g) ** 3 * 0.1).cuda().contiguous()
        w1 = (torch.randn(N, k * k * C, generator=g) * 0.05).cuda().contiguous()
        w2 = (torch.randn(N, 9 * N, generator=g) * 0.05).cuda().contiguous()
        bias = (torch.randn(N, generator=g) * 0.01).cuda()
        calls = {}
        for fmt in FORMATS:
            def operand(w, fmt=fmt):
                q = ops.mx_fakequant(w, fmt, want=("codes", "scales"))
                return ops.mx_pack_codes(q["codes"], q["scales"], fmt)
            a, b1, b2 = ops.mx_quant_pack(x, fmt), operand(w1), operand(w2)
            conv = lambda a=a, b1=b1: ops.mx_conv2d(a, b1, (B, H, W), k, stride, pad, bias)
            packed = lambda a=a, b1=b1, fmt=fmt: ops.mx_conv2d(a, b1, (B, H, W), k, stride, pad, bias, out_fmt=fmt, act="lrelu")
            three = lambda conv=conv, fmt=fmt: ops.mx_quant_pack(ops.lrelu(conv()).reshape(-1, N), fmt)
            second = lambda mid, b2=b2: ops.mx_conv2d(mid, b2, (B, So, So), 3, 1, 1, bias)
            got, want = packed(), three()
            if not (torch.equal(got.packed, want.packed) and torch.equal(got.scales, want.scales)):
                raise SystemExit(f"{name} {fmt}: the packed launch and the three launches differ")
            y = conv()
            calls[fmt, "conv2d_packed"] = packed
            calls[fmt, "conv2d+lrelu+quant_pack"] = three
            calls[fmt, "conv2d"] = conv
            calls[fmt, "lrelu"] = lambda y=y: ops.lrelu(y)
            calls[fmt, "quant_pack"] = lambda y=y, fmt=fmt: ops.mx_quant_pack(y.reshape(-1, N), fmt)
            calls[fmt, "pair.chained"] = lambda packed=packed, second=second: second(packed())
            calls[fmt, "pair.unchained"] = lambda three=three, second=second: second(three())
            del got, want
        for fn in calls.values():                                  # warm-up: code objects, the allocator's blocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {key: [] for key in calls}
        for _ in range(rounds):                                    # alternate within one process
            for key, fn in calls.items():
                t[key].append(_time_us(fn, reps))
        for (fmt, what), v in t.items():
            row = dict(shape=name, B=B, H=H, W=W, C=C, N=N, k=k, stride=stride, pad=pad, M=B * So * So, format=fmt, call=what,
                       us=round(statistics.median(v), 2), spread_us=[round(min(v), 2), round(max(v), 2)], reps=reps, rounds=rounds)
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--log", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_chain needs a GPU: there is no CPU path to time")
    rows = run(a.reps, a.rounds)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
