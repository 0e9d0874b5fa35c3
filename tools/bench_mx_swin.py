#!/usr/bin/env python3
"""The MX Swin kernels (`ops.mx_layer_norm_pack`, `ops.mx_swin_mlp`; csrc/mx_swin.hip) on one MI355X at the Lu2022 width C = 192 /
Hd = 384, 16 384 and 65 536 tokens, mxfp4 and mxfp8_e4m3 for activations and weights alike.  Per shape and format, from one process,
alternating:
  ln_composition   `ops.layer_norm` + `ops.mx_quant_pack`: what the norm1 -> qkv producer takes without the kernel (two launches)
  mx_ln_pack       `ops.mx_layer_norm_pack` (one launch)
  mlp_composition  the eight launches a switched-off block runs for t + fc2(gelu(fc1(norm2(t)))), t = x + a: add, layer_norm,
                   mx_quant_pack, mx_gemm, gelu, mx_quant_pack, mx_gemm, add
  mx_swin_mlp      `ops.mx_swin_mlp` (one launch)
A first measurement and a record, not a bar: what is to be seen is whether the one launch is below the composition by more than the
spread between windows of one call.

Device-event timing around `reps` calls after warm-up, `rounds` alternating windows; the median window is reported with its spread.
Before timing, the launch's bytes are compared with the composition's -- with `ops.add_layer_norm` as the LayerNorm, whose bits the
kernels keep -- on the timed shape: the packed operand and scale bytes of the producer and the fp32 output of the MLP must be equal
(`bits_equal`), or the run stops.

    python tools/bench_mx_swin.py [--reps 20] [--rounds 7] [--json out.json] [--log profiles/mx_swin_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

C, HD = 192, 384
TOKENS = (16384, 65536)
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
    for rows in TOKENS:
        x = (torch.randn(rows, C, generator=g) ** 3 * 0.3).cuda().contiguous()
        a = torch.randn(rows, C, generator=g).cuda().contiguous()
        lw, lb = (1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
        b1, b2 = (0.1 * torch.randn(HD, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
        W1, W2 = (torch.randn(HD, C, generator=g) * C ** -0.5).cuda(), (torch.randn(C, HD, generator=g) * HD ** -0.5).cuda()
        for fmt in FORMATS:
            w1, w2 = ops.mx_quant_pack(W1, fmt), ops.mx_quant_pack(W2, fmt)

            def mlp_composition(ln=ops.layer_norm):
                t = ops.add(x, a)
                h = ops.gelu(ops.mx_gemm(ops.mx_quant_pack(ln(t, lw, lb), fmt), w1, b1))
                return ops.add(t, ops.mx_gemm(ops.mx_quant_pack(h, fmt), w2, b2))

            same_ln = lambda t, w, b: ops.add_layer_norm(t, None, w, b)
            got, want = ops.mx_layer_norm_pack(x, None, lw, lb, fmt), ops.mx_quant_pack(same_ln(x, lw, lb), fmt)
            if not (torch.equal(got.packed, want.packed) and torch.equal(got.scales, want.scales)):
                raise SystemExit(f"{rows} tokens {fmt}: mx_layer_norm_pack's bytes are not the composition's")
            if not torch.equal(ops.mx_swin_mlp(x, a, lw, lb, w1, b1, w2, b2, fmt), mlp_composition(same_ln)):
                raise SystemExit(f"{rows} tokens {fmt}: mx_swin_mlp's output is not the composition's")
            del got, want
            calls = {"ln_composition": lambda: ops.mx_quant_pack(ops.layer_norm(x, lw, lb), fmt),
                     "mx_ln_pack": lambda: ops.mx_layer_norm_pack(x, None, lw, lb, fmt),
                     "mlp_composition": mlp_composition,
                     "mx_swin_mlp": lambda: ops.mx_swin_mlp(x, a, lw, lb, w1, b1, w2, b2, fmt)}
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
                base = med["ln_composition" if "ln" in what else "mlp_composition"]
                row = dict(shape=f"swin{C}x{HD}@{rows}", rows=rows, C=C, Hd=HD, format=fmt, call=what, us=round(med[what], 2),
                           spread_us=[round(min(v), 2), round(max(v), 2)], of_composition=round(med[what] / base, 3), reps=reps, rounds=rounds,
                           bits_equal=True)
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
        raise SystemExit("bench_mx_swin needs a GPU: there is no CPU path to time")
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
