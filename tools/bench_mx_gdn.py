#!/usr/bin/env python3
"""The one-launch MX GDN / IGDN (`ops.mx_gdn`; csrc/mx_gdn.hip) on one MI355X, at the GDN shapes of the image coders at batch 4:
C = 192 on 64^2 and 128^2 pixels (rows = 4 * 64^2, 4 * 128^2), GDN and IGDN, with mxfp8_e4m3 and mxfp4 for both x o x and gamma'.  Per
shape, direction and format, from one process, alternating:
  fp32_gdn      the GDN forward the modules run today (`ops.conv2d_fwd_pack` with EPI_GDN / EPI_IGDN, square_input=True)
  composition   what the entries before this kernel take for the same result: x * x, `ops.mx_quant_pack`, `ops.mx_gemm`, x * n^-+1/2
  mx_gdn        the new launch with the fp32 output
  mx_gdn_packed the new launch with the output packed in the same format
A first measurement and a record, not a bar.

Device-event timing around `reps` calls after warm-up; the median window is reported, with the spread.  `flop_floor_us` is 2 rows C C
over the dense peak of the format's block-scaled instruction (10 PF for FP4, 5 PF for FP8; a pair with an FP8 operand issues eight
instructions per K step, which the floor does not count; the fp32 kernel is given none), `byte_floor_us` the bytes the call has to move
(x in, y out -- fp32 or packed --, gamma' and beta' in; the composition's fp32 round trips are NOT in its floor: it is given the
floor of the one launch, so `floor_share` compares like with like) at the 6.3 TB/s a copy achieves; `bound` names
the larger, `floor_share` = it / time.  Before timing, the launch is compared with the composition: the norm and y must be equal bits
(`bits_equal`), or the run stops.

    python tools/bench_mx_gdn.py [--reps 20] [--rounds 7] [--json out.json] [--log profiles/mx_gdn_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

BATCH, C = 4, 192
SIDES = (64, 128)
FORMATS = ("mxfp8_e4m3", "mxfp4")
HBM_BYTES_PER_US = 6.3e6          # achievable HBM: what a device-to-device copy reaches
PEAK_FLOP_PER_US = {"mxfp8_e4m3": 5e9, "mxfp4": 10e9}      # dense peak of the block-scaled instruction per element format


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def run(reps, rounds):
    from hipops import _lib as L
    from hipops import ops
    g = torch.Generator().manual_seed(1005)
    out = []
    for S in SIDES:
        rows = BATCH * S * S
        x = (torch.randn(rows, C, generator=g) ** 3 * 0.3).cuda().contiguous()
        gamma = (torch.randn(C, C, generator=g).abs() * 0.02 + 0.1 * torch.eye(C)).cuda().contiguous()
        beta = (torch.rand(C, generator=g) + 0.5).cuda()
        x4 = x.reshape(BATCH, S, S, C)
        fp_pack = ops.WeightPack(gamma.reshape(C, 1, 1, C), beta)
        for inverse in (False, True):
            epi = L.EPI_IGDN if inverse else L.EPI_GDN
            power = 0.5 if inverse else -0.5

            def composition(fmt, gq):
                n = ops.mx_gemm(ops.mx_quant_pack(x * x, fmt), gq, beta)
                return x * (torch.sqrt(n) if inverse else torch.rsqrt(n)), n

            calls = {("fp32", "fp32_gdn"): lambda: ops.conv2d_fwd_pack(x4, fp_pack, 1, 0, epilogue=epi, aux=x4, square_input=True)}
            floors = {("fp32", "fp32_gdn"): (0.0, (rows * C * 8 + C * C * 4 + C * 4) / HBM_BYTES_PER_US)}
            for fmt in FORMATS:
                bits = L.MX_FORMATS[fmt][1]
                gq = ops.mx_quant_pack(gamma, fmt)
                y, n = ops.mx_gdn(x, gq, beta, fmt, inverse=inverse, want_norm=True)
                n_ref = ops.mx_gemm(ops.mx_quant_pack(x * x, fmt), gq, beta)
                if not torch.equal(n, n_ref):
                    raise SystemExit(f"{S}^2 {fmt} inverse={inverse}: the launch's norm is not the composition's")
                rel = float((y.double() - x.double() * n.double() ** power).norm() / y.double().norm())
                if not rel < 1e-6:
                    raise SystemExit(f"{S}^2 {fmt} inverse={inverse}: y is off its float64 reference, relative L2 {rel:.3e}")
                del y, n, n_ref
                packed = lambda r, inner: r * inner * bits / 8 + r * inner / 32
                calls[fmt, "composition"] = lambda fmt=fmt, gq=gq: composition(fmt, gq)
                calls[fmt, "mx_gdn"] = lambda fmt=fmt, gq=gq: ops.mx_gdn(x, gq, beta, fmt, inverse=inverse)
                calls[fmt, "mx_gdn_packed"] = lambda fmt=fmt, gq=gq: ops.mx_gdn(x, gq, beta, fmt, inverse=inverse, out_fmt=fmt)
                flop = 2.0 * rows * C * C / PEAK_FLOP_PER_US[fmt]
                fixed = packed(C, C) + C * 4
                floors[fmt, "composition"] = floors[fmt, "mx_gdn"] = (flop, (rows * C * 8 + fixed) / HBM_BYTES_PER_US)
                floors[fmt, "mx_gdn_packed"] = (flop, (rows * C * 4 + packed(rows, C) + fixed) / HBM_BYTES_PER_US)
            for fn in calls.values():                                  # warm-up: code objects, the allocator's blocks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t = {key: [] for key in calls}
            for _ in range(rounds):                                    # alternate within one process
                for key, fn in calls.items():
                    t[key].append(_time_us(fn, reps))
            for (fmt, what), v in t.items():
                flop_us, byte_us = floors[fmt, what]
                row = dict(shape=f"gdn{C}@{S}", B=BATCH, H=S, W=S, C=C, rows=rows, inverse=int(inverse), format=fmt, call=what,
                           us=round(statistics.median(v), 2), spread_us=[round(min(v), 2), round(max(v), 2)], reps=reps, rounds=rounds,
                           flop_floor_us=round(flop_us, 2), byte_floor_us=round(byte_us, 2), bound="flops" if flop_us > byte_us else "bytes")
                row["floor_share"] = round(max(flop_us, byte_us) / row["us"], 3)
                if fmt != "fp32":
                    row["bits_equal"] = True
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
        raise SystemExit("bench_mx_gdn needs a GPU: there is no CPU path to time")
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
