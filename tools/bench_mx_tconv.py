#!/usr/bin/env python3
"""The native MX transposed convolution (`ops.mx_quant_pack` + `ops.mx_conv_transpose2d`; csrc/mx_tconv.hip) on one MI355X, on the
synthesis deconv of the image coders at batch 4: 5x5 192 -> 192 stride 2 (padding 2, output padding 1) from a 64^2 and from a 128^2
input, with mxfp8_e4m3 x mxfp8_e4m3 and mxfp4 x mxfp4 (activations x weights).  Per shape and format: the producer alone, the transposed
convolution alone, both in sequence (what `mx.native_tconv` launches), and `ops.conv_transpose2d` -- the kernels the modules' own
forward runs -- on the same shape from the same process, alternating.  A first measurement and a record, not a bar.

Device-event timing around `reps` calls after warm-up; the median window is reported, with the spread.  Two floors per row:
`flop_floor_us` is 2 x (input pixels) x N x k k C -- every input pixel meets every tap once; the borders are not taken off -- over the
dense peak of the format's block-scaled instruction (10 PF for FP4, 5 PF for FP8; a pair with an FP8 operand issues eight instructions
per K step, which the floor does not count; none for the producer, and the fp32 kernels are given no flop floor), `byte_floor_us` the
bytes the call has to move (fp32 pixels in, packed rows and scales out; packed operands, scales and bias in, fp32 out) at the 6.3 TB/s
a copy achieves; `bound` names the larger, `floor_share` = it / time.  Before timing, the native result is
compared with `conv_transpose2d` on the decoded operands: `rel_l2` of every row; a relative L2 of 1e-3 or more (a wrong layout gives
O(1)) stops the run.

    python tools/bench_mx_tconv.py [--reps 20] [--rounds 7] [--json out.json] [--log profiles/mx_tconv_bench.log]"""
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
SHAPES = (("deconv5x5s2@64", 64, 192, 192, 5, 2, 2, 1), ("deconv5x5s2@128", 128, 192, 192, 5, 2, 2, 1))
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
    for name, S, C, N, k, stride, pad, opad in SHAPES:
        B, H, W = BATCH, S, S
        So = (S - 1) * stride - 2 * pad + k + opad
        M, K = B * So * So, k * k * C
        x = (torch.randn(B, H, W, C, generator=g) ** 3 * 0.1).cuda().contiguous()
        w = (torch.randn(N, K, generator=g) * 0.05).cuda().contiguous()
        bias = (torch.randn(N, generator=g) * 0.01).cuda()
        rows = x.reshape(-1, C)
        fp_pack = ops.WeightPack(w.reshape(N, k, k, C), bias)
        rels = {}
        calls = {("conv_transpose2d", "fp32"): lambda: ops.conv_transpose2d(x, None, None, stride, pad, opad, epilogue=L.EPI_NONE, pack=fp_pack)}
        floors = {("conv_transpose2d", "fp32"): (0.0, (B * H * W * C * 4 + N * K * 4 + N * 4 + M * N * 4) / HBM_BYTES_PER_US)}
        for fmt in FORMATS:
            bits = L.MX_FORMATS[fmt][1]
            q = ops.mx_fakequant(w, fmt, want=("codes", "scales", "wq"))
            b = ops.mx_pack_codes(q["codes"], q["scales"], fmt)
            a, xq = ops.mx_quant_pack(rows, fmt, want_xq=True)
            native = ops.mx_conv_transpose2d(a, b, (B, H, W), k, stride, pad, opad, bias)
            emulated = ops.conv_transpose2d(xq.reshape(B, H, W, C), None, None, stride, pad, opad, epilogue=L.EPI_NONE,
                                            pack=ops.WeightPack(q["wq"].reshape(N, k, k, C), bias))
            rel = float((native - emulated).double().norm() / emulated.double().norm())
            if not rel < 1e-3:
                raise SystemExit(f"{name} {fmt}: native and emulated transposed convolutions differ, relative L2 {rel:.3e}")
            del native, emulated, xq
            packed = lambda r, inner: r * inner * bits / 8 + r * inner / 32
            rels[fmt] = rel
            calls[fmt, "quant_pack"] = lambda fmt=fmt: ops.mx_quant_pack(rows, fmt)
            calls[fmt, "conv_transpose2d"] = lambda a=a, b=b: ops.mx_conv_transpose2d(a, b, (B, H, W), k, stride, pad, opad, bias)
            calls[fmt, "quant_pack+conv_transpose2d"] = lambda fmt=fmt, b=b: ops.mx_conv_transpose2d(ops.mx_quant_pack(rows, fmt), b, (B, H, W), k,
                                                                                                     stride, pad, opad, bias)
            flop = 2.0 * B * H * W * N * K / PEAK_FLOP_PER_US[fmt]
            floors[fmt, "quant_pack"] = (0.0, (B * H * W * C * 4 + packed(B * H * W, C)) / HBM_BYTES_PER_US)
            floors[fmt, "conv_transpose2d"] = (flop, (packed(B * H * W, C) + packed(N, K) + N * 4 + M * N * 4) / HBM_BYTES_PER_US)
            floors[fmt, "quant_pack+conv_transpose2d"] = (flop, floors[fmt, "quant_pack"][1] + floors[fmt, "conv_transpose2d"][1])
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
            row = dict(shape=name, B=B, H=H, W=W, C=C, N=N, k=k, stride=stride, pad=pad, output_padding=opad, M=M, K=K, format=fmt, call=what,
                       us=round(statistics.median(v), 2), spread_us=[round(min(v), 2), round(max(v), 2)], reps=reps, rounds=rounds,
                       flop_floor_us=round(flop_us, 2), byte_floor_us=round(byte_us, 2), bound="flops" if flop_us > byte_us else "bytes")
            row["floor_share"] = round(max(flop_us, byte_us) / row["us"], 3)
            if fmt in rels:
                row["rel_l2"] = float(f"{rels[fmt]:.3e}")
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
        raise SystemExit("bench_mx_tconv needs a GPU: there is no CPU path to time")
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
