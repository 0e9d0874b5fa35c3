#!/usr/bin/env python3
"""The native MX path (`ops.mx_quant_pack` + `ops.mx_gemm`; csrc/mx_gemm.hip) on one MI355X, on the token-matrix Linears of the Lu2022
codec at a 4 x 64 x 64 feature map (16384 tokens): qkv 192 -> 576 and the MLP pair 192 -> 768 -> 192, with mxfp8_e4m3 x mxfp8_e4m3 and
mxfp4 x mxfp4 (activations x weights).  Per layer and format: the producer alone, the GEMM alone, both in sequence (what
`mx.native_linear` launches), and `ops.linear_h2` -- the split-fp16 kernel the modules' own forward runs -- on the same shape from the
same process, alternating.  A record, not a bar: nobody has tuned this path, and the fp32 output write bounds it.

Device-event timing around `reps` calls after warm-up; the median window is reported, with the spread.  `floor_us` is the time of the
bytes the call has to move (fp32 rows in, packed rows and scales out; packed operands, scales and bias in, fp32 out) at the 6.3 TB/s a
copy achieves; `floor_share` = floor / time.  Before timing, the native product is compared with the split-fp16
kernel on the decoded operands: `rel_l2` of every row; a relative L2 of 1e-3 or more (a wrong layout gives O(1)) stops the run.

    python tools/bench_mx_gemm.py [--reps 200] [--rounds 7] [--json out.json] [--log profiles/mx_gemm_bench.log]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

TOKENS = 4 * 64 * 64
LAYERS = (("qkv", 192, 576), ("mlp.fc1", 192, 768), ("mlp.fc2", 768, 192))
FORMATS = ("mxfp8_e4m3", "mxfp4")
HBM_BYTES_PER_US = 6.3e6          # achievable HBM: what a device-to-device copy reaches


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
    for layer, K, N in LAYERS:
        x = (torch.randn(TOKENS, K, generator=g) ** 3 * 0.1).cuda().contiguous()
        w = (torch.randn(N, K, generator=g) * 0.05).cuda().contiguous()
        bias = (torch.randn(N, generator=g) * 0.01).cuda()
        planes = ops.split_h2_linear(w)
        y_h2 = torch.empty(TOKENS, N, device="cuda")
        rels = {}
        calls, floors = {("linear_h2", "fp32"): lambda: ops.linear_h2(x, planes, bias, out=y_h2)}, {}
        floors["linear_h2", "fp32"] = (TOKENS * K * 4 + N * K * 4 + TOKENS * N * 4) / HBM_BYTES_PER_US
        for fmt in FORMATS:
            bits = L.MX_FORMATS[fmt][1]
            q = ops.mx_fakequant(w, fmt, want=("codes", "scales", "wq"))
            b = ops.mx_pack_codes(q["codes"], q["scales"], fmt)
            a, xq = ops.mx_quant_pack(x, fmt, want_xq=True)
            native = ops.mx_gemm(a, b, bias)
            emulated = ops.linear_h2(xq, ops.split_h2_linear(q["wq"]), bias)
            rel = float((native - emulated).double().norm() / emulated.double().norm())
            if not rel < 1e-3:
                raise SystemExit(f"{layer} {fmt}: native and emulated products differ, relative L2 {rel:.3e}")
            packed = lambda r: r * K * bits / 8 + r * K / 32
            rels[fmt] = rel
            calls[fmt, "quant_pack"] = lambda fmt=fmt: ops.mx_quant_pack(x, fmt)
            calls[fmt, "gemm"] = lambda a=a, b=b: ops.mx_gemm(a, b, bias)
            calls[fmt, "quant_pack+gemm"] = lambda fmt=fmt, b=b: ops.mx_gemm(ops.mx_quant_pack(x, fmt), b, bias)
            floors[fmt, "quant_pack"] = (TOKENS * K * 4 + packed(TOKENS)) / HBM_BYTES_PER_US
            floors[fmt, "gemm"] = (packed(TOKENS) + packed(N) + N * 4 + TOKENS * N * 4) / HBM_BYTES_PER_US
            floors[fmt, "quant_pack+gemm"] = floors[fmt, "quant_pack"] + floors[fmt, "gemm"]
        for fn in calls.values():                                  # warm-up: code objects, the allocator's blocks
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {key: [] for key in calls}
        for _ in range(rounds):                                    # alternate within one process
            for key, fn in calls.items():
                t[key].append(_time_us(fn, reps))
        for (fmt, what), v in t.items():
            row = dict(layer=layer, rows=TOKENS, K=K, N=N, format=fmt, call=what, us=round(statistics.median(v), 2),
                       spread_us=[round(min(v), 2), round(max(v), 2)], reps=reps, rounds=rounds)
            row["floor_us"] = round(floors[fmt, what], 2)
            row["floor_share"] = round(row["floor_us"] / row["us"], 3)
            if fmt in rels:
                row["rel_l2"] = float(f"{rels[fmt]:.3e}")
            out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--log", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_gemm needs a GPU: there is no CPU path to time")
    rows = run(a.reps, a.rounds)
    lines = [json.dumps(r) for r in rows]
    print("\n".join(lines), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
