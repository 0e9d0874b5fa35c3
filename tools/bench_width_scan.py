#!/usr/bin/env python3
"""The width scan of the bit allocation (`ops.uaq_width_scan`, rdo_uaq_width_scan of csrc/bit_alloc.hip) on one MI355X with K = 4
widths, over every weight tensor of Cheng2020-anchor N = 192 as its weight quantiser sees it (channel-wise rows; --per-tensor: each
weight as ONE row, the split path), next to the sequence it replaces on the same tensors: K x (`ops.uaq_init_minmax` +
`ops.uaq_fakequant` + a torch reduction of (w - wq)^2 in float64) and one torch reduction for the energy.

Device-event timing after warm-up, the two ALTERNATING in one process (scan window, sequence window, ...; the median window is
reported): µs per pass over all tensors, and the weight bytes of one read over the scan's time.

    python tools/bench_width_scan.py [--reps 20] [--rounds 7] [--per-tensor] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

WIDTHS = (4, 5, 6, 8)


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def weight_rows(per_tensor):
    """the row matrices [rows, inner] of every weighted QuantModule of Cheng2020-anchor N = 192 (random init: the time does not depend on
    the values)"""
    import lic
    from quantization import QuantModel, QuantModule
    torch.manual_seed(1005)
    wq = {"n_bits": 8, "channel_wise": not per_tensor, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(lic.Cheng2020Anchor(N=192).cuda().eval(), wq, aq, is_cheng=True).cuda().eval()
    out = []
    for m in qnn.modules():
        if isinstance(m, QuantModule) and m.org_weight is not None:
            wr = m.weight_quantizer._rows(m.weight.detach())
            out.append(wr.reshape(wr.shape[0], -1).contiguous())
    return out


def bench(reps, rounds, per_tensor):
    from hipops import ops
    mats = weight_rows(per_tensor)
    descs = {b: [ops.ada_desc(w, 2 ** b, conv_layout=False) for w in mats] for b in WIDTHS}

    def scan():
        for w in mats:
            ops.uaq_width_scan(w, WIDTHS)

    def sequence():
        for i, w in enumerate(mats):
            (w.double() ** 2).sum(1)
            for b in WIDTHS:
                d, z = ops.uaq_init_minmax(w, 2 ** b)
                wq = ops.uaq_fakequant(descs[b][i], w, d, z)
                ((w - wq).double() ** 2).sum(1)

    calls = {"scan": scan, "sequence": sequence}
    for fn in calls.values():                                      # warm-up: code objects, workspaces, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in calls}
    for _ in range(rounds):                                        # alternate within one process
        for name, fn in calls.items():
            t[name].append(_time_us(fn, reps))
    med = {name: statistics.median(v) for name, v in t.items()}
    nbytes = 4.0 * sum(w.numel() for w in mats)
    row = dict(model="Cheng2020Anchor N=192", per_tensor=per_tensor, tensors=len(mats), widths=list(WIDTHS), mbytes=round(nbytes / 2 ** 20, 2),
               split_rows=sum(1 for w in mats if w.shape[1] > 8192), reps=reps, rounds=rounds)
    for name in calls:
        row.update({f"{name}_us": round(med[name], 1), f"{name}_spread_us": [round(min(t[name]), 1), round(max(t[name]), 1)]})
    row["scan_bytes_per_us"] = round(nbytes / med["scan"], 1)
    row["speedup"] = round(med["sequence"] / med["scan"], 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="passes over all tensors per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--per-tensor", action="store_true", help="each weight as one row (a per-tensor quantiser): the split path")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_width_scan needs a GPU: there is no CPU path to time")
    row = bench(a.reps, a.rounds, a.per_tensor)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"width_scan": row}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
