#!/usr/bin/env python3
"""The pack / unpack kernels of the packed checkpoint (`ops.weight_pack`, `ops.weight_unpack`; csrc/weight_pack.hip) on one MI355X, on
a 192 x 1728 weight (a 3 x 3 192 -> 192 convolution as its weight quantiser sees it) at widths 3 and 8, next to a device-to-device
copy of the same input bytes (the fp32 weight), all in one process and alternating; then the wall time of `save_packed` and
`load_packed` on the toy Cheng2020 (N = 8) of the test suite.  A record, not a bar: the kernels are launch-latency sized.

Device-event timing after warm-up (the median window is reported, with the spread); the wall times end in a device synchronise.

    python tools/bench_weight_pack.py [--reps 200] [--rounds 7] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))
sys.path.insert(0, ROOT)

ROWS, INNER, WIDTHS = 192, 1728, (3, 8)


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels(reps, rounds):
    from hipops import ops
    g = torch.Generator().manual_seed(1005)
    w = torch.randn(ROWS, INNER, generator=g).cuda()
    alpha = torch.randn(ROWS, INNER, generator=g).cuda()
    dst = torch.empty_like(w)
    calls = {"copy_d2d": lambda: dst.copy_(w)}
    for b in WIDTHS:
        d, z = ops.uaq_init_minmax(w, 2 ** b)
        packed = ops.weight_pack(w, d, z, b)
        lv = torch.empty(ROWS, INNER, dtype=torch.int32, device="cuda")
        wq = torch.empty_like(w)
        calls[f"pack_nearest_w{b}"] = lambda d=d, z=z, b=b, out=packed.clone(): ops.weight_pack(w, d, z, b, out=out)
        calls[f"pack_adaround_w{b}"] = lambda d=d, z=z, b=b, out=packed.clone(): ops.weight_pack(w, d, z, b, alpha_rows=alpha, out=out)
        calls[f"unpack_wq_w{b}"] = lambda d=d, z=z, b=b, p=packed, wq=wq: ops.weight_unpack(p, d, z, INNER, b, levels=False, wq_out=wq)
        calls[f"unpack_both_w{b}"] = lambda d=d, z=z, b=b, p=packed, wq=wq, lv=lv: ops.weight_unpack(p, d, z, INNER, b, levels_out=lv, wq_out=wq)
    for fn in calls.values():                                      # warm-up: code objects, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in calls}
    for _ in range(rounds):                                        # alternate within one process
        for name, fn in calls.items():
            t[name].append(_time_us(fn, reps))
    row = dict(rows=ROWS, inner=INNER, input_bytes=4 * ROWS * INNER, reps=reps, rounds=rounds)
    for name, v in t.items():
        row[f"{name}_us"] = round(statistics.median(v), 2)
        row[f"{name}_spread_us"] = [round(min(v), 2), round(max(v), 2)]
    return row


def checkpoint():
    """save_packed and load_packed on the toy Cheng2020 of the suite (N = 8, round to nearest at 8 bits): wall time, the second of two runs"""
    import lic
    from quantization import QuantModel
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}

    def toy():
        torch.manual_seed(1005)
        qnn = QuantModel(lic.Cheng2020Anchor(N=8).cuda().eval(), wq, aq, is_cheng=True).cuda().eval()
        qnn.set_quant_state(True, False)
        with torch.no_grad():
            qnn(torch.rand(1, 3, 64, 64, device="cuda"))
        return qnn
    src = toy()
    row = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "toy.rdopack")
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = src.save_packed(path)
            torch.cuda.synchronize()
            row["save_packed_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        for _ in range(2):
            dst = toy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.load_packed(path)
            torch.cuda.synchronize()
            row["load_packed_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    row.update(model="Cheng2020Anchor N=8", modules=info["modules"], weights=info["weights"], file_bytes=info["file_bytes"])
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_pack needs a GPU: there is no CPU path to time")
    out = {"weight_pack": kernels(a.reps, a.rounds), "checkpoint": checkpoint()}
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
