#!/usr/bin/env python3
"""Time the differentiable MS-SSIM (losses.ms_ssim on a tracked input, forward + backward: five rdo_ssim_level, four pairs of
rdo_avg_pool2, then rdo_ssim_level_bwd x 5 and rdo_avg_pool2_bwd x 4 with the scalar glue on torch's tape) next to the forward
alone, on a [B, 3, S, S] batch.

    python tools/bench_msssim.py [--batch 4] [--size 256] [--iters 200]

Prints one line per form: ms per call (HIP events around `iters` calls after 20 warm-up calls)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rdo-ptq_amd")):
    sys.path.insert(0, p)
import torch

from losses.losses import ms_ssim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim: needs a GPU")
    g = torch.Generator().manual_seed(0)
    x = torch.rand(a.batch, 3, a.size, a.size, generator=g)
    y = (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(0, 1)
    x, y = x.cuda(), y.cuda()
    xt = x.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            ms_ssim(x, y)

    def fwd_bwd():
        torch.autograd.grad(ms_ssim(xt, y), xt)

    for name, fn in (("forward", fwd), ("forward+backward", fwd_bwd)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"ms_ssim {a.batch}x3x{a.size}x{a.size} {name:17s}: {e0.elapsed_time(e1) / a.iters:.3f} ms/call", flush=True)


if __name__ == "__main__":
    main()
