"""The GDN / IGDN block of a unit as one launch (ops.gdn_fwd_bwd) against the four launches it replaces (linear_h2(square_input),
loss_gdn_bwd, linear_h2 on gamma'^T, gdn_bwd_dx_h2) at the workload's three map sizes: device events around alternating windows of
`--reps` calls, median over `--windows` windows per form.  usage: python tools/bench_gdn_fused.py [--inverse] [--no-dout]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rdo-ptq_amd"))
from hipops import ops  # noqa: E402

C = 192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--inverse", action="store_true")
    ap.add_argument("--no-dout", action="store_true", help="dL/dout is not written by the fused launch (an RBWS without a skip conv)")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(1)
    gam = 0.1 * torch.eye(C, device="cuda") + 0.002 * torch.rand(C, C, device="cuda", generator=g)
    scale = ops.pow2_scale(gam.abs().max())
    fwd, bwd = ops.split_h2_linear(gam.contiguous(), scale=scale), ops.split_h2_linear(gam.t().contiguous(), scale=scale)
    beta = 0.5 + torch.rand(C, device="cuda", generator=g)
    print(f"{'shape':>12s} {'chain us':>9s} {'fused us':>9s} {'ratio':>6s} {'fused GB/s':>10s}")
    for B, H in ((4, 128), (4, 64), (4, 32)):
        c = torch.randn(B, H, H, C, device="cuda", generator=g)
        res = torch.randn(B, H, H, C, device="cuda", generator=g)
        tgt = torch.randn(6, H, H, C, device="cuda", generator=g)
        idx = torch.tensor([[1, 4, 2, 0]], dtype=torch.int32, device="cuda")
        it = torch.zeros(1, dtype=torch.int32, device="cuda")
        log = torch.zeros(1, 32, device="cuda")
        norm, acc, dout, t, dx = (torch.empty_like(c) for _ in range(5))
        pl = ops.h2_empty(c.shape, "cuda", 2.0 ** 10)

        def chain():
            ops.linear_h2(c.view(-1, C), fwd, beta, out=norm.view(-1, C), square_input=True)
            ops.loss_gdn_bwd(c, norm, res, tgt, idx, it, 2.0, a.inverse, log, dout, t=t)
            ops.linear_h2(t.view(-1, C), bwd, None, out=acc.view(-1, C))
            ops.gdn_bwd_dx_h2(dout, c, norm, acc, a.inverse, dx_planes=pl)

        def fused():
            ops.gdn_fwd_bwd(c, fwd, bwd, beta, res, tgt, idx, it, 2.0, a.inverse, log, t, grad_out=None if a.no_dout else dout, dx_planes=pl)

        times = {"chain": [], "fused": []}
        for f in (chain, fused):
            f()
        torch.cuda.synchronize()
        for _ in range(a.windows):
            for name, f in (("chain", chain), ("fused", fused)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        ch, fu = statistics.median(times["chain"]), statistics.median(times["fused"])
        n = c.numel()
        byts = n * (12 + 4 + (0 if a.no_dout else 4) + 4) + 8 * C * C      # c, target, residual in; t (, dout), dx planes out
        print(f"{B}x{H}^2".rjust(12), f"{ch:9.1f} {fu:9.1f} {fu / ch:6.2f} {byts / fu / 1e3:10.0f}")
        ops.h2_overflow(reset=True)


if __name__ == "__main__":
    main()
