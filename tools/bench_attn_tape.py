"""The two backward kernels of the activation-quantised window attention (ops.window_attention_pv_bwd, ops.window_attention_probs_bwd)
at the model's shape, next to the fused backward they stand beside (ops.window_attention_bwd, which recomputes the probabilities and
reads and writes no [windows, N, N, heads] tensor): device events around alternating windows of `--reps` calls, median over `--windows`
windows per kernel.  Byte floor of each new kernel: the two [windows, N, N, heads] tensors it reads or writes, 2 x N^2 x heads x 4 B per
window, at the 6.3 TB/s a copy achieves.  usage: python tools/bench_attn_tape.py [--shape B H W C heads window shift]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rdo-ptq_amd"))
from hipops import ops  # noqa: E402

ACHIEVABLE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--shape", type=int, nargs=7, default=(4, 128, 128, 192, 6, 8, 4), metavar=("B", "H", "W", "C", "heads", "window", "shift"))
    a = ap.parse_args()
    B, H, W, C, heads, ws, shift = a.shape
    d = ops.attn_desc(B, H, W, C, heads, ws, shift)
    N, nwin = ws * ws, B * (H // ws) * (W // ws)
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn(B, H, W, 3 * C, device="cuda", generator=g)
    dout = torch.randn(B, H, W, C, device="cuda", generator=g)
    bias = torch.randn(heads, N, N, device="cuda", generator=g)
    probs = torch.empty(nwin, N, N, heads, device="cuda")
    ops.window_attention(d, qkv, bias, probs=probs, compute_out=False)
    dprobs, dqkv = torch.empty_like(probs), torch.empty_like(qkv)
    forms = {"pv_bwd": lambda: ops.window_attention_pv_bwd(d, qkv, probs, dout, dprobs=dprobs, dqkv=dqkv),
             "probs_bwd": lambda: ops.window_attention_probs_bwd(d, qkv, probs, dprobs, dqkv=dqkv),
             "fused bwd": lambda: ops.window_attention_bwd(d, qkv, bias, dout, dqkv=dqkv)}
    times = {k: [] for k in forms}
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    for _ in range(a.windows):
        for name, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    floor_bytes = 2 * nwin * N * N * heads * 4
    floor_us = floor_bytes / ACHIEVABLE * 1e6
    print(f"shape {tuple(a.shape)}: {nwin} windows, byte floor {floor_bytes / 1e6:.1f} MB = {floor_us:.1f} us at {ACHIEVABLE / 1e12:.1f} TB/s")
    print(f"{'kernel':>10s} {'us':>8s} {'min us':>8s} {'floor / time':>12s}")
    for name, ts in times.items():
        med = statistics.median(ts)
        share = f"{floor_us / med:12.2f}" if name != "fused bwd" else f"{'-':>12s}"
        print(f"{name:>10s} {med:8.1f} {min(ts):8.1f} {share}")


if __name__ == "__main__":
    main()
