"""Reference of the per-channel rate sums (`rdo_neg_log2_channel_sums` of csrc/entropy.hip, `ops.neg_log2_channel_sums`), shared by
tests/test_rd_report_args.py (CPU) and tests/test_gpu_rd_report.py (GPU).  No tests here.

The tensor is [outer][C][inner], element (o, c, i) at ((o C) + c) inner + i; out[c] = sum over o, i of -log2(lik[o, c, i]).
  channel_bits      the float64 restatement and sum |t_i| of its terms, per channel
  channel_sums32    a float32 restatement: the same expression, summed in the kernel's own order
  channel_bound     the derived bound per channel

The kernel's summation structure (the comment in front of rate_channel_part_kernel).  A channel's n = outer * inner elements are numbered
j = o inner + i.  geometry(outer, C, inner) -> (PL, S): PL element lanes a workgroup (256 for inner > 1; 256 // min(C, 64) for inner = 1),
S = min(256, ceil(n / (8 PL))) workgroups down the channel.
  1. lane pl of workgroup s adds its elements j = s PL + pl, + S PL, + 2 S PL, .. serially onto 0: at most L = ceil(n / (S PL)) terms,
     so at most L roundings on the path of a term (the first addition, onto 0, is exact);
  2. the PL lanes fold as a binary tree, lane pl += lane pl + h for h = 128, 64, .., 1 while pl + h < PL: a step adds something only
     when PL > h, so a term passes ceil(log2 PL) roundings;
  3. the fold kernel: lane j of sixteen adds the partial sums j, j + 16, .. serially onto 0 (at most ceil(S / 16) roundings), then the xor
     tree 8, 4, 2, 1 (4 roundings).
Every term therefore passes at most D = L + ceil(log2 PL) + ceil(S / 16) + 4 fp32 additions, each of relative error <= u = 2^-24, and the
sum's error from the additions is at most ((1 + u)^D - 1) sum |t_i| <= 1.01 D u sum |t_i| for D u < 0.01 (D is below 1e5 for every shape
the entry accepts in practice; the function asserts it).  On top, the term itself: log2f is accurate to 1 ulp = 2 u |t_i| by the HIP
maths documentation; 2 ulp = 4 u |t_i| are allowed, the allowance `ordered_bound` of tests/test_entropy_reference.py makes for the same
expression (the negation is exact).  Together
    bound[c] = 1.01 (D + 4) u sum_i |t_i|
with nothing in it taken from a measurement of the kernel.  An input of exactly representable terms whose partial sums stay below 2^24
units (the exact cases of the GPU test) passes every addition without rounding, in any order."""
import math

import numpy as np
import torch

U = 2.0 ** -24
F64 = torch.float64
f32 = np.float32


def geometry(outer, C, inner):
    """-> (PL, S) of rc_geom in csrc/entropy.hip"""
    cpb = min(C, 64) if inner == 1 else 1
    PL = 256 // cpb
    n = outer * inner
    return PL, min(256, -(-n // (PL * 8)))


def depth(outer, C, inner):
    """D: the most fp32 additions a term passes (see the module docstring)"""
    PL, S = geometry(outer, C, inner)
    L = -(-(outer * inner) // (S * PL))
    return L + (PL - 1).bit_length() + -(-S // 16) + 4


def _terms64(lik, outer, C, inner):
    """float64 terms [C, n] in the order of j"""
    t = -torch.log2(torch.as_tensor(lik).detach().cpu().reshape(outer, C, inner).to(F64))
    return t.permute(1, 0, 2).reshape(C, outer * inner)


def channel_bits(lik, outer, C, inner):
    """-> (bits [C], sum |t_i| [C]) in float64 on the CPU; `lik`: any tensor whose flat storage order is [outer][C][inner]"""
    t = _terms64(lik, outer, C, inner)
    return t.sum(1), t.abs().sum(1)


def channel_bound(outer, C, inner, abs_total):
    D = depth(outer, C, inner)
    assert D * U < 0.01
    return 1.01 * (D + 4) * U * abs_total


def channel_sums32(lik, outer, C, inner):
    """float32 restatement: -log2 in float32 (torch's CPU log2), added in the kernel's order -> float32 numpy [C]"""
    x = torch.as_tensor(lik).detach().cpu().reshape(outer, C, inner)
    assert x.dtype == torch.float32
    t = (-torch.log2(x)).permute(1, 0, 2).reshape(C, outer * inner).numpy()
    assert t.dtype == f32
    PL, S = geometry(outer, C, inner)
    n = outer * inner
    L = -(-n // (S * PL))
    pad = np.zeros((C, L * S * PL), f32)                   # an absent term is a 0: adding it is exact
    pad[:, :n] = t
    laps = pad.reshape(C, L, S, PL)
    acc = np.zeros((C, S, PL), f32)
    for k in range(L):                                     # 1. the lane's serial chain
        acc = acc + laps[:, k]
    lanes = np.zeros((C, S, 256), f32)
    lanes[:, :, :PL] = acc
    for h in (128, 64, 32, 16, 8, 4, 2, 1):                # 2. the LDS tree
        lanes[:, :, :h] = lanes[:, :, :h] + lanes[:, :, h:2 * h]
    part = lanes[:, :, 0]
    K = -(-S // 16)
    p = np.zeros((C, K * 16), f32)
    p[:, :S] = part
    r = np.zeros((C, 16), f32)
    for row in np.moveaxis(p.reshape(C, K, 16), 1, 0):     # 3. the fold's lane chains, then its xor tree
        r = r + row
    idx = np.arange(16)
    for o in (8, 4, 2, 1):
        r = r + r[:, idx ^ o]
    assert r.dtype == f32
    return r[:, 0]


def make_lik(outer, C, inner, seed):
    """likelihoods [outer, C, inner] log-uniform in [1e-9, 1], with planted 1.0 and 1e-9 elements (the floor and the ceiling of what the
    entropy models return) -> float32 CPU tensor"""
    g = torch.Generator().manual_seed(seed)
    lik = torch.exp(torch.rand(outer, C, inner, generator=g) * math.log(1e-9)).clamp(1e-9, 1.0)
    flat = lik.reshape(-1)
    n = flat.numel()
    for k, v in ((0, 1.0), (n - 1, 1e-9), (n // 2, 1.0), (n // 3, 1e-9)):
        flat[k] = v
    return lik.contiguous()


def as_nchw_and_channels_last(lik):
    """[outer, C, inner] values -> the same values as a 4-D tensor [outer, C, inner, 1] stored NCHW, and stored channels-last"""
    x = lik.reshape(lik.shape[0], lik.shape[1], lik.shape[2], 1).contiguous()
    return x, x.contiguous(memory_format=torch.channels_last)


# (outer, C, inner) of the kernel tests.  The last one is ours: NCHW it is n = 3000 elements a channel on 256 lanes -> S = 2 partial sums a
# channel; channels-last it is (3000, 5, 1): 5 channels side by side, PL = 51 lanes, S = ceil(3000 / 408) = 8 partial sums a channel --
# more than one workgroup down every channel in each of the two index mappings, with a ragged last lap in both.
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 7, 16), (3, 5, 63), (2, 192, 256), (512, 7, 1), (1536, 320, 1), (3, 5, 1000)]
