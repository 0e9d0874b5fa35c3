"""Inputs and case lists shared by tests/test_attention_reference.py (CPU) and tests/test_gpu_attention.py (GPU).  No tests here.

`trained_like(g, seed)` draws operands at the scales trained Lu2022 models have, which `randn * 1.5` at head dims <= 4 never reaches:
  - per-head temperatures: q and k of head h are scaled so that the standard deviation of a row's logits is about 0.5, 4 or 12
    (heads in turn; scale * q.k over hd terms of variance a^4 has the deviation a^2), the largest |logit| several deviations out;
  - bias 2 randn with planted +8 / -8 entries; the LAST head of a multi-head case has an all-zero bias;
  - v and dout with per-channel scales 10^[-1, 1], two decades;
  - planted in window 0 (when the window has the tokens for it): a row with two exactly equal maxima (two identical k rows, equal bias),
    a row that is one-hot to float32 precision (one logit about 40 above the rest, in the coolest head), and one window of all
    zeros (the last one: in shifted cases the corner window that holds every region) -- its probabilities are softmax(bias + mask), and
    uniform over each region in the zero-bias head."""
import torch

from oracle import attention_oracle as A

# name -> (B, H, W, C, heads, window, shift); the name says which path of csrc/swin.hip the case takes
PATH_CASES = {
    "vec_it1_full_hd16": (2, 16, 16, 64, 4, 8, 4),
    "vec_it2_model_head_hd32": (1, 16, 16, 64, 2, 8, 4),
    "vec_it3_hd48": (1, 16, 8, 96, 2, 8, 0),
    "vec_it4_hs65_hd64": (1, 8, 16, 128, 2, 8, 4),
    "vec_it4_hd52": (1, 8, 16, 104, 2, 8, 4),
    "vec_n16_hyper_hd12": (2, 8, 8, 48, 4, 4, 2),
    "vec_n16_ndb_hd32": (2, 8, 8, 64, 2, 4, 2),
    "vec_n16_ndb_hd20": (1, 8, 8, 40, 2, 4, 0),
    "vec_n36_ndb_hd48": (1, 12, 12, 96, 2, 6, 3),
    "vec_n4_ndb_hd64": (1, 4, 4, 64, 1, 2, 1),
    "scalar_n64_hd3": (1, 16, 16, 12, 4, 8, 4),
    "scalar_n64_hd5": (1, 8, 16, 10, 2, 8, 0),
    "scalar_n64_hd33": (1, 8, 8, 66, 2, 8, 4),
    "scalar_n64_hd6": (1, 16, 8, 12, 2, 8, 4),
    "scalar_n16_hd3": (2, 8, 8, 12, 4, 4, 2),
    "scalar_n16_hd5": (1, 8, 4, 10, 2, 4, 0),
    "scalar_n16_hd33": (1, 4, 8, 66, 2, 4, 2),
    "scalar_n16_hd6": (2, 4, 4, 12, 2, 4, 1),
    "scalar_n1_hd5": (2, 3, 2, 10, 2, 1, 0),
    "vec_n1_hd16": (2, 2, 3, 32, 2, 1, 0),
    "one_window_per_axis_shift4": (1, 8, 8, 32, 2, 8, 4),
    "single_token_region_shift1": (1, 16, 24, 32, 2, 8, 1),
    "single_token_region_shift7": (1, 16, 24, 32, 2, 8, 7),
    "windows_not_multiple_of_8_b3_hd16": (3, 16, 16, 64, 4, 8, 4),
    "windows_not_multiple_of_8_b3_hd12_n16": (3, 8, 8, 48, 4, 4, 2),
}

# the cases the parent's kernels leave channels of out / dqkv unwritten in (vector path, N < 64, more 16-channel blocks than quads per thread)
NDB_CASES = ("vec_n16_ndb_hd32", "vec_n16_ndb_hd20", "vec_n36_ndb_hd48", "vec_n4_ndb_hd64")

TEMPERATURES = (0.5, 4.0, 12.0)


def trained_like(g, seed):
    """-> qkv [B, H, W, 3C], bias [heads, N, N], dout [B, H, W, C], float32 on the CPU"""
    gen = torch.Generator().manual_seed(seed)
    N, hd, heads = g.N, g.hd, g.heads
    q = torch.randn(g.windows, heads, N, hd, generator=gen)
    k = torch.randn(g.windows, heads, N, hd, generator=gen)
    amp = torch.tensor([TEMPERATURES[h % 3] ** 0.5 for h in range(heads)]).view(1, heads, 1, 1)
    amp = amp * (hd ** 0.5 * g.scale) ** -0.5                                  # (a scale other than hd^-1/2 keeps the logits' deviation)
    q, k = q * amp, k * amp
    chan = 10.0 ** (2 * torch.rand(heads, hd, generator=gen) - 1).view(1, heads, 1, hd)
    v = torch.randn(g.windows, heads, N, hd, generator=gen) * chan
    dO = torch.randn(g.windows, heads, N, hd, generator=gen) * 10.0 ** (2 * torch.rand(heads, hd, generator=gen) - 1).view(1, heads, 1, hd)
    bias = 2 * torch.randn(heads, N, N, generator=gen)
    flat = bias.view(-1)
    idx = torch.randperm(flat.numel(), generator=gen)[:max(2, flat.numel() // 50)]
    flat[idx[0::2]] = 8.0
    flat[idx[1::2]] = -8.0
    if heads >= 2:
        bias[heads - 1] = 0.0
    reg = A.token_regions(g)[0]
    same = (reg == reg[0]).nonzero().view(-1)                                  # tokens of window 0 in token 0's region
    if same.numel() >= 4:
        i1, j1, j2, j3 = (int(t) for t in same[:4].roll(-1))                   # rows 0 and i1, columns j1 | j2, j3: all in one region
        # one-hot row: row 0 of (window 0, head 0, the coolest); k_j1 along q_0 with scale * q_0 . k_j1 = 40
        q0 = q[0, 0, 0]
        k[0, 0, j1] = q0 * (40.0 / (g.scale * float(q0 @ q0)))
        # two equal maxima: row i1 of (window 0, head h_eq); k_j2 = k_j3 along q_i1 with the logit 30, and the same bias
        h_eq = 1 if heads >= 2 else 0
        q1 = q[0, h_eq, i1]
        k[0, h_eq, j2] = q1 * (30.0 / (g.scale * float(q1 @ q1)))
        k[0, h_eq, j3] = k[0, h_eq, j2]
        bias[h_eq, i1, j3] = bias[h_eq, i1, j2]
    if g.windows >= 2:
        q[-1], k[-1], v[-1] = 0.0, 0.0, 0.0
    qkv = A.scatter(g, [q, k, v], torch.float32)
    dout = A.scatter(g, [dO], torch.float32)
    assert bool(torch.isfinite(qkv).all()) and bool(torch.isfinite(dout).all())
    return qkv.contiguous(), bias.contiguous(), dout.contiguous()


def planted_rows(g, ref):
    """what the plants of `trained_like` did to the reference probabilities -> dict of measured facts (for the CPU test to assert)"""
    p = ref["p"]                                                                # [windows, heads, N, N]
    top2 = p.topk(min(2, g.N), dim=-1).values
    return {"one_hot_rows": int((top2[..., 0] >= 1 - 2.0 ** -25).sum()),
            "tied_rows": int((top2[..., 0] == top2[..., -1]).sum()) if g.N >= 2 else 0,
            "max_abs_logit": float(ref["s"][ref["s"] > -60].abs().max()),
            "min_prob": float(p.min())}


def ln_inputs(rows, C, seed):
    """LayerNorm operands -> x [rows, C], w [C] in [0.3, 3] (the gains helpers.trained_like_nic_ draws), b, dy.  Row 0 (and every 5th):
    mean 100, spread 0.1; row 1: constant; row 2: variance 1e-7, below eps; the rest 2 randn + 0.3"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=gen) * 2 + 0.3
    x[0::5] = 100.0 + 0.1 * torch.randn(x[0::5].shape, generator=gen)
    if rows > 1:
        x[1] = 3.7
    if rows > 2:
        x[2] = 0.5 + 1e-7 ** 0.5 * torch.randn(C, generator=gen)
    w = 0.3 + 2.7 * torch.rand(C, generator=gen)
    return x, w, torch.randn(C, generator=gen), torch.randn(rows, C, generator=gen)


def gelu_inputs(n):
    """a grid over [-12, 12] with +-0, +-1e-30, +-5, +-8.5 planted in front"""
    v = torch.linspace(-12.0, 12.0, n)
    plant = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 5.0, -5.0, 8.5, -8.5])
    v[:plant.numel()] = plant
    return v
