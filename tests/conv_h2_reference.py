"""CPU reference of the plane-input convolution forward rdo_conv2d_fwd_h2 (csrc/conv_fwd_h2.hip, conv_fwd_h2k.hip, conv_h2_common.h): plain
torch / numpy, NHWC as the kernels see their operands, no GPU and no import of the library.  tests/test_conv_h2_reference.py pins it;
tests/test_gpu_conv_h2_parity.py compares every launch of the dispatcher with it.  Not covered here: the `_px` store modes
(test_gpu_subpel.py), the `_tail` entry (test_gpu_tail_parity.py), the bf16x6 / fp32 kernels and conv2d_wgrad_h2.

The split (`split`): for a float32 value v and a power-of-two scale s
    p0 = RNE fp16(v s),   p1 = RNE fp16(v s - float32(p0))                                 (rdo::h2_split_pk / h2_split_store)
stored as [C/16][pixel][16] for activations (`act_planes`) and in the fragment order [Cin/16][KH][KW][Cout][16] for weights
(`weight_planes`, rdo::frag_index).  It returns the planes and the float64 operand they REPRESENT, (p0 + p1) / s: a float32 number (the
remainder v s - p0 has no bit below the last bit of v s, so p0 + p1 fits 24 bits).

The reference works on the represented operands x', w' -- what the kernel is handed -- so the rounding of the split is no part of the
conv's error budget:
    ref = conv(x', w') + bias   in float64,     S = conv(|x'|, |w'|) + |bias|,
    q   = the error of the reference's OWN sequential float32 chain (tape_reference.chain32: float32 products added one after the other,
          tap-major and channel-minor, then the bias, then the activation's slope, then the residual) in units of u S, u = 2^-24,
          subsampled by MAX_PRODUCTS as there.

The bound of an element is tape_reference.bound with d = D_OF["h2"] = 4:   (2 q + 4) u S + 2 u |ref|.   Derivation, none of it measured:
  * the kernel forms hi.hi + hi.lo + lo.hi of x' = xh + xl, w' = wh + wl (fp16 planes, times s_x s_w).  A product of two fp16 numbers
    has 22 significant bits: exact in the MFMA's fp32 accumulation.  What is summed is therefore a float32 chain over exact products,
    in an order of the kernel's own: 2 q u S, the factor 2 being the margin for another summation order (as for every kernel that
    tape_reference and wgrad_reference hold);
  * the dropped lo.lo: |xl| <= 2^-11 |xh| and |wl| <= 2^-11 |wh| (half an ulp of an 11-bit significand), so |xl wl| <= 2^-22 |xh wh| =
    4 u |xh wh|, and |xh wh| <= (1 + 2^-11)^2 |x' w'| -- the excess is 2^-10 of the term, far inside the margin of the 2 q.  Summed: 4 u S;
  * acc_scale = 1 / (s_x s_w) is a power of two: exact.  The bias add is one rounding, <= u |ref| (1 + ...): inside 2 u |ref|;
  * a K split adds the partial tiles (each a float32 chain over its own stages) in float32: another summation order, inside 2 q.
The slope and the residual are one rounding each and part of the chain that q is taken from.

Epilogues, as `finish16` (conv_h2_common.h) and the direct epilogue of the K32 kernel apply them: `pre` = conv + bias is copied out, then
the activation, then `+ residual`.
  LRELU      v > 0 ? v : 0.01f v          RELU       v > 0 ? v : 0
  LRELU_BWD  aux > 0 ? v : 0.01f v        RELU_BWD   aux > 0 ? v : 0        (with aux_planes: the sign of plane 0, which is the value's)
LRELU / RELU jump (in the derivative, RELU_BWD-like forms in the value) at 0: `mask` marks the elements whose float64 pre-activation is
within its own bound of 0.  Outside the mask the kernel must take the reference's branch; inside it either branch's value is accepted
(`alt`).  The masked share of a case must be <= MASK_CAP: a condition on the inputs that test_conv_h2_reference.py asserts on the CPU for
every case, so that no GPU run can hide elements behind the mask.  The `_BWD` forms branch on aux, drawn with |aux| >= 2^-6: no mask.

Two input families, drawn on the CPU with a seed fixed by the case's name up to its '@variant' suffix (the variants of a geometry -- the
same conv under other tuning keys -- share their operands and their reference):
  * 'exact': integers in [-3, 3], about a quarter of them zero, for x, w, bias, residual and aux; plane 1 is all zero, every product and
    partial sum is a float32 integer in any order (max S < 2^24 over the table): a correct launch returns float32(ref) bit for bit, K
    splits included.  Behind LRELU the expected value is the epilogue's own float32 arithmetic on that exact pre-activation
    (`finish32`: float32(0.01f v), then the float32 add of the residual), which is what "as the kernel applies them" means bit for bit;
  * 'randn': x ~ 3 randn, w ~ randn / sqrt(K^2 Cin), bias ~ 0.1 randn, residual, aux ~ randn; where a tensor has two channels or more
    its first is scaled by 1e-3 and its last by 1e3 (as wgrad_reference does), so that the max-norm cannot stand in for the per-element
    bound.  Scales: `pow2_scale`, the largest magnitude into (2^6, 2^7].

`expected_launch` restates the dispatcher (h2_ksplit, h2k_ksplit, h2_halo_shape, h2k_supported and the h2_n48 substitution of
conv2d_fwd_h2_impl) and `workspace_floats` rdo_conv2d_fwd_h2_workspace, as pure Python."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tape_reference import MASK_CAP, MAX_PRODUCTS, U, _seed, bound, chain32, rows_of  # noqa: F401  (the project's own, not restated)

F32 = np.float32
D_OF = {"h2": 4}
SLOPE32 = F32(0.01)
EPI_NONE, EPI_LRELU, EPI_LRELU_BWD, EPI_RELU, EPI_RELU_BWD = 0, 1, 2, 5, 6            # include/rdo_ptq_hip.h
AUX_MIN = 2.0 ** -6
H2_TARGET = 128.0
F16_MAX = 65504.0


# ---- the split ------------------------------------------------------------------------------------------------------------------------------
def pow2_scale(amax, target=H2_TARGET):
    """the power of two s with target / 2 < amax s <= target (1 for an all-zero tensor): ops.pow2_scale restated"""
    amax = float(amax)
    if amax <= 0.0:
        return 1.0
    return 2.0 ** min(60, max(-60, math.floor(math.log2(target / amax))))


def split(v, s):
    """float32 tensor, power-of-two scale -> (p0, p1 fp16 tensors of v's shape, float64 (p0 + p1) / s)"""
    xs = v.float() * float(s)                                                         # float32 product (exact: s is a power of two)
    p0 = xs.to(torch.float16)
    p1 = (xs - p0.float()).to(torch.float16)
    return p0, p1, (p0.double() + p1.double()) / float(s)


def act_planes(p0, p1):
    """planes of an activation [..., C] -> int16 [2, C/16, pixels, 16] (slice-major)"""
    C = p0.shape[-1]
    lay = lambda p: p.contiguous().view(torch.int16).reshape(-1, C // 16, 16).permute(1, 0, 2)
    return torch.stack([lay(p0), lay(p1)]).contiguous()


def weight_planes(p0, p1):
    """planes of a weight [Cout,KH,KW,Cin] -> int16 [2, Cout,KH,KW,Cin] holding the fragment order [Cin/16][KH][KW][Cout][16]"""
    Cout, KH, KW, Cin = p0.shape
    lay = lambda p: p.contiguous().view(torch.int16).view(Cout, KH, KW, Cin // 16, 16).permute(3, 1, 2, 0, 4).reshape(Cout, KH, KW, Cin)
    return torch.stack([lay(p0), lay(p1)]).contiguous()


def planes_to_float64(planes, shape, s):
    """int16 [2, C/16, pixels, 16] -> float64 [..., C] = (p0 + p1) / s"""
    v = planes.view(torch.float16).double().sum(0) / float(s)
    return v.permute(1, 0, 2).reshape(shape)


# ---- the dispatcher, restated ---------------------------------------------------------------------------------------------------------------
TUNING_DEFAULTS = {"h2_k32": 3, "x6p_halo": 1, "h2_n48": 1}
TAGS = ("conv_fwd_h2_256x192", "conv_fwd_h2_halo", "conv_fwd_h2_halo64", "conv_fwd_h2_halo64k")


def out_hw(H, W, K, stride, pad):
    return (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1


def _cdiv(a, b):
    return -(-a // b)


def h2_ksplit(g):
    """K split of the per-tap kernel (0: the shape is not on the plane path)"""
    B, H, W, Cin, Cout, K, s, p = g
    Ho, Wo = out_hw(H, W, K, s, p)
    tiles = _cdiv(B * Ho * Wo, 256) * _cdiv(Cout, 192)
    stages = K * K * (Cin // 16)
    best = 0
    for ks in range(1, 13):
        if tiles * ks >= 192 and stages // ks >= 9:
            best = ks
            if tiles * ks >= 256:
                break
    return best


def _same3(g):
    B, H, W, Cin, Cout, K, s, p = g
    return K == 3 and s == 1 and p == 1 and H % 16 == 0 and W % 16 == 0


def h2k_ksplit(g, t):
    """-> (split, shape) of the K32 kernel's K-split form; (0, 2): not applicable"""
    B, H, W, Cin, Cout, K, s, p = g
    mode = t["h2_k32"]
    if not (t["x6p_halo"] and mode >= 2 and _same3(g) and Cin % 32 == 0 and Cout % 64 == 0):
        return 0, 2
    patches, cpairs = B * H * W // 256, Cin // 32
    if mode >= 3 and Cout % 48 == 0:
        tiles = patches * (Cout // 48)
        if 24 <= tiles < 200:
            best = 0
            for ks in range(2, cpairs + 1):
                if cpairs % ks == 0 and tiles * ks <= 256:
                    best = ks
            if best:
                return best, 3
    tiles = patches * (Cout // 64)
    if tiles >= 160 or tiles < 24:
        return 0, 2
    for ks in range(2, cpairs + 1):
        if cpairs % ks == 0 and tiles * ks >= 192:
            return ks, 2
    return 0, 2


def h2_halo_shape(g, t):
    B, H, W, Cin, Cout, K, s, p = g
    if not (t["x6p_halo"] and _same3(g)):
        return 0
    if h2_ksplit(g) == 1:
        return 1
    patches = B * H * W // 256
    if t["x6p_halo"] != 2 and Cout % 64 == 0 and patches * (Cout // 64) >= 160:
        return 2
    if t["x6p_halo"] != 2 and t["h2_k32"] and Cout % 48 == 0 and Cout % 64 != 0 and Cin % 32 == 0 and patches * (Cout // 48) >= 96:
        return 3
    return 0


def h2k_supported(g, shape, ksplit):
    B, H, W, Cin, Cout, K, s, p = g
    return (Cout % {1: 192, 2: 64, 3: 48}[shape] == 0 and _same3(g) and Cin % 32 == 0 and 1 <= ksplit <= Cin // 32 and (shape >= 2 or ksplit == 1)
            and Cin * 9 * Cout * 16 < 1 << 30 and B * H * W * Cin < 1 << 30)


def supported(g):
    """rdo_conv2d_fwd_h2_supported (with the split-precision kernels enabled, the default)"""
    B, H, W, Cin, Cout, K, s, p = g
    return Cin % 16 == 0 and Cout % 16 == 0 and B * H * W * Cin * 2 < 1 << 31 and Cout * K * K * Cin * 2 < 1 << 31 and h2_ksplit(g) >= 1


def workspace_floats(g, t):
    """rdo_conv2d_fwd_h2_workspace: room for the larger of the two K splits, whichever launch runs"""
    B, H, W, Cin, Cout, K, s, p = g
    Ho, Wo = out_hw(H, W, K, s, p)
    ks = max(h2_ksplit(g), h2k_ksplit(g, t)[0])
    return ks * B * Ho * Wo * Cout if ks > 1 else 0


def expected_launch(case):
    """case: a name of CASES or its tuple -> dict(tag, kernel, tile, ksplit).  kernel: 'h2' = conv_fwd_h2_kernel (per tap), 'h2h' =
    conv_fwd_h2h_kernel (halo, 16-channel stages), 'h2k' = conv_fwd_h2k_kernel (halo, 32-channel stages); tile = (pixels, channels);
    ksplit > 1: partial tiles + h2_splitk_epilogue."""
    c = CASES[case] if isinstance(case, str) else case
    g = tuple(c[:8])
    t = dict(TUNING_DEFAULTS, **c[9])
    assert supported(g), g
    ks = h2_ksplit(g)
    halo = h2_halo_shape(g, t)
    if not halo:
        ks2, kshape = h2k_ksplit(g, t)
        if ks2 >= 2 and h2k_supported(g, kshape, ks2):
            return {"tag": "conv_fwd_h2_halo64k", "kernel": "h2k", "tile": (256, 48 if kshape == 3 else 64), "ksplit": ks2}
    if halo and t["h2_k32"] and (halo >= 2 or ks == 1):
        B, H, W, Cin, Cout = g[:5]
        shape, patches = halo, B * H * W // 256
        if (halo == 2 and t["h2_n48"] and Cout % 48 == 0 and patches * (Cout // 64) < 256 and patches * (Cout // 48) <= 256
                and h2k_supported(g, 3, 1)):
            shape = 3
        if h2k_supported(g, shape, 1):
            return {"tag": "conv_fwd_h2_halo" if shape == 1 else "conv_fwd_h2_halo64", "kernel": "h2k", "tile": (256, {1: 192, 2: 64, 3: 48}[shape]),
                    "ksplit": 1}
    if halo == 1 and ks == 1:
        return {"tag": "conv_fwd_h2_halo", "kernel": "h2h", "tile": (256, 192), "ksplit": 1}
    if halo == 2:
        return {"tag": "conv_fwd_h2_halo64", "kernel": "h2h", "tile": (256, 64), "ksplit": 1}
    return {"tag": "conv_fwd_h2_256x192", "kernel": "h2", "tile": (256, 192), "ksplit": ks}


def launch_name(e):
    """the `launch` column of CASES for an expected_launch() result"""
    if e["kernel"] == "h2":
        return "pertap" if e["ksplit"] == 1 else "pertap_split"
    if e["kernel"] == "h2h":
        return f"k16_{e['tile'][1]}"
    return f"k32_{e['tile'][1]}" + ("_split" if e["ksplit"] > 1 else "")


# ---- the case table -------------------------------------------------------------------------------------------------------------------------
# geometry: (B, H, W, Cin, Cout, K, stride, pad)
GEOMS = {
    "1x1_m49062": (1, 221, 222, 144, 16, 1, 1, 0),          # M = 49 062: 192 M tiles, the last of 166 rows; 9 stages; N tile 16 of 192
    "3x3_s2_odd": (1, 443, 443, 16, 16, 3, 2, 1),           # stride 2, odd size, border taps; M = 222^2 = 49 284 (193 tiles, last 132 rows)
    "1x1_cout208": (1, 157, 157, 144, 208, 1, 1, 0),        # two N tiles, the second 16 of 192; M = 24 649: 97 M tiles, the last of 73 rows
    "5x5_m4095": (1, 63, 65, 80, 16, 5, 1, 2),              # M = 4095 (16 tiles, last 255 rows); 125 stages over 12 splits: 10 or 11 each
    "3x3_m4095": (1, 63, 65, 192, 16, 3, 1, 1),             # 3 x 3 'same' off the halo kernels by H, W % 16 != 0; 108 stages over 12
    "halo_cin16": (3, 128, 128, 16, 16, 3, 1, 1),           # Cin % 32 != 0: h2h<4,2,2,3>; every patch border; zero halo
    "halo64_cin48": (5, 64, 128, 48, 64, 3, 1, 1),          # halo == 2 with Cin % 32 != 0: h2h<8,1,1,2>; non-square image
    "k32_192": (4, 128, 128, 32, 192, 3, 1, 1),             # K32 shape 1: 256 tiles (with 192 to 255 the 18 stages would split in two)
    "k32_64": (5, 64, 128, 32, 64, 3, 1, 1),                # K32 shape 2
    "k32_n48": (4, 64, 64, 64, 192, 3, 1, 1),               # K32 shape 3 by h2_n48 (192 tiles of 64 -> 256 of 48)
    "k32_halo3": (6, 64, 64, 32, 48, 3, 1, 1),              # K32 shape 3 by halo == 3 (Cout % 64 != 0)
    "k32_split64": (2, 64, 64, 96, 192, 3, 1, 1),           # K32 K split, shape 2: cpairs = 3, ks = 3
    "k32_split48": (1, 64, 64, 192, 192, 3, 1, 1),          # K32 K split, shape 3: ks = 3 of 6 slice pairs
}
K16 = {"h2_k32": 0}
PERTAP = {"x6p_halo": 0}
# name -> geometry + (launch, tuning overrides, flags); flags: "epi" = every epilogue form, "ovf" = the overflow-word check
_ROWS = (
    ("1x1_m49062", "pertap", {}, ()),
    ("3x3_s2_odd", "pertap", {}, ()),
    ("1x1_cout208", "pertap", {}, ()),
    ("5x5_m4095", "pertap_split", {}, ("epi", "ovf")),
    ("3x3_m4095", "pertap_split", {}, ()),
    ("halo_cin16", "k16_192", {}, ("epi",)),
    ("halo_cin16@pertap", "pertap", PERTAP, ()),
    ("halo64_cin48", "k16_64", {}, ()),
    ("halo64_cin48@pertap", "pertap_split", PERTAP, ()),
    ("k32_192", "k32_192", {}, ()),
    ("k32_192@k16", "k16_192", K16, ()),
    ("k32_192@pertap", "pertap", PERTAP, ()),
    ("k32_64", "k32_64", {}, ("epi",)),
    ("k32_64@k16", "k16_64", K16, ()),
    ("k32_64@pertap", "pertap_split", PERTAP, ()),
    ("k32_n48", "k32_48", {}, ()),
    ("k32_n48@n64", "k32_64", {"h2_n48": 0}, ()),
    ("k32_n48@k16", "k16_64", K16, ()),
    ("k32_n48@pertap", "pertap_split", PERTAP, ()),
    ("k32_halo3", "k32_48", {}, ()),
    ("k32_halo3@k16", "pertap_split", K16, ()),             # halo == 3 exists on the K32 kernel only
    ("k32_split64", "k32_64_split", {}, ()),                # 128 tiles of 48 admit no even split within 256 workgroups: 64 tiles of 64 x 3
    ("k32_split64@k16", "pertap_split", K16, ()),
    ("k32_split48", "k32_48_split", {}, ("epi",)),
    ("k32_split48@mode2", "k32_64_split", {"h2_k32": 2}, ()),   # mode 2: 256 x 64 tiles, the smallest split that reaches 192 workgroups
    ("k32_split48@pertap", "pertap_split", PERTAP, ()),
)
CASES = {name: GEOMS[name.split("@")[0]] + (launch, tuning, flags) for name, launch, tuning, flags in _ROWS}
# the rows of the issue's table: launch -> the cases that must reach it
TABLE = {
    "pertap": ("1x1_m49062", "3x3_s2_odd", "1x1_cout208"),
    "pertap_split": ("5x5_m4095", "3x3_m4095"),
    "k16_192": ("halo_cin16",),
    "k16_64": ("halo64_cin48",),
    "k32_192": ("k32_192",),
    "k32_64": ("k32_64", "k32_n48@n64"),
    "k32_48": ("k32_n48", "k32_halo3"),
    "k32_64_split": ("k32_split64",),
    "k32_48_split": ("k32_split48",),
}
FAMILIES = ("exact", "randn")
# (epilogue, aux, residual, pre) -- every case runs the first two, the "epi" cases all of them
EPILOGUES = {
    "none": (EPI_NONE, False, False, False),
    "lrelu_res_pre": (EPI_LRELU, False, True, True),
    "none_res": (EPI_NONE, False, True, False),
    "relu": (EPI_RELU, False, False, False),
    "lrelu_bwd": (EPI_LRELU_BWD, True, False, False),
    "relu_bwd_res": (EPI_RELU_BWD, True, True, False),
}
BASIC = ("none", "lrelu_res_pre")


def epilogues_of(name):
    return tuple(EPILOGUES) if "epi" in CASES[name][10] else BASIC


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _draw(shape, gen, family, scale):
    if family == "exact":
        v = torch.randint(-3, 4, shape, generator=gen).float()
        # 1/7 + 6/7 * 1/8 = a quarter zeros, all of them +0: rdo_split_h2_conv leaves the sign of a -0 weight in plane 1 (+0, -0) where the
        # formula above puts it in plane 0 (-0, +0) -- the same operand, other bits; test_split_h2_round_trip_and_overflow_flag holds the
        # activation form on -0
        return torch.where(torch.rand(shape, generator=gen) >= 0.125, v, torch.zeros_like(v))
    v = torch.randn(shape, generator=gen) * scale
    if shape[-1] >= 2:
        v[..., 0] *= 1e-3
        v[..., -1] *= 1e3
    return v


def inputs(name, family):
    """-> dict(x [B,H,W,Cin], w [Cout,K,K,Cin], bias, res, aux [B,Ho,Wo,Cout]): float32, NHWC"""
    base = name.split("@")[0]
    B, H, W, Cin, Cout, K, s, p = GEOMS[base]
    Ho, Wo = out_hw(H, W, K, s, p)
    gen = torch.Generator().manual_seed(_seed(base + ":" + family))
    x = _draw((B, H, W, Cin), gen, family, 3.0)
    w = _draw((Cout, K, K, Cin), gen, family, 1.0 / (K * K * Cin) ** 0.5)
    bias = _draw((Cout,), gen, family, 0.1)
    res = _draw((B, Ho, Wo, Cout), gen, family, 1.0)
    aux = _draw((B, Ho, Wo, Cout), gen, family, 1.0)
    if family == "exact":
        aux = torch.where(aux == 0, torch.ones_like(aux), aux)                          # the sign decides: no zero
    else:
        aux = torch.where(aux >= 0, aux.clamp_min(AUX_MIN), aux.clamp_max(-AUX_MIN))
    return {"x": x, "w": w, "bias": bias, "res": res, "aux": aux}


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def finish32(pre32, epi, aux, res):
    """the epilogue's own float32 arithmetic on a float32 pre-activation (numpy float32 arrays; aux / res None where absent)"""
    v = pre32.astype(F32)
    t = aux if epi in (EPI_LRELU_BWD, EPI_RELU_BWD) else v
    if epi in (EPI_LRELU, EPI_LRELU_BWD):
        v = np.where(t > 0, v, SLOPE32 * v).astype(F32)
    elif epi in (EPI_RELU, EPI_RELU_BWD):
        v = np.where(t > 0, v, F32(0)).astype(F32)
    if res is not None:
        v = (v + res).astype(F32)
    return v


class Out:
    """one epilogue form of a case: ref, S, q, bnd (float64 [B,Ho,Wo,Cout]); mask (bool), alt (the other branch's value) and alt_bnd (its
    bound) for the forms that branch on the pre-activation, else None"""
    __slots__ = ("ref", "S", "q", "bnd", "mask", "alt", "alt_bnd")


class ConvH2Ref:
    """x, w, bias, res, aux: float32 CPU tensors (NHWC / [Cout,K,K,Cin]); sx, sw: the power-of-two scales of the planes"""

    def __init__(self, x, w, bias, res, aux, stride, pad, sx=None, sw=None, max_products=MAX_PRODUCTS):
        self.sx = pow2_scale(x.abs().max()) if sx is None else sx
        self.sw = pow2_scale(w.abs().max()) if sw is None else sw
        self.bias, self.res, self.aux, self.stride, self.pad = bias, res, aux, stride, pad
        x0, x1, self.x64 = split(x, self.sx)
        w0, w1, self.w64 = split(w, self.sw)
        self.xplanes, self.wplanes = act_planes(x0, x1), weight_planes(w0, w1)
        self.plane1_zero = not bool(x1.float().any()) and not bool(w1.float().any())
        xn, wn = nchw(self.x64), nchw(self.w64)
        self.pre = nhwc(F.conv2d(xn, wn, bias.double(), stride, pad))
        self.S_pre = nhwc(F.conv2d(xn.abs(), wn.abs(), bias.double().abs(), stride, pad))
        self._xn32, self._wn32 = xn.float(), wn.float()                                # exact: the represented operands are float32 numbers
        self._max_products = max_products
        self.q_pre = self._q(None, None, self.pre, self.S_pre)
        self.d = D_OF["h2"]
        self.bound_pre = bound(self.S_pre, self.pre, self.q_pre, self.d)
        self._outs = {}

    def _q(self, slope32, res, ref, S):
        idx, c = chain32(self._xn32, self._wn32, self.bias, self.stride, self.pad, None if slope32 is None else nchw(slope32),
                         max_products=self._max_products)
        if res is not None:
            c = c + res.reshape(-1, res.shape[-1])[idx]
        r, s = ref.reshape(-1, ref.shape[-1])[idx], S.reshape(-1, S.shape[-1])[idx]
        err = (c.double() - r).abs()
        assert bool((err[s == 0] == 0).all())
        live = s > 0
        return float((err[live] / (U * s[live])).max()) if bool(live.any()) else 0.0

    def out(self, key):
        if key in self._outs:
            return self._outs[key]
        epi, use_aux, use_res, _ = EPILOGUES[key]
        o = Out()
        pre, S = self.pre, self.S_pre
        lo = float(SLOPE32) if epi in (EPI_LRELU, EPI_LRELU_BWD) else 0.0
        o.mask = o.alt = o.alt_bnd = None
        if epi == EPI_NONE:
            slope = None
            y, Sy = pre, S
        else:
            pos = (self.aux > 0) if use_aux else (pre > 0)
            slope = torch.where(pos, 1.0, lo).double()
            y, Sy = pre * slope, S * slope
            if not use_aux:
                o.mask = pre.abs() <= self.bound_pre
                o.alt = pre * torch.where(pos, lo, 1.0).double()
        if use_res:
            y, Sy = y + self.res.double(), Sy + self.res.double().abs()
            if o.alt is not None:
                o.alt = o.alt + self.res.double()
        o.ref, o.S = y, Sy
        o.q = self.q_pre if slope is None and not use_res else max(
            self.q_pre, self._q(None if slope is None else slope.float(), self.res if use_res else None, y, Sy))
        o.bnd = bound(Sy, y, o.q, self.d)
        o.alt_bnd = None if o.alt is None else bound(S * (1.0 + lo - slope) + (self.res.double().abs() if use_res else 0.0), o.alt, o.q, self.d)
        self._outs[key] = o
        return o

    def expected32(self, key):
        """'exact' family: the float32 tensors (out, pre) a correct launch returns bit for bit"""
        epi, use_aux, use_res, _ = EPILOGUES[key]
        pre32 = self.pre.float()
        assert torch.equal(pre32.double(), self.pre)
        out = finish32(pre32.numpy(), epi, self.aux.numpy() if use_aux else None, self.res.numpy() if use_res else None)
        return torch.from_numpy(out), pre32


@functools.lru_cache(maxsize=None)
def case(name, family):
    """-> dict(x, w, bias, res, aux, ref: ConvH2Ref) of one CASES entry (shared by its '@variant's), built once and left unchanged"""
    base = name.split("@")[0]
    if base != name:
        return case(base, family)
    g = GEOMS[base]
    c = inputs(base, family)
    c["ref"] = ConvH2Ref(c["x"], c["w"], c["bias"], c["res"], c["aux"], g[6], g[7])
    return c


def overflow_setup(name):
    """'exact' family, NONE + residual: -> (residual with ONE element changed, out_scale = 2^j, expected float32 out).  j is the largest
    with every other |out| 2^j <= 65504; the changed element (the largest output) becomes 2^(16 - j), so 65536 > 65504 is the only
    scaled magnitude beyond fp16's range."""
    c = case(name, "exact")
    o = c["ref"].out("none_res")
    flat = o.ref.reshape(-1)
    e = int(flat.abs().argmax())
    others = flat.abs().clone()
    others[e] = 0.0
    j = math.floor(math.log2(F16_MAX / float(others.max())))
    big = 2.0 ** (16 - j)
    res = c["res"].clone()
    res.view(-1)[e] += float(big - flat[e])
    want = c["ref"].pre + res.double()
    assert float(want.reshape(-1)[e]) == big and float(others.max()) * 2.0 ** j <= F16_MAX < big * 2.0 ** j
    assert float(res.abs().max()) < 2.0 ** 16 and torch.equal(want.float().double(), want)
    return res, 2.0 ** j, want.float()
