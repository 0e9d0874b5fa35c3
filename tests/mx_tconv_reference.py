"""Reference of the MX transposed convolution (include/rdo_ptq_mxtconv.h), shared by tests/test_mx_tconv_args.py,
tests/test_gpu_mx_tconv.py and tests/test_gpu_mx_forward.py: numpy on the CPU, building on tests/mx_gemm_reference.py and
tests/mx_conv_reference.py.  The transposed convolution is stated as what it is defined to be: per phase (ry, rx) = ((oy + pad) % s,
(ox + pad) % s) of the output, the GEMM of the gathered activation matrix -- row (b, oy, ox) holds, tap after tap in ascending (kh, kw)
order over kh in {ry, ry + s, ...} < k and kw in {rx, rx + s, ...} < k, the C channels of input pixel (b, (oy + pad - kh) / s,
(ox + pad - kw) / s), or zeros (code 0 under the scale byte 127) where that pixel lies outside the image -- with the gathered weight
matrix, columns (kh k + kw) C .. (kh k + kw) C + C - 1 of the weight rows [N, k k C] in the same tap order."""
import numpy as np

import mx_conv_reference as CR
import mx_gemm_reference as G

BLOCK = G.BLOCK

# (B, H, W, C, N, k, stride, pad, output_padding): the all-pairs case (phases of 4, 2, 2 and 1 taps), the models' 5x5 stride-2 deconv
# with an N tail and K steps that straddle taps, stride 1 (one phase), k = s (one tap a phase), stride 3 with output padding 2 (the last
# rows and columns are bias only), 4x4 stride 2, and k < s (three of four phases have no tap)
PAIRS_GEOMETRY = (1, 3, 3, 32, 16, 3, 2, 1, 1)
GEOMETRIES = ((2, 4, 5, 64, 37, 5, 2, 2, 1), (2, 3, 4, 96, 24, 3, 1, 1, 0), (1, 4, 3, 32, 20, 2, 2, 0, 0), (1, 3, 3, 32, 16, 3, 3, 0, 2),
              (2, 2, 2, 64, 33, 4, 2, 1, 0), (1, 3, 3, 32, 16, 1, 2, 0, 1))
ALL_GEOMETRIES = (PAIRS_GEOMETRY,) + GEOMETRIES
# (x, w) format pairs of the exact test over GEOMETRIES
EXACT_PAIRS = (("mxfp4", "mxfp4"), ("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp4"), ("mxfp4", "mxfp8_e5m2"))


def out_size(n, k, stride, pad, opad):
    return (n - 1) * stride - 2 * pad + k + opad


def phases(B, H, W, k, stride, pad, opad):
    """The s * s phases in (ry, rx) order, each a dict: ry, rx, taps = [(kh, kw)] ascending, pixels = int64 [M_p] the output pixel
    (b Ho + oy) Wo + ox of every row in (b, oy, ox) order, index = int64 [M_p, len(taps)] the source pixel (b H + iy) W + ix of every
    (output pixel, tap of its phase), -1 outside the image.  Every output pixel lies in exactly one phase."""
    Ho, Wo = out_size(H, k, stride, pad, opad), out_size(W, k, stride, pad, opad)
    out = []
    for ry in range(stride):
        for rx in range(stride):
            taps = [(kh, kw) for kh in range(ry, k, stride) for kw in range(rx, k, stride)]
            oys = [o for o in range(Ho) if (o + pad) % stride == ry]
            oxs = [o for o in range(Wo) if (o + pad) % stride == rx]
            b, oy, ox = (a.reshape(-1) for a in np.meshgrid(np.arange(B), np.array(oys, dtype=np.int64), np.array(oxs, dtype=np.int64),
                                                            indexing="ij"))
            idx = np.full((b.size, len(taps)), -1, dtype=np.int64)
            for t, (kh, kw) in enumerate(taps):
                iy, ix = (oy + pad - kh) // stride, (ox + pad - kw) // stride
                assert ((oy + pad - kh) % stride == 0).all() and ((ox + pad - kw) % stride == 0).all()
                inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                idx[:, t] = np.where(inside, (b * H + iy) * W + ix, -1)
            out.append({"ry": ry, "rx": rx, "taps": taps, "pixels": ((b * Ho + oy) * Wo + ox).astype(np.int64), "index": idx})
    return out


def gathered_activation(codes, scales, phase):
    """codes uint8 [B H W, C] and scales uint8 [B H W, C / 32] -> the phase's gathered operand: codes [M_p, T C] and scales [M_p, T C / 32],
    code 0 and scale 127 at -1"""
    return CR.im2col_operand(codes, scales, phase["index"])


def gathered_weight(w, phase, k, per):
    """columns of w [N, k k per] of the phase's taps, in tap order: [N, T per] (per = C for values and codes, C / 32 for scales)"""
    w = np.asarray(w)
    cols = [np.arange((kh * k + kw) * per, (kh * k + kw + 1) * per) for kh, kw in phase["taps"]]
    return w[:, np.concatenate(cols)] if cols else w[:, :0]


def tconv64(x_codes, x_scales, fx, w_codes, w_scales, fw, geometry, bias=None):
    """float64 [B Ho Wo, N]: per phase `product64` of the decoded gathered operands, each row at its output pixel"""
    B, H, W, C, N, k, stride, pad, opad = geometry
    Ho, Wo = out_size(H, k, stride, pad, opad), out_size(W, k, stride, pad, opad)
    y = np.full((B * Ho * Wo, N), np.nan)
    for ph in phases(B, H, W, k, stride, pad, opad):
        ac, asc = gathered_activation(x_codes, x_scales, ph)
        wc, ws = gathered_weight(w_codes, ph, k, C), gathered_weight(w_scales, ph, k, C // BLOCK)
        y[ph["pixels"]] = G.product64(G.decode(ac, asc, fx), G.decode(wc, ws, fw), bias)
    assert not np.isnan(y).any()
    return y


def abs_tconv64(x64, w64, geometry, bias=None):
    """float64 [B Ho Wo, N]: sum |a b| (+ |bias|) of decoded values x64 [B H W, C] and w64 [N, k k C], and K_p, the elements of every
    output pixel's gathered row, int64 [B Ho Wo]"""
    B, H, W, C, N, k, stride, pad, opad = geometry
    Ho, Wo = out_size(H, k, stride, pad, opad), out_size(W, k, stride, pad, opad)
    s, K = np.zeros((B * Ho * Wo, N)), np.zeros(B * Ho * Wo, dtype=np.int64)
    for ph in phases(B, H, W, k, stride, pad, opad):
        s[ph["pixels"]] = G.abs_product64(CR.im2col(x64, ph["index"]), gathered_weight(w64, ph, k, C))
        K[ph["pixels"]] = len(ph["taps"]) * C
    if bias is not None:
        s = s + np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return s, K


def values64(x64, w64, geometry, bias=None):
    """float64 [B Ho Wo, N] of decoded values x64 [B H W, C] and w64 [N, k k C]"""
    B, H, W, C, N, k, stride, pad, opad = geometry
    Ho, Wo = out_size(H, k, stride, pad, opad), out_size(W, k, stride, pad, opad)
    y = np.zeros((B * Ho * Wo, N))
    for ph in phases(B, H, W, k, stride, pad, opad):
        y[ph["pixels"]] = G.product64(CR.im2col(x64, ph["index"]), gathered_weight(w64, ph, k, C), bias)
    return y


def exact_tconv_case(fx, fw, geometry, seed):
    """The inputs of the exact-product test: an activation [B H W, C] in `fx` and a weight [N, k k C] in `fw` drawn independently by
    `G.exact_operand` (non-zero data at every pixel), and a bias of multiples of 2^-4 below 8 in magnitude.  Every product is a multiple
    of 2^-4 of at most 36 x 4 = 144 = 2304 x 2^-4, so with 2304 K + 128 < 2^24, K = k k C (no gathered row is longer), every partial sum
    is a multiple of 2^-4 below 2^24 of that unit: exact in fp32 in any order.
    -> dict of numpy arrays: x_codes, x_scales, w_codes, w_scales, bias (float32), ref (float64 [B Ho Wo, N])"""
    B, H, W, C, N, k, stride, pad, opad = geometry
    K = k * k * C
    assert 2304 * K + 128 < 2 ** 24
    rng = np.random.default_rng(seed)
    xc, xs = G.exact_operand(B * H * W, C, fx, rng)
    wc, ws = G.exact_operand(N, K, fw, rng)
    bias = (rng.integers(-127, 128, N) / 16.0).astype(np.float32)
    return {"x_codes": xc, "x_scales": xs, "w_codes": wc, "w_scales": ws, "bias": bias,
            "ref": tconv64(xc, xs, fx, wc, ws, fw, geometry, bias)}
