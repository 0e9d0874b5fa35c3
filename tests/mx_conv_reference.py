"""Reference of the MX convolution (include/rdo_ptq_mxconv.h), shared by tests/test_mx_conv_args.py and tests/test_gpu_mx_conv.py: numpy
on the CPU, building on tests/mx_gemm_reference.py.  The convolution is stated as what it is defined to be: the GEMM on the im2col
matrix of the NHWC activation, whose row m = (b, oy, ox) holds, tap after tap in (kh, kw) order, the C channels of input pixel
(b, oy stride - pad + kh, ox stride - pad + kw), or zeros (code 0 under the scale byte 127) where that pixel lies in the padding."""
import numpy as np

import mx_gemm_reference as G

BLOCK = G.BLOCK

# (B, H, W, C, N, k, stride, pad): the first is the all-pairs case (nb = 9: every K step spans several taps, the last holds one block),
# then taps that straddle K steps unevenly with M and N tails, 5x5 stride 2, 3x3 stride 2 on odd sizes, no padding, and 1x1
PAIRS_GEOMETRY = (1, 4, 4, 32, 16, 3, 1, 1)
GEOMETRIES = ((2, 5, 7, 32, 24, 3, 1, 1), (2, 5, 7, 96, 37, 3, 1, 1), (2, 8, 6, 64, 16, 5, 2, 2), (1, 7, 9, 64, 20, 3, 2, 1),
              (2, 6, 6, 32, 16, 3, 1, 0), (3, 5, 5, 64, 33, 1, 1, 0))
MODULE_GEOMETRIES = ((2, 6, 7, 64, 24, 3, 1, 1), (2, 6, 7, 32, 16, 5, 2, 2))          # the two modules of the module-level test


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def im2col_index(B, H, W, k, stride, pad):
    """int64 [M, k * k], M = B Ho Wo: the source pixel (b H + iy) W + ix of every tap of every output pixel, -1 in the padding"""
    Ho, Wo = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    b, oy, ox, ky, kx = np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), np.arange(k), np.arange(k), indexing="ij")
    iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
    inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    return np.where(inside, (b * H + iy) * W + ix, -1).reshape(B * Ho * Wo, k * k).astype(np.int64)


def _gather(values, idx, fill):
    v = np.asarray(values)
    padded = np.concatenate([v, np.full((1, v.shape[1]), fill, dtype=v.dtype)])      # row -1 is the padding row
    return padded[idx].reshape(idx.shape[0], idx.shape[1] * v.shape[1])


def im2col(values, idx):
    """values [B * H * W, C] -> [M, k * k * C], zeros at -1"""
    return _gather(values, idx, 0)


def im2col_operand(codes, scales, idx):
    """codes uint8 [B * H * W, C] and scales uint8 [B * H * W, C / 32] -> codes [M, k * k * C] and scales [M, k * k * C / 32]: code 0 and
    scale 127 at -1"""
    return _gather(codes, idx, 0), _gather(scales, idx, 127)


def conv64(x_codes, x_scales, fx, w_codes, w_scales, fw, geometry, bias=None):
    """float64 [M, N]: `product64` of the decoded im2col operand and the decoded weight rows"""
    B, H, W, C, N, k, stride, pad = geometry
    ac, asc = im2col_operand(x_codes, x_scales, im2col_index(B, H, W, k, stride, pad))
    return G.product64(G.decode(ac, asc, fx), G.decode(w_codes, w_scales, fw), bias)


def exact_conv_case(fx, fw, geometry, seed):
    """The inputs of the exact-product test: an activation [B H W, C] in `fx` and a weight [N, k k C] in `fw` drawn independently by
    `G.exact_operand` (non-zero data at every pixel), and a bias of multiples of 2^-4 below 8 in magnitude.  Every product is a multiple
    of 2^-4 of at most 36 x 4 = 144 = 2304 x 2^-4, so with 2304 K + 128 < 2^24 every partial sum is a multiple of 2^-4 below 2^24 of
    that unit: exact in fp32 in any order (K <= 7281).
    -> dict of numpy arrays: x_codes, x_scales, w_codes, w_scales, bias (float32), ref (float64 [M, N])"""
    B, H, W, C, N, k, stride, pad = geometry
    K = k * k * C
    assert 2304 * K + 128 < 2 ** 24
    rng = np.random.default_rng(seed)
    xc, xs = G.exact_operand(B * H * W, C, fx, rng)
    wc, ws = G.exact_operand(N, K, fw, rng)
    bias = (rng.integers(-127, 128, N) / 16.0).astype(np.float32)
    return {"x_codes": xc, "x_scales": xs, "w_codes": wc, "w_scales": ws, "bias": bias,
            "ref": conv64(xc, xs, fx, wc, ws, fw, geometry, bias)}
