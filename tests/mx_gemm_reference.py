"""Reference of the packed MX operand and the MX GEMM (include/rdo_ptq_mxgemm.h), shared by tests/test_mx_gemm_args.py and
tests/test_gpu_mx_gemm.py: numpy / torch on the CPU, building on tests/mx_reference.py.  Bit-packing of one-code-per-byte codes into
blocks of 4 b bytes (element j of a block at bits [j b, (j + 1) b) of the block's little-endian bit string), decode of codes and scales
to float64 (every value exact), the float64 product and a k-ordered fp32 accumulation of the decoded operands; and the inputs of the
exact-product test, whose sums are exact in fp32 in any order."""
import numpy as np
import torch

import mx_reference as R

NAMES = R.NAMES
BLOCK = R.BLOCK


def pack(codes, fmt):
    """codes uint8 [rows, K] (numpy or torch), K % 32 == 0 -> uint8 numpy [rows, K / 32 * 4 b]"""
    c = np.asarray(codes, dtype=np.uint8)
    b = R.element_bits(fmt)
    rows, K = c.shape
    assert K % BLOCK == 0
    bits = np.unpackbits(c[:, :, None], axis=2, bitorder="little")[:, :, :b]          # [rows, K, b], the low bit first
    return np.packbits(bits.reshape(rows, K * b), axis=1, bitorder="little")           # K b bits a row = K / 32 blocks of 32 b bits


def unpack(packed, K, fmt):
    """the inverse of `pack` -> uint8 numpy [rows, K]"""
    p = np.asarray(packed, dtype=np.uint8)
    b = R.element_bits(fmt)
    rows = p.shape[0]
    assert p.shape[1] * 8 == K * b
    bits = np.unpackbits(p, axis=1, bitorder="little").reshape(rows, K, b)
    full = np.zeros((rows, K, 8), dtype=np.uint8)
    full[:, :, :b] = bits
    return np.packbits(full, axis=2, bitorder="little")[:, :, 0]


def decode_elements(codes, fmt):
    """the element values of codes (any integer array) as float64 numpy, without a scale.  The E4M3 NaN patterns and the E5M2
    exponent-31 patterns are decoded as if they were numbers: the callers leave them out"""
    _, eb, M, bias, _, _ = R.FORMATS[fmt]
    c = np.asarray(codes).astype(np.int64)
    neg = (c >> (eb + M)) & 1
    ex, m = (c >> M) & ((1 << eb) - 1), c & ((1 << M) - 1)
    mag = np.where(ex == 0, m * 2.0 ** (1 - bias - M), (1.0 + m / 2.0 ** M) * np.exp2((ex - bias).astype(np.float64)))
    return np.where(neg == 1, -mag, mag)


def decode(codes, scales, fmt):
    """codes uint8 [rows, K], scales uint8 [rows, K / 32] (none of them 255) -> float64 numpy [rows, K]"""
    sc = np.repeat(np.asarray(scales).astype(np.int64), BLOCK, axis=1)
    return decode_elements(codes, fmt) * np.exp2((sc - 127).astype(np.float64))


def finite_codes(fmt):
    """every element code of the format that is a number: all but the two E4M3 NaN patterns and the E5M2 exponent-31 patterns"""
    n = 1 << R.element_bits(fmt)
    c = np.arange(n)
    if fmt == "mxfp8_e4m3":
        return c[(c & 0x7F) != 0x7F]
    if fmt == "mxfp8_e5m2":
        return c[((c >> 2) & 31) != 31]
    return c


def code_of(value, fmt):
    """the element code of an exactly representable value (the smallest such code)"""
    c = finite_codes(fmt)
    v = decode_elements(c, fmt)
    hit = c[(v == value) & (np.signbit(v) == np.signbit(value))]
    assert hit.size, (value, fmt)
    return int(hit[0])


def product64(a, b, bias=None):
    """float64 [M, N] = a b^T (+ bias) of float64 [M, K] and [N, K]"""
    y = a @ b.T
    return y if bias is None else y + np.asarray(bias, dtype=np.float64)[None, :]


def abs_product64(a, b):
    """sum_k |a b| float64 [M, N]"""
    return np.abs(a) @ np.abs(b).T


def chain32(a, b, bias=None):
    """the k-ordered fp32 accumulation acc <- acc + fl(a_k b_k), k ascending from 0, then + bias: float32 [M, N]"""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert (a32 == a).all() and (b32 == b).all()
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = acc + a32[:, k, None] * b32[None, :, k]
    return acc if bias is None else acc + np.asarray(bias, dtype=np.float32)[None, :]


EXACT_MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)       # representable in all five formats; 0.5 is the FP4 / E2M3 subnormal


def exact_operand(rows, K, fmt, rng):
    """codes uint8 [rows, K] drawn from +-EXACT_MAGNITUDES and scales uint8 [rows, K / 32] = 127 + e, e in {-1, 0, 1} drawn per block"""
    table = np.array([[code_of(s * m, fmt) for m in EXACT_MAGNITUDES] for s in (1.0, -1.0)], dtype=np.uint8)
    codes = table[rng.integers(0, 2, (rows, K)), rng.integers(0, len(EXACT_MAGNITUDES), (rows, K))]
    scales = (127 + rng.integers(-1, 2, (rows, K // BLOCK))).astype(np.uint8)
    return codes, scales


def exact_case(fa, fb, M, N, K, seed):
    """The inputs of the exact-product test: A [M, K] in `fa` and B [N, K] in `fb`, drawn independently (`exact_operand`), and a bias of
    multiples of 2^-4 below 8 in magnitude.  Every product is a multiple of 2^-4 (elements multiples of 2^-1, scales >= 2^-1) of at
    most 36 x 4, so every partial sum over K <= 256 terms is a multiple of 2^-4 below 2^24 of that unit: exact in fp32 in any order.
    -> dict of numpy arrays: a_codes, a_scales, b_codes, b_scales, bias (float32), ref (float64 [M, N])"""
    assert K <= 256
    rng = np.random.default_rng(seed)
    ac, asc = exact_operand(M, K, fa, rng)
    bc, bsc = exact_operand(N, K, fb, rng)
    bias = (rng.integers(-127, 128, N) / 16.0).astype(np.float32)
    ref = product64(decode(ac, asc, fa), decode(bc, bsc, fb), bias)
    return {"a_codes": ac, "a_scales": asc, "b_codes": bc, "b_scales": bsc, "bias": bias, "ref": ref}


EXACT_PAIRS = (("mxfp4", "mxfp6_e3m2"), ("mxfp8_e4m3", "mxfp8_e4m3"), ("mxfp6_e2m3", "mxfp8_e5m2"))
EXACT_SHAPES = ((19, 37, 32), (19, 37, 96), (33, 16, 160), (16, 50, 256))


def to_torch(a):
    return torch.from_numpy(np.ascontiguousarray(a))
