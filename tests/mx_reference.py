"""Reference of the MX block formats (include/rdo_ptq_mx.h), shared by tests/test_mx_args.py and tests/test_gpu_mx.py: a float64
restatement in torch on the CPU.  Every step is exact: `torch.frexp` gives floor(log2(.)) of a float64 (which holds every fp32 value,
subnormals included, as a normal number), the division by the power-of-two scale and by the spacing of the element's binade only move
the exponent, `torch.round` rounds halves to even, and the product of the rounded magnitude and the scale is checked to survive the
trip through float32."""
import torch

BLOCK = 32
#         name          id  exponent bits, mantissa bits, bias, emax, max
FORMATS = {"mxfp4": (0, 2, 1, 1, 2, 6.0),
           "mxfp6_e2m3": (1, 2, 3, 1, 2, 7.5),
           "mxfp6_e3m2": (2, 3, 2, 3, 4, 28.0),
           "mxfp8_e4m3": (3, 4, 3, 7, 8, 448.0),
           "mxfp8_e5m2": (4, 5, 2, 15, 15, 57344.0)}
NAMES = tuple(FORMATS)


def element_bits(fmt):
    _, eb, mb, _, _, _ = FORMATS[fmt]
    return 1 + eb + mb


def blocks(inner):
    return -(-inner // BLOCK)


def size_bits(rows, inner, fmt):
    """element bits x elements + 8 x blocks"""
    return element_bits(fmt) * rows * inner + 8 * rows * blocks(inner)


def _floor_log2(a):
    """floor(log2(a)) of positive float64 values as int64 (frexp: a = m 2^e with m in [0.5, 1))"""
    return torch.frexp(a)[1].to(torch.int64) - 1


def _pow2(e):
    return torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e)


def quantize(w, fmt):
    """w fp32 [rows, inner] on the CPU -> dict: wq fp32 [rows, inner], scales uint8 [rows, blocks], codes uint8 [rows, inner], err and
    energy float64 [rows] (d = w - wq formed in fp32, squared and added in float64).  A block with a NaN or an infinity: scale 255, wq
    NaN, codes 0 (unspecified in the kernel)."""
    _, eb, M, bias, emax, vmax = FORMATS[fmt]
    emin = 1 - bias
    assert w.dtype == torch.float32 and w.dim() == 2 and not w.is_cuda
    rows, inner = w.shape
    nb = blocks(inner)
    pad = nb * BLOCK - inner
    x = torch.nn.functional.pad(w, (0, pad)).double().reshape(rows, nb, BLOCK)
    neg = torch.signbit(torch.nn.functional.pad(w, (0, pad))).reshape(rows, nb, BLOCK)
    bad = ~torch.isfinite(x).all(2, keepdim=True)
    x = torch.where(bad, torch.zeros_like(x), x)
    a = x.abs()
    amax = a.amax(2, keepdim=True)
    E = torch.where(amax > 0, _floor_log2(torch.where(amax > 0, amax, torch.ones_like(amax))) - emax,
                    torch.full(amax.shape, -127, dtype=torch.int64)).clamp(-127, 127)
    X = _pow2(E)
    u = torch.clamp(a / X, max=vmax)                                     # exact; saturation before rounding
    eu = _floor_log2(torch.where(u > 0, u, torch.ones_like(u)))
    step = _pow2(torch.clamp(eu, min=emin) - M)                          # the spacing of the binade u lies in
    mag = torch.clamp(torch.round(u / step) * step, max=vmax)            # half to even; saturation after rounding
    # codes: subnormals m, normals (e - emin + 1) 2^M + (mantissa field)
    em = _floor_log2(torch.where(mag > 0, mag, torch.ones_like(mag)))
    normal = mag >= 2.0 ** emin
    field = torch.where(normal, ((em - emin + 1) << M) + (mag / _pow2(em - M)).to(torch.int64) - (1 << M),
                        (mag / 2.0 ** (emin - M)).to(torch.int64))
    codes = field + (neg.to(torch.int64) << (eb + M))
    q64 = torch.where(neg, -(mag * X), mag * X)
    wq = q64.float()
    assert torch.equal(wq.double(), q64), "wq is not exactly representable in float32"
    nan = torch.full_like(wq, float("nan"))
    wq = torch.where(bad, nan, wq).reshape(rows, nb * BLOCK)[:, :inner].contiguous()
    codes = torch.where(bad, torch.zeros_like(codes), codes).reshape(rows, nb * BLOCK)[:, :inner].to(torch.uint8).contiguous()
    scales = torch.where(bad, torch.full_like(E, 255), E + 127).reshape(rows, nb).to(torch.uint8).contiguous()
    d = w - wq                                                            # float32
    return {"wq": wq, "scales": scales, "codes": codes, "err": (d.double() * d.double()).sum(1), "energy": (w.double() * w.double()).sum(1)}


def dequantize(codes, scales, fmt):
    """codes uint8 [rows, inner], scales uint8 [rows, blocks] -> fp32 [rows, inner]; a scale code of 255 gives NaN"""
    _, eb, M, bias, _, _ = FORMATS[fmt]
    c = codes.to(torch.int64)
    neg = ((c >> (eb + M)) & 1).bool()
    ex, m = (c >> M) & ((1 << eb) - 1), (c & ((1 << M) - 1)).double()
    mag = torch.where(ex == 0, m * 2.0 ** (1 - bias - M), (1.0 + m / 2 ** M) * _pow2(ex - bias))
    sc = scales.to(torch.int64).repeat_interleave(BLOCK, dim=1)[:, :codes.shape[1]]
    val = mag * _pow2(sc - 127)
    val = torch.where(neg, -val, val)
    return torch.where(sc == 255, torch.full_like(val, float("nan")), val).float()
