"""CPU checks of the MX codes on the block-scaled matrix instruction: include/rdo_ptq_mxgemm.h against `EXPORTS_MXGEMM` and the built
library, the refusals of the C entries (RDO_EINVAL without touching a device) and of the `ops.mx_*` wrappers, `rdo_mx_packed_bytes`, the
eligibility refusals of `mx.native_operand` and the argument refusals of `mx_native_report` on toy modules (no kernel runs), and the
reference's own properties (tests/mx_gemm_reference.py): pack / unpack, its decode against tests/mx_reference.py, and the exactness of
the exact-product inputs in fp32."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import mx_gemm_reference as G
import mx_reference as R

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rdo_mx_packed_bytes", "rdo_mx_pack_codes", "rdo_mx_quant_pack", "rdo_mx_unpack_codes", "rdo_mx_gemm"}
WQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
AQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}


def two_layer_model():
    """the smallest model with an eligible module: a 3x3 conv 3 -> 32 (not eligible), LeakyReLU, a 1x1 conv 32 -> 16 (eligible)"""
    from quantization import QuantModel
    torch.manual_seed(11)
    net = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv2d(32, 16, 1))
    return QuantModel(net.eval(), WQ, AQ).eval()


# ----------------------------------------------------------------------------- the header, the exports
def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxgemm.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXGEMM) == NAMES
    assert '#include "rdo_ptq_mx.h"' in hdr
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_BIAS, L.EXPORTS_BITS, L.EXPORTS_PACK, L.EXPORTS_SUBPEL, L.EXPORTS_ACTBITS, L.EXPORTS_ATTNQ,
              L.EXPORTS_MX, L.EXPORTS_MXROUND)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert len(L.EXPORTS) == 124 and len(L.EXPORTS_MX) == 4 and len(L.EXPORTS_MXROUND) == 4


def test_packed_bytes():
    from hipops import _lib as L
    h = L.lib()
    for fmt in R.NAMES:
        fid, bits = L.MX_FORMATS[fmt]
        assert h.rdo_mx_packed_bytes(3, 96, fid) == 3 * 3 * 4 * bits == G.pack(np.zeros((3, 96), np.uint8), fmt).size
        assert h.rdo_mx_packed_bytes(1, 32, fid) == {4: 16, 6: 24, 8: 32}[bits]
        assert h.rdo_mx_packed_bytes(2 ** 20, 2 ** 25, fid) == 2 ** 40 * 4 * bits                     # exactly 2^40 blocks
        for rows, K in ((0, 32), (-1, 32), (3, 0), (3, -32), (3, 40), (3, 31), (2 ** 31 - 1, 2 ** 40), (2 ** 20, 2 ** 25 + 32)):
            assert h.rdo_mx_packed_bytes(rows, K, fid) == 0, (rows, K)
    assert h.rdo_mx_packed_bytes(3, 96, -1) == 0 and h.rdo_mx_packed_bytes(3, 96, 5) == 0


def test_c_entries_refuse_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    odd = C.c_void_p(C.addressof(buf) + 2)

    def refused(fn, names, base, bad, who):
        for kw in bad:
            a = dict(base, **kw)
            assert fn(*[a[n] for n in names], None) == RDO_EINVAL, (who, kw)
            assert who.encode() in h.rdo_last_error(), (who, kw)

    sizes = [dict(rows=0), dict(rows=-3), dict(K=0), dict(K=-32), dict(K=40), dict(K=33), dict(format=-1), dict(format=5),
             dict(rows=2 ** 31 - 1, K=2 ** 40)]
    refused(h.rdo_mx_pack_codes, ["codes", "rows", "K", "format", "packed"], dict(codes=p, rows=3, K=64, format=0, packed=p),
            [dict(codes=None), dict(packed=None), dict(packed=odd)] + sizes, "rdo_mx_pack_codes")
    refused(h.rdo_mx_unpack_codes, ["packed", "rows", "K", "format", "codes"], dict(packed=p, rows=3, K=64, format=1, codes=p),
            [dict(codes=None), dict(packed=None), dict(packed=odd)] + sizes, "rdo_mx_unpack_codes")
    refused(h.rdo_mx_quant_pack, ["x", "rows", "K", "format", "packed", "scales", "xq"],
            dict(x=p, rows=3, K=64, format=3, packed=p, scales=p, xq=None),
            [dict(x=None), dict(packed=None), dict(scales=None), dict(x=odd), dict(packed=odd), dict(xq=odd)] + sizes, "rdo_mx_quant_pack")
    gemm = ["a", "sa", "fa", "b", "sb", "fb", "M", "N", "K", "bias", "y"]
    refused(h.rdo_mx_gemm, gemm, dict(a=p, sa=p, fa=0, b=p, sb=p, fb=4, M=5, N=7, K=64, bias=None, y=p),
            [dict(a=None), dict(sa=None), dict(b=None), dict(sb=None), dict(y=None), dict(a=odd), dict(b=odd), dict(bias=odd), dict(y=odd),
             dict(M=0), dict(M=-1), dict(N=0), dict(N=-5), dict(K=0), dict(K=-64), dict(K=48), dict(fa=-1), dict(fa=5), dict(fb=-1), dict(fb=5),
             dict(M=2 ** 31 - 1, K=2 ** 40), dict(N=2 ** 31 - 1, K=2 ** 40)], "rdo_mx_gemm")


# ----------------------------------------------------------------------------- the wrappers
@pytest.fixture()
def no_library(monkeypatch):
    """any library call or pointer conversion after the argument checks fails the test"""
    from hipops import _lib as L
    from hipops import ops

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(ops, "_ptr", boom)
    return ops


def test_wrappers_refuse_malformed_operands(no_library):
    ops = no_library
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    good = ops.MXOperand(u8(3, 2 * 16), u8(3, 2), "mxfp4", 3, 64)
    cases = [
        (ops.mx_quant_pack, (torch.zeros(3, 64).double(), "mxfp4"), "mx_quant_pack: x2d must be an fp32 tensor"),
        (ops.mx_quant_pack, (torch.zeros(192), "mxfp4"), "mx_quant_pack: .*rank 2"),
        (ops.mx_quant_pack, (torch.zeros(3, 128)[:, ::2], "mxfp4"), "mx_quant_pack: .*contiguous"),
        (ops.mx_quant_pack, (torch.zeros(3, 64), "mxfp5"), "mx_quant_pack: unknown MX format 'mxfp5'; the formats are"),
        (ops.mx_quant_pack, (torch.zeros(3, 40), "mxfp4"), "mx_quant_pack: K = 40 is no multiple of the MX block size 32"),
        (ops.mx_quant_pack, (torch.zeros(3, 64), "mxfp4"), "mx_quant_pack: .*no CPU path"),
        (ops.mx_pack_codes, (torch.zeros(3, 64), u8(3, 2), "mxfp4"), "mx_pack_codes: codes must be an uint8 tensor"),
        (ops.mx_pack_codes, (u8(3, 72), u8(3, 3), "mxfp4"), "mx_pack_codes: K = 72 is no multiple"),
        (ops.mx_pack_codes, (u8(3, 64), u8(3, 3), "mxfp4"), "mx_pack_codes: scales must be a contiguous uint8 \\[3, 2\\]"),
        (ops.mx_pack_codes, (u8(3, 64), u8(3, 2), "fp4"), "mx_pack_codes: unknown MX format 'fp4'"),
        (ops.mx_pack_codes, (u8(3, 64), u8(3, 2), "mxfp4"), "mx_pack_codes: .*no CPU path"),
        (ops.mx_unpack_codes, (u8(3, 32),), "mx_unpack_codes: op must be an MXOperand, got Tensor"),
        (ops.mx_unpack_codes, (ops.MXOperand(u8(3, 32), u8(3, 2), "mxfp6_e2m3", 3, 64),), "mx_unpack_codes: op.packed must be a contiguous uint8 \\[3, 48\\]"),
        (ops.mx_unpack_codes, (ops.MXOperand(u8(3, 32), u8(3, 1), "mxfp4", 3, 64),), "mx_unpack_codes: op.scales must be a contiguous uint8 \\[3, 2\\]"),
        (ops.mx_unpack_codes, (ops.MXOperand(u8(3, 20), u8(3, 2), "mxfp4", 3, 40),), "mx_unpack_codes: K = 40 is no multiple"),
        (ops.mx_unpack_codes, (good,), "mx_unpack_codes: .*no CPU path"),
        (ops.mx_gemm, (good, None), "mx_gemm: b must be an MXOperand, got NoneType"),
        (ops.mx_gemm, (good, ops.MXOperand(u8(5, 32), u8(5, 1), "mxfp8_e4m3", 5, 32)), "mx_gemm: a has K = 64, b has K = 32"),
        (ops.mx_gemm, (good, ops.MXOperand(u8(5, 64), u8(5, 2), "mxfp8_e4m3", 5, 64), torch.zeros(3)), "mx_gemm: bias must be a contiguous fp32 \\[5\\]"),
        (ops.mx_gemm, (good, ops.MXOperand(u8(5, 64), u8(5, 2), "mxfp9", 5, 64)), "mx_gemm: unknown MX format 'mxfp9'"),
        (ops.mx_gemm, (good, ops.MXOperand(u8(5, 64), u8(5, 2), "mxfp8_e4m3", 5, 64), torch.zeros(5)), "mx_gemm: .*no CPU path"),
    ]
    for fn, args, what in cases:
        with pytest.raises(ValueError, match=what):
            fn(*args)


# ----------------------------------------------------------------------------- native_operand, mx_native_report
def test_native_operand_refuses_what_is_not_eligible():
    from quantization import QuantModule
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer, native_linear, native_operand, native_refusal

    def module(org, q=None):
        m = QuantModule(org, WQ, AQ)
        if q is not None:
            m.weight_quantizer = q
        return m
    cases = [
        (module(nn.Linear(40, 8), MXQuantizer("mxfp4")), "its 40 input channels are no multiple of the MX block size 32"),
        (module(nn.Linear(64, 8)), "its weight quantiser is a UniformAffineQuantizer"),
        (module(nn.Conv2d(32, 8, 3, padding=1), MXQuantizer("mxfp4")), "kernel \\(3, 3\\).* is not a 1x1 stride-1 unpadded conv"),
        (module(nn.Conv2d(32, 8, 1, stride=2), MXQuantizer("mxfp4")), "stride \\(2, 2\\).* is not a 1x1 stride-1 unpadded conv"),
        (module(nn.Conv2d(32, 8, 1, padding=1), MXQuantizer("mxfp4")), "padding \\(1, 1\\).* is not a 1x1 stride-1 unpadded conv"),
        (module(nn.Conv2d(24, 8, 1), MXAdaRoundQuantizer("mxfp6_e2m3")), "its 24 input channels are no multiple"),
        (module(nn.ConvTranspose2d(32, 8, 1), MXQuantizer("mxfp4", tconv=True)), "a tconv module is not GEMM-shaped"),
        (module(nn.LayerNorm(32), MXQuantizer("mxfp4")), "a layernorm module is not GEMM-shaped"),
    ]
    for m, why in cases:
        assert re.search(why, native_refusal(m))
        with pytest.raises(ValueError, match=f"native_operand: module QuantModule\\({m.kind}, .*{why}"):
            native_operand(m)
        with pytest.raises(ValueError, match="native_operand: module"):
            native_linear(m, torch.zeros(2, 40), "mxfp8_e4m3")
    # what is eligible goes on to the kernels, which have no CPU path
    for org, q, x in ((nn.Linear(64, 8), MXQuantizer("mxfp4"), torch.zeros(2, 3, 64)),
                      (nn.Conv2d(32, 8, 1), MXAdaRoundQuantizer("mxfp8_e5m2"), torch.zeros(2, 32, 3, 3))):
        m = module(org, q)
        assert native_refusal(m) is None
        with pytest.raises(ValueError, match="mx_fakequant: .*no CPU path"):
            native_linear(m, x, "mxfp8_e4m3")
        assert m._pack_memo == {}


def test_quantisers_still_refuse_activations_and_point_to_native_linear():
    from quantization.mx import MXAdaRoundQuantizer, MXQuantizer
    for cls in (MXQuantizer, MXAdaRoundQuantizer):
        with pytest.raises(NotImplementedError, match=f"{cls.__name__}\\(mxfp4\\): MX activations are not built.*native_linear"):
            cls("mxfp4")(torch.zeros(2, 32), True)


def test_report_refuses_bad_arguments_before_any_gpu_work(monkeypatch):
    from hipops import ops
    from quantization import dp
    qnn = two_layer_model()
    monkeypatch.setattr(ops, "_ptr", lambda *a, **k: (_ for _ in ()).throw(AssertionError("reached the library")))
    qnn.set_weight_format("mxfp4")
    images = torch.rand(2, 3, 32, 32)
    assert list(qnn.units()) == ["0", "2"]
    for kw, what in ((dict(images=images.double()), "images must be an fp32 tensor"), (dict(images=images[0]), "images must be \\[n, 3, H, W\\]"),
                     (dict(batch=0), "batch must be an integer >= 1"), (dict(units=["9"]), "unknown unit name\\(s\\) \\['9'\\]"),
                     (dict(act_fmt="mxfp5"), "unknown MX format 'mxfp5'; the formats are"),
                     (dict(units=["0"]), "unit '0' holds no eligible module: .*kernel \\(3, 3\\)")):
        with pytest.raises(ValueError, match=f"mx_native_report: {what}"):
            qnn.mx_native_report(**dict(dict(images=images), **kw))
    qnn.set_weight_format("int")
    with pytest.raises(ValueError, match="mx_native_report: unit '2' holds no eligible module: .*UniformAffineQuantizer"):
        qnn.mx_native_report(images, units=["2"])
    monkeypatch.setattr(dp, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="mx_native_report: not built for data-parallel runs \\(world_size > 1\\)"):
        qnn.mx_native_report(images)


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("fmt", R.NAMES)
def test_reference_pack_and_decode(fmt):
    b = R.element_bits(fmt)
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 1 << b, (3, 96)).astype(np.uint8)
    packed = G.pack(codes, fmt)
    assert packed.shape == (3, 3 * 4 * b) and packed.dtype == np.uint8
    assert (G.unpack(packed, 96, fmt) == codes).all()
    # element j of a block occupies bits [j b, (j + 1) b) of the block's little-endian bit string
    for r, j in ((0, 0), (1, 5), (2, 31), (0, 37), (2, 95)):
        blk = packed[r, (j // 32) * 4 * b:(j // 32 + 1) * 4 * b]
        word = int.from_bytes(blk.tobytes(), "little")
        assert (word >> ((j % 32) * b)) & ((1 << b) - 1) == int(codes[r, j])
    if b == 8:
        assert (packed == codes).all()
    if b == 4:
        assert (packed == (codes[:, 0::2] | (codes[:, 1::2] << 4))).all()
    # the decode is mx_reference's, for every finite code under several scales
    fin = G.finite_codes(fmt)
    n = -(-fin.size // 32) * 32
    c = np.zeros((1, n), np.uint8)
    c[0, :fin.size] = fin
    for s in (120, 127, 134):
        sc = np.full((1, n // 32), s, np.uint8)
        mine, theirs = G.decode(c, sc, fmt), R.dequantize(G.to_torch(c), G.to_torch(sc), fmt).double().numpy()
        assert (mine == theirs).all() and (np.signbit(mine) == np.signbit(theirs)).all()
    assert fin.size == {"mxfp4": 16, "mxfp6_e2m3": 64, "mxfp6_e3m2": 64, "mxfp8_e4m3": 254, "mxfp8_e5m2": 248}[fmt]
    for v in G.EXACT_MAGNITUDES:
        assert G.decode_elements(G.code_of(v, fmt), fmt) == v and G.decode_elements(G.code_of(-v, fmt), fmt) == -v
    # round trip with the quantiser's reference: codes of quantised data decode to its wq
    w = (torch.distributions.StudentT(3.0).sample((3, 64)) * 0.01).float()
    q = R.quantize(w, fmt)
    assert (G.decode(q["codes"].numpy(), q["scales"].numpy(), fmt) == q["wq"].double().numpy()).all()


def test_reference_fp32_chain_reproduces_the_float64_product_on_the_exact_inputs():
    cases = [(fa, fb, 16, 16, 128) for fa in R.NAMES for fb in R.NAMES] + [(fa, fb, *s) for fa, fb in G.EXACT_PAIRS for s in G.EXACT_SHAPES]
    assert len(cases) == 25 + 12
    for i, (fa, fb, M, N, K) in enumerate(cases):
        c = G.exact_case(fa, fb, M, N, K, seed=i)
        a, b = G.decode(c["a_codes"], c["a_scales"], fa), G.decode(c["b_codes"], c["b_scales"], fb)
        assert set(np.unique(np.abs(G.decode_elements(c["a_codes"], fa)))) <= set(G.EXACT_MAGNITUDES)
        assert set(np.unique(c["a_scales"])) <= {126, 127, 128} and (np.abs(c["bias"]) < 8).all() and (c["bias"] * 16 == np.round(c["bias"] * 16)).all()
        ref = c["ref"]
        assert (ref * 16 == np.round(ref * 16)).all() and np.abs(ref).max() < 2.0 ** 20
        assert (G.chain32(a, b, c["bias"]).astype(np.float64) == ref).all()
        assert (G.chain32(a[:, ::-1], b[:, ::-1], c["bias"]).astype(np.float64) == ref).all()          # ... in another order too
        assert M != N or not (a.shape == b.shape and (a == b).all())
