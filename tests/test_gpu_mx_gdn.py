"""GPU checks of the one-launch MX GDN / IGDN (include/rdo_ptq_mxgdn.h): the norm pool against the composition it fuses, bit for bit;
y against float64; the packed output against `ops.mx_quant_pack` of the fp32 output; a non-finite row; and the module level -- the
`gdn` flag of `set_mx_activations`, native against emulated, the chain into a conv, and the packed checkpoint."""
import numpy as np
import pytest
import torch

from test_mx_gdn_args import gdn_model

pytestmark = pytest.mark.gpu

# rows 70: a last tile of 6 rows; 20: one part-filled tile.  C 32: one block of a 4-block K step, two units for four waves; 96: a 3-of-4
# K tail, six units; 160: two K steps, the second with one block
SHAPES = [(70, 32), (70, 96), (70, 160), (20, 32), (20, 96), (20, 160)]
PAIRS = [("mxfp4", "mxfp4"), ("mxfp8_e4m3", "mxfp6_e2m3"), ("mxfp6_e3m2", "mxfp8_e5m2")]      # (x o x, gamma')
_DATA = {}


def _data(C):
    """x = 0.5 t(3) [70, C], gamma' = 0.05 |t(3)| [C, C], beta' in [0.5, 1.5]: seeded, made once per C and shared unchanged"""
    if C not in _DATA:
        rng = np.random.RandomState(900 + C)
        x = torch.from_numpy((0.5 * rng.standard_t(3, (70, C))).astype(np.float32)).cuda()
        gamma = torch.from_numpy((0.05 * np.abs(rng.standard_t(3, (C, C)))).astype(np.float32)).cuda()
        beta = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)).cuda()
        _DATA[C] = (x, gamma, beta, {})
    return _DATA[C]


def _case(rows, C, fg):
    from hipops import ops
    x, gamma, beta, packed = _data(C)
    if fg not in packed:
        packed[fg] = ops.mx_quant_pack(gamma, fg)
    return x[:rows].contiguous(), packed[fg], beta


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("rows,C", SHAPES)
@pytest.mark.parametrize("fx,fg", PAIRS)
def test_norm_is_the_gemm_of_the_packed_squares_and_y_is_within_two_roundings(fx, fg, rows, C, inverse):
    from hipops import ops
    x, g, beta = _case(rows, C, fg)
    y, norm = ops.mx_gdn(x, g, beta, fx, inverse=inverse, want_norm=True)
    assert torch.equal(norm, ops.mx_gemm(ops.mx_quant_pack(x * x, fx), g, beta)) and float(norm.min()) >= 0.5
    # two correctly rounded fp32 operations on the fp32 norm: (1 + 2^-24)^2 - 1 < 2^-22
    ref = x.double() * norm.double() ** (0.5 if inverse else -0.5)
    ratio = float(((y.double() - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    print(f"worst |y - ref| / |ref| = {ratio * 2 ** 22:.4f} x 2^-22")
    assert bool(((y.double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all())
    assert torch.equal(y, ops.mx_gdn(x, g, beta, fx, inverse=inverse))                 # without the norm store


@pytest.mark.parametrize("out_fmt", ["mxfp4", "mxfp6_e2m3", "mxfp8_e4m3"])
@pytest.mark.parametrize("rows,C,inverse", [(70, 96, False), (20, 160, True), (70, 32, True)])
def test_packed_output_is_quant_pack_of_the_fp32_output(out_fmt, rows, C, inverse):
    from hipops import ops
    fx, fg = PAIRS[1]
    x, g, beta = _case(rows, C, fg)
    got, norm = ops.mx_gdn(x, g, beta, fx, inverse=inverse, out_fmt=out_fmt, want_norm=True)
    y, norm32 = ops.mx_gdn(x, g, beta, fx, inverse=inverse, want_norm=True)
    want = ops.mx_quant_pack(y, out_fmt)
    assert (got.fmt, got.rows, got.K) == (out_fmt, rows, C) and torch.equal(norm, norm32)
    assert torch.equal(got.scales, want.scales) and torch.equal(ops.mx_unpack_codes(got), ops.mx_unpack_codes(want))


def test_an_infinity_in_one_row_stays_in_its_row():
    from hipops import ops
    fx, fg = PAIRS[1]
    x, g, beta = _case(70, 96, fg)
    bad = x.clone()
    bad[37, 40] = float("inf")
    keep = torch.arange(70, device="cuda") != 37
    assert torch.equal(ops.mx_gdn(bad, g, beta, fx)[keep], ops.mx_gdn(x, g, beta, fx)[keep])
    got, want = ops.mx_gdn(bad, g, beta, fx, out_fmt="mxfp6_e2m3"), ops.mx_gdn(x, g, beta, fx, out_fmt="mxfp6_e2m3")
    assert torch.equal(got.scales[keep], want.scales[keep]) and torch.equal(got.packed[keep], want.packed[keep])
    # the norm of row 37 sums over the block that holds the infinity: every block of its y is non-finite
    assert bool((got.scales[37] == 255).all()) and not ops.mx_unpack_codes(got)[37].any()


def test_switched_gdn_modules_native_emulated_chained_and_stored(tmp_path):
    from quantization import mx
    from quantization.mx_packed import load_mx_packed, save_mx_packed
    fmt = "mxfp8_e4m3"
    qnn = gdn_model().cuda()
    qnn.set_weight_format("mxfp6_e2m3")
    qnn.set_quant_state(True, False)
    rep = qnn.set_mx_activations(fmt, "native", gdn=True)
    assert dict(rep["native"]) == {"0": "conv", "1": "gdn", "2": "conv", "3": "gdn"}
    rng = np.random.RandomState(7)
    x = torch.from_numpy((0.5 * rng.standard_t(3, (2, 32, 7, 9))).astype(np.float32)).cuda()
    conv1, gdn, conv2, igdn = (qnn.model[i] for i in range(4))
    with torch.no_grad():
        h = conv1(x)
        y = gdn(h)
        assert torch.equal(y, mx.native_gdn(gdn, h, fmt))
        assert torch.equal(mx.native_gdn_chain(gdn, conv2, h, fmt), mx.native_conv(conv2, y, fmt))
        h2 = conv2(y)
        out = qnn(x)
        assert torch.equal(out, igdn(h2))
        # Native and emulated pools sum the same exact products a_k b_k >= 0 and beta' > 0, each within K 2^-23 (sum |a b| + |beta|) =
        # K 2^-23 n of the real sum n (include/rdo_ptq_mxgemm.h), so the two norms differ by at most 2 K 2^-23 n; n^-+1/2 halves a
        # relative error (to first order; 2^-10 more covers the second), and each side rounds rsqrt / sqrt and the product: 2 x 2^-22.
        for m, inp, nat in ((gdn, h, y), (igdn, h2, out)):
            m.mx_activations = (fmt, "emulated")
            emu = m(inp)
            m.mx_activations = (fmt, "native")
            K = int(m.weight.shape[0])
            bound = (K * 2.0 ** -23 * (1 + 2.0 ** -10) + 2.0 ** -21) * emu.double().abs()
            assert bool(((nat.double() - emu.double()).abs() <= bound).all()) and float(emu.abs().max()) > 0
        path = str(tmp_path / "gdn.rdomx")
        save_mx_packed(qnn, path)
        fresh = gdn_model().cuda()
        load_mx_packed(fresh, path)
        fresh.set_quant_state(True, False)
        assert fresh.model[1].mx_activations == (fmt, "native") and fresh.model[3].mx_activations == (fmt, "native")
        assert torch.equal(fresh(x), out)
