"""Parts of the calibration engine that need no GPU: the conv / zero-insertion geometry helpers against torch's own output shapes, and the
context manager that swaps modules' forwards for the R + lambda*D tail (quantization/engine_rd.py)."""
import pytest
import torch
import torch.nn.functional as F

SIZES = [(5, 6), (8, 8)]


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("p", [0, 1, 2])
def test_conv_out_hw_is_torchs(H, W, k, s, p):
    from quantization.engine import conv_out_hw
    y = F.conv2d(torch.zeros(1, 1, H, W), torch.zeros(1, 1, k, k), stride=s, padding=p)
    assert conv_out_hw(H, W, k, s, p) == tuple(y.shape[-2:])


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("opad", [0, 1])
def test_zero_insert_hw_of_a_transposed_conv(H, W, k, p, opad):
    """the stride-1 / pad-0 conv of the zero-inserted map has the transposed conv's output size"""
    from quantization.engine import conv_out_hw, zero_insert_hw
    s = 2
    y = F.conv_transpose2d(torch.zeros(1, 1, H, W), torch.zeros(1, 1, k, k), stride=s, padding=p, output_padding=opad)
    q, Hu, Wu = zero_insert_hw(H, W, k, s, p, opad)
    assert q == k - 1 - p
    assert conv_out_hw(Hu, Wu, k, 1, 0) == tuple(y.shape[-2:])
    # the zero-inserted map itself: the elements s apart, q zeros in front, q + opad behind
    assert (Hu, Wu) == ((H - 1) * s + 1 + 2 * q + opad, (W - 1) * s + 1 + 2 * q + opad)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("p", [1, 2])
def test_zero_insert_hw_of_a_strided_convs_input_gradient(H, W, k, p):
    """dgrad of a strided conv = the transposed conv of dy whose output_padding restores the input size, axis by axis: 5 and 6 under
    k = 3 / s = 2 / p = 1 need 0 and 1, 8 needs 1"""
    from quantization.engine import conv_out_hw, zero_insert_hw
    from hipops import ops
    s = 2
    x = torch.zeros(1, 1, H, W)
    y = F.conv2d(x, torch.zeros(1, 1, k, k), stride=s, padding=p)
    assert conv_out_hw(H, W, k, s, p) == tuple(y.shape[-2:])
    opads = []
    for n, no in zip((H, W), y.shape[-2:]):
        opad = n - ops.tap_out_size(no, k, s, p, True)
        assert 0 <= opad < s
        opads.append(opad)
        dx = F.conv_transpose2d(torch.zeros(1, 1, no, no), torch.zeros(1, 1, k, k), stride=s, padding=p, output_padding=opad)
        assert tuple(dx.shape[-2:]) == (n, n)
        q, Hu, Wu = zero_insert_hw(no, no, k, s, p, opad)
        assert conv_out_hw(Hu, Wu, k, 1, 0) == (n, n)
    if (k, p) == (3, 1):
        assert tuple(opads) == {(5, 6): (0, 1), (8, 8): (1, 1)}[(H, W)]


def test_zero_insert_hw_refuses_padding_beyond_the_kernel():
    from quantization.engine import zero_insert_hw
    with pytest.raises(NotImplementedError):
        zero_insert_hw(4, 4, 3, 2, 3, 0)


def test_forwards_swaps_and_restores():
    from quantization.engine_rd import forwards
    torch.manual_seed(0)
    a, b = torch.nn.Linear(4, 3), torch.nn.Linear(3, 2)
    x = torch.randn(5, 4)
    want_a, want_b = a(x), b(a(x))
    with forwards({a: lambda t: t[:, :3] * 2.0, b: lambda t: t + 1.0}):
        assert torch.equal(a(x), x[:, :3] * 2.0)                 # the replacements run, through Module.__call__
        assert torch.equal(b(a(x)), x[:, :3] * 2.0 + 1.0)
    for m in (a, b):
        assert "forward" not in m.__dict__
    assert torch.equal(a(x), want_a) and torch.equal(b(a(x)), want_b)

    class Boom(RuntimeError):
        pass
    with pytest.raises(Boom):
        with forwards({a: lambda t: t[:, :3], b: lambda t: t}):
            assert "forward" in a.__dict__ and "forward" in b.__dict__
            raise Boom()
    for m in (a, b):
        assert "forward" not in m.__dict__
    assert torch.equal(a(x), want_a) and torch.equal(b(a(x)), want_b)

    with forwards({}):                                           # nothing to swap: nothing happens
        assert torch.equal(a(x), want_a)
    assert "forward" not in a.__dict__ and "forward" not in b.__dict__
