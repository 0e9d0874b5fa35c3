"""CPU checks of the entropy / rate surface: the eight wrappers of hipops.ops refuse mismatched operands with ValueError before any
pointer is taken or library call made (each such call would be an out-of-bounds device access), and the C entry points of
csrc/entropy.hip return RDO_EINVAL with a message for null pointers and non-positive counts without touching a device."""
import ctypes as C

import pytest
import torch

RDO_EINVAL = -22


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


def _t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_factorized_wrappers_refuse_mismatched_operands(no_library):
    ops = no_library
    z, params, med = _t(4, 5, 6), _t(6, 58), _t(6)
    bad = [
        (z, _t(5, 58), med),                        # params of another channel count
        (z, _t(6, 57), med),
        (z, _t(6 * 58), med),
        (z, params, _t(5)),                         # medians of another channel count
        (z, params, _t(6, 1)),
        (z, params.double(), med),
        (z, params, med.double()),
        (z.double(), params, med),
        (z.half(), params, med),
        (_t(0, 6), params, med),                    # empty
        (_t(()), _t(0, 58), _t(0)),
        (z, None, med),
        (z, params, None),
    ]
    for args in bad:
        with pytest.raises(ValueError, match="factorized_likelihood"):
            ops.factorized_likelihood(*args)
    for args in [(z, _t(5, 58)), (z, _t(6, 57)), (z, params.double()), (z.to(torch.int32), params), (_t(0, 6), params), (z, None)]:
        with pytest.raises(ValueError, match="factorized_likelihood_bwd"):
            ops.factorized_likelihood_bwd(*args)


def test_gaussian_wrappers_refuse_mismatched_operands(no_library):
    ops = no_library
    y, s, m = _t(2, 3, 4, 5), _t(2, 3, 4, 5), _t(2, 3, 4, 5)
    bad = [
        (y, _t(2, 3, 4, 4), m),                     # fewer scales than y
        (y, s, _t(2, 3, 4, 4)),                     # fewer means than y
        (y, _t(1), m),
        (y, s, _t(1)),
        (y, s.double(), m),
        (y, s, m.double()),
        (y.double(), s, m),
        (_t(0), _t(0), _t(0)),
        (_t(0), _t(0), None),
        (y, None, m),
    ]
    for args in bad:
        with pytest.raises(ValueError, match="gaussian_likelihood"):
            ops.gaussian_likelihood(*args)
        with pytest.raises(ValueError, match="gaussian_likelihood_bwd"):
            ops.gaussian_likelihood_bwd(*args)


@pytest.mark.parametrize("name", ["neg_log2_sum", "neg_log2_sum_ordered"])
def test_log_sum_wrappers_refuse_mismatched_operands(no_library, name):
    fn = getattr(no_library, name)
    lik = _t(100)
    for args, kw in [((lik.double(),), {}), ((_t(0),), {}), ((lik,), {"out": _t(2)}), ((lik,), {"out": _t(0)}), ((lik,), {"out": _t(1).double()}),
                     ((lik,), {"out": _t(1, dtype=torch.int32)}), ((lik,), {"out": 0.0}), ((None,), {})]:
        with pytest.raises(ValueError, match=name):
            fn(*args, **kw)


@pytest.mark.parametrize("name", ["sq_diff_sum", "sq_diff_sum_ordered"])
def test_sq_sum_wrappers_refuse_mismatched_operands(no_library, name):
    fn = getattr(no_library, name)
    a, b = _t(100), _t(100)
    for args, kw in [((a, _t(99)), {}), ((_t(99), b), {}), ((a, b.double()), {}), ((a.half(), b.half()), {}), ((_t(0), _t(0)), {}),
                     ((a, b), {"out": _t(2)}), ((a, b), {"out": _t(1).double()}), ((a, b), {"out": _t(1, 2)}), ((a, None), {})]:
        with pytest.raises(ValueError, match=name):
            fn(*args, **kw)


def test_out_on_another_device_is_refused(no_library):
    ops = no_library
    lik = _t(10)
    out = torch.zeros(1, device="meta")
    for fn, args in ((ops.neg_log2_sum, (lik,)), (ops.neg_log2_sum_ordered, (lik,)), (ops.sq_diff_sum, (lik, lik)), (ops.sq_diff_sum_ordered, (lik, lik))):
        with pytest.raises(ValueError, match="out must be one fp32 element"):
            fn(*args, out=out)
    with pytest.raises(ValueError, match="gaussian_likelihood"):
        ops.gaussian_likelihood(lik, torch.zeros(10, device="meta"))
    with pytest.raises(ValueError, match="factorized_likelihood"):
        ops.factorized_likelihood(_t(5, 2), torch.zeros(2, 58, device="meta"), _t(2))


def test_well_formed_cpu_operands_reach_the_pointer_check():
    """the argument checks pass well-formed operands on: a CPU tensor is then refused by `_ptr` (no CPU path), still before any launch"""
    from hipops import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gaussian_likelihood(_t(7), _t(7), _t(7))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.factorized_likelihood(_t(3, 2), _t(2, 58), _t(2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sq_diff_sum(_t(7), _t(7), out=_t(1))


def test_c_abi_refuses_null_pointers_and_non_positive_counts():
    """RDO_REQUIRE runs before any launch: the non-null arguments below are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))

    def refused(rc, name):
        assert rc == RDO_EINVAL, (name, rc)
        assert name.encode() in h.rdo_last_error(), (name, h.rdo_last_error())

    f = h.rdo_factorized_likelihood_fwd
    for args in [(None, p, p, 8, 2, p, p), (p, None, p, 8, 2, p, p), (p, p, None, 8, 2, p, p), (p, p, p, 8, 2, None, p), (p, p, p, 8, 2, p, None),
                 (p, p, p, 0, 2, p, p), (p, p, p, -8, 2, p, p), (p, p, p, 8, 0, p, p), (p, p, p, 8, -1, p, p)]:
        refused(f(*args, None), "rdo_factorized_likelihood_fwd")
    f = h.rdo_factorized_likelihood_bwd
    for args in [(None, p, 8, 2, 1.0, p), (p, None, 8, 2, 1.0, p), (p, p, 8, 2, 1.0, None), (p, p, 0, 2, 1.0, p), (p, p, -1, 2, 1.0, p),
                 (p, p, 8, 0, 1.0, p), (p, p, 8, -2, 1.0, p)]:
        refused(f(*args, None), "rdo_factorized_likelihood_bwd")
    f = h.rdo_gaussian_likelihood_fwd
    for args in [(None, p, p, 8, 0.11, p, p), (p, None, p, 8, 0.11, p, p), (p, p, p, 8, 0.11, p, None), (p, p, None, 0, 0.11, None, p),
                 (p, p, p, -3, 0.11, p, p)]:
        refused(f(*args, None), "rdo_gaussian_likelihood_fwd")
    f = h.rdo_gaussian_likelihood_bwd
    for args in [(None, p, p, 8, 0.11, 1.0, p, p), (p, None, p, 8, 0.11, 1.0, p, p), (p, p, p, 8, 0.11, 1.0, None, None),      # both outputs null
                 (p, p, None, 8, 0.11, 1.0, None, None), (p, p, p, 0, 0.11, 1.0, p, p), (p, p, p, -8, 0.11, 1.0, p, None)]:
        refused(f(*args, None), "rdo_gaussian_likelihood_bwd")
    for args in [(None, 8, 1.0, p), (p, 8, 1.0, None), (p, 0, 1.0, p), (p, -1, 1.0, p)]:
        refused(h.rdo_neg_log2_sum(*args, None), "rdo_neg_log2_sum")
    for args in [(None, 8, 1.0, p, p), (p, 8, 1.0, None, p), (p, 8, 1.0, p, None), (p, 0, 1.0, p, p)]:
        refused(h.rdo_neg_log2_sum_ordered(*args, None), "rdo_neg_log2_sum_ordered")
    for args in [(None, p, 8, 1.0, 0, p), (p, None, 8, 1.0, 0, p), (p, p, 8, 1.0, 1, None), (p, p, 0, 1.0, 0, p), (p, p, -8, 1.0, 0, p)]:
        refused(h.rdo_sq_diff_sum(*args, None), "rdo_sq_diff_sum")
    for args in [(None, p, 8, 1.0, 0, p, p), (p, None, 8, 1.0, 0, p, p), (p, p, 8, 1.0, 0, None, p), (p, p, 8, 1.0, 0, p, None), (p, p, 0, 1.0, 1, p, p)]:
        refused(h.rdo_sq_diff_sum_ordered(*args, None), "rdo_sq_diff_sum_ordered")
    assert h.rdo_ordered_sum_workspace() == 2048
