"""The argument checks every host wrapper shares (hipops/_args.py) and the workspace cache of hipops/ops.py: the messages, their order
and the cache rules, on the CPU and without a library call."""
import numpy as np
import pytest
import torch

F32, F64, I32 = torch.float32, torch.float64, torch.int32


def _t(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


def test_the_module_stands_alone():
    """`_args` is pure: it imports neither the library loader nor the wrappers"""
    import hipops._args as A
    with open(A.__file__) as f:
        imports = [line.split()[1] for line in f if line.startswith(("import ", "from "))]
    assert sorted(imports) == ["numbers", "torch"]


REF = _t(2, 3)                       # a CPU reference operand
ONE = dict(oneshot=True)
TENSOR_CASES = [
    # stepwise: one message per condition
    ("stepwise non-tensor", 0.5, {}, "t must be an fp32 tensor, got float"),
    ("stepwise None", None, {}, "t must be an fp32 tensor, got NoneType"),
    ("stepwise dtype", _t(2, 3, dtype=F64), {}, "t must be an fp32 tensor, got torch.float64"),
    ("stepwise dtype word", _t(2, 3), dict(dtype=F64, word="float64"), "t must be a float64 tensor, got torch.float32"),
    ("stepwise dtype word int", _t(2, 3), dict(dtype=I32, word="int32"), "t must be an int32 tensor, got torch.float32"),
    ("stepwise rank", _t(2, 3, 4), dict(rank=2, layout="of rank 2 [rows, inner]"), "t must be of rank 2 \\[rows, inner\\], got rank 3"),
    ("stepwise rank, no layout", _t(6), dict(rank=2), "t must be of rank 2, got rank 1"),
    ("stepwise shape", _t(3, 2), dict(shape=(2, 3)), "t has shape \\(3, 2\\), expected \\(2, 3\\)"),
    ("stepwise count", _t(5), dict(numel=6), "t holds 5 elements, expected 6"),
    ("stepwise empty", _t(2, 0), {}, "t is empty"),
    ("stepwise strided", _t(2, 6)[:, ::2], dict(contiguous=True), "t must be contiguous"),
    ("stepwise device", torch.zeros(2, 3, device="meta"), dict(device=REF.device, other="w_ref"), "t is on meta, w_ref on cpu"),
    ("stepwise device, unnamed", torch.zeros(2, 3, device="meta"), dict(device=REF.device), "t is on meta, the other operands on cpu"),
    # the order: dtype, rank, empty, contiguous, device, count, shape
    ("order dtype < contiguous", _t(2, 6, dtype=F64)[:, ::2], dict(contiguous=True), "t must be an fp32 tensor"),
    ("order rank < empty", _t(0), dict(rank=2), "t must be of rank 2, got rank 1"),
    ("order empty < contiguous", _t(0, 6)[:, ::2], dict(contiguous=True), "t is empty"),
    ("order contiguous < device", torch.zeros(2, 6, device="meta")[:, ::2], dict(contiguous=True, device=REF.device), "t must be contiguous"),
    ("order device < count", torch.zeros(5, device="meta"), dict(device=REF.device, numel=6), "t is on meta"),
    ("order count < shape", _t(5), dict(numel=6, shape=(2, 3)), "t holds 5 elements"),
    # one-shot: the whole requirement in one message, whatever fails
    ("one-shot non-tensor", 0.5, dict(shape=(9, 4), contiguous=True, device=REF.device, **ONE),
     "t must be a contiguous fp32 \\[9, 4\\] on cpu, got float$"),
    ("one-shot None", None, dict(shape=(4,), contiguous=True, **ONE), "t must be a contiguous fp32 \\[4\\], got NoneType$"),
    ("one-shot dtype", _t(9, 4, dtype=F64), dict(shape=(9, 4), contiguous=True, device=REF.device, **ONE),
     "t must be a contiguous fp32 \\[9, 4\\] on cpu, got \\(torch.float64, \\(9, 4\\), device\\(type='cpu'\\)\\)"),
    ("one-shot dtype word", _t(3, 7), dict(dtype=I32, word="int32", shape=(3, 7), contiguous=True, **ONE), "t must be a contiguous int32 \\[3, 7\\], got"),
    ("one-shot rank", _t(6), dict(rank=2, **ONE), "t must be a non-empty fp32 tensor of rank 2, got"),
    ("one-shot shape", _t(4, 9), dict(shape=(9, 4), contiguous=True, **ONE), "t must be a contiguous fp32 \\[9, 4\\], got .*\\(4, 9\\)"),
    ("one-shot shape, strides free", _t(3, 58), dict(shape=(4, 58), **ONE), "t must be fp32 \\[4, 58\\], got"),
    ("one-shot count", _t(2), dict(numel=1, device=REF.device, **ONE), "t must be one fp32 element on cpu, got"),
    ("one-shot count > 1", _t(5), dict(numel=6, contiguous=True, **ONE), "t must be 6 contiguous fp32 elements, got"),
    ("one-shot empty", _t(0, 3), dict(rank=2, contiguous=True, **ONE), "t must be a non-empty contiguous fp32 tensor of rank 2, got"),
    ("one-shot strided", _t(9, 8)[:, ::2], dict(shape=(9, 4), contiguous=True, **ONE), "t must be a contiguous fp32 \\[9, 4\\], got"),
    ("one-shot device", torch.zeros(9, 4, device="meta"), dict(shape=(9, 4), contiguous=True, device=REF.device, **ONE),
     "t must be a contiguous fp32 \\[9, 4\\] on cpu, got .*meta"),
]


@pytest.mark.parametrize("t,kw,message", [c[1:] for c in TENSOR_CASES], ids=[c[0] for c in TENSOR_CASES])
def test_tensor_check_refuses(t, kw, message):
    from hipops import _args as A
    with pytest.raises(ValueError, match=f"^some_op: {message}"):
        A.tensor("some_op", "t", t, **kw)
    if t is not None:                                    # `optional` lets None through, and nothing else
        with pytest.raises(ValueError, match=f"^some_op: {message}"):
            A.tensor("some_op", "t", t, optional=True, **kw)


def test_tensor_check_passes():
    from hipops import _args as A
    strided = _t(9, 8)[:, ::2]
    everything = dict(rank=2, numel=36, shape=(9, 4), contiguous=True, device=REF.device)
    for oneshot in (False, True):
        assert A.tensor("some_op", "t", None, optional=True, oneshot=oneshot, **everything) is None
        assert A.tensor("some_op", "t", _t(9, 4), oneshot=oneshot, **everything) is None
        assert A.tensor("some_op", "t", _t(9, 4, dtype=I32), I32, "int32", oneshot=oneshot, **everything) is None
        assert A.tensor("some_op", "t", strided, shape=(9, 4), oneshot=oneshot) is None            # contiguity only where asked for
        assert A.tensor("some_op", "t", _t(0, 4), nonempty=False, rank=2, oneshot=oneshot) is None
        assert A.tensor("some_op", "t", _t(3), shape=torch.Size([3]), oneshot=oneshot) is None      # a shape of any sequence type
    assert A.tensor("some_op", "t", _t(0, 4), shape=(0, 4), oneshot=True) is None                   # an exact shape decides emptiness


WHOLE_BAD = [
    (True, {}, "n must be a whole number, got True"),
    (3.0, {}, "n must be a whole number, got 3.0"),
    ("3", {}, "n must be a whole number, got '3'"),
    (None, dict(lo=1), "n must be a whole number >= 1, got None"),
    (0, dict(lo=1), "n must be a whole number >= 1, got 0"),
    (17, dict(lo=2, hi=16), "n must be a whole number in 2 .. 16, got 17"),
    (1, dict(lo=2, hi=16), "n must be a whole number in 2 .. 16, got 1"),
    (False, dict(lo=0, hi=16), "n must be a whole number in 0 .. 16, got False"),
    (9, dict(hi=8), "n must be a whole number <= 8, got 9"),
    (np.int64(0), dict(lo=1), "n must be a whole number >= 1, got "),
    (np.float32(3), dict(lo=1), "n must be a whole number >= 1, got "),
    (0, dict(lo=1, want="a positive whole number of output pixels"), "n must be a positive whole number of output pixels, got 0"),
]


@pytest.mark.parametrize("v,kw,message", WHOLE_BAD, ids=[f"{c[0]!r} {c[1]}" for c in WHOLE_BAD])
def test_whole_number_check_refuses(v, kw, message):
    from hipops import _args as A
    with pytest.raises(ValueError, match=f"^some_op: {message}"):
        A.whole("some_op", "n", v, **kw)


def test_whole_number_check_returns_an_int():
    from hipops import _args as A
    for v, kw in ((3, {}), (np.int64(3), dict(lo=1)), (np.int32(3), dict(lo=3, hi=3)), (np.uint8(3), dict(hi=3)), (3, dict(lo=2, hi=16))):
        got = A.whole("some_op", "n", v, **kw)
        assert got == 3 and type(got) is int, (v, kw)
    assert A.whole("some_op", "n", -5) == -5 and A.whole("some_op", "n", 2 ** 40, lo=0) == 2 ** 40


def test_workspace_cache_rules():
    from hipops import ops
    a = ops._workspace("test_op_a", "cpu", 10, torch.float32, 7, 3)
    assert a.numel() >= 10 and a.dtype == F32 and a.device.type == "cpu"
    assert ops._workspace("test_op_a", "cpu", 10, torch.float32, 7, 3) is a                  # the same op, device and key: the same tensor
    assert ops._workspace("test_op_a", torch.device("cpu"), 4, torch.float32, 7, 3) is a     # however the device is spelt; a smaller need
    grown = ops._workspace("test_op_a", "cpu", 25, torch.float32, 7, 3)                       # a larger need replaces it
    assert grown is not a and grown.numel() >= 25
    assert ops._workspace("test_op_a", "cpu", 10, torch.float32, 7, 3) is grown              # a smaller need afterwards: the grown one
    other_key = ops._workspace("test_op_a", "cpu", 10, torch.float32, 7, 4)
    no_key = ops._workspace("test_op_a", "cpu", 10)
    b = ops._workspace("test_op_b", "cpu", 10, torch.float32, 7, 3)                           # two ops with equal keys do not share
    assert len({id(t) for t in (grown, other_key, no_key, b)}) == 4
    d = ops._workspace("test_op_b", "cpu", 6, torch.float64)
    assert d.dtype == F64 and d.numel() >= 6
    assert {id(t) for t in ops._workspaces("test_op_a")} == {id(grown), id(other_key), id(no_key)}
    assert {id(t) for t in ops._workspaces("test_op_b")} == {id(b), id(d)}
    assert ops._workspaces("test_op_c") == []
    for ws in ops._workspaces("test_op_b"):                                                   # what the GPU tests do: poison the live ones
        ws.fill_(float("nan"))
    assert bool(torch.isnan(b).all()) and bool(torch.isnan(d).all()) and not bool(torch.isnan(grown.fill_(0.0)).any())


def test_float64_pointers_go_through_the_pointer_check():
    """`_ptr64` is `_ptr` for float64: None passes, a CPU or non-float64 tensor is refused with `_ptr`'s RuntimeError"""
    from hipops import ops
    assert ops._ptr64(None) is None
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops._ptr64(_t(3, dtype=F64))
    with pytest.raises(RuntimeError, match="needs contiguous float64 tensors, got torch.float32"):
        ops._ptr64(_FakeCuda(F32, True))
    with pytest.raises(RuntimeError, match="needs contiguous float64 tensors, got torch.float64 contiguous=False"):
        ops._ptr64(_FakeCuda(F64, False))
    with pytest.raises(RuntimeError, match="needs contiguous fp32/int32 tensors, got torch.float64"):
        ops._ptr(_FakeCuda(F64, True))
    assert ops._ptr64(_FakeCuda(F64, True)).value == 4096 and ops._ptr(_FakeCuda(I32, True)).value == 4096


class _FakeCuda:
    """what `_ptr` reads of a tensor, claiming to be on the GPU (the address is never dereferenced)"""
    is_cuda, device = True, "cuda:0"

    def __init__(self, dtype, contiguous):
        self.dtype, self._c = dtype, contiguous

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return 4096
