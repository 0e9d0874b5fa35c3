"""Argument checks of the host wrappers (hipops.ops).  Pure functions of their arguments: nothing here touches a device or the library,
and every refusal is a ValueError that begins with `what`, the wrapper's name.  The wrappers call them before they take a pointer or
make a library call: the kernels index every operand by the geometry of one of them, so an operand of another dtype, size or device is
an out-of-bounds device access."""
import numbers

import torch


def _want(word, rank, layout, numel, shape, nonempty, contiguous):
    """the whole requirement of a one-shot message: `a contiguous fp32 [9, 4]`, `one fp32 element`, `a non-empty int32 tensor of rank 2`"""
    c = "contiguous " if contiguous else ""
    if shape is not None:
        return f"{'a ' if c else ''}{c}{word} {list(shape)}"
    if numel is not None:
        return f"{'one' if numel == 1 else numel} {c}{word} element{'' if numel == 1 else 's'}"
    return f"a {'non-empty ' if nonempty else ''}{c}{word} tensor" + ("" if rank is None else f" {layout or f'of rank {rank}'}")


def tensor(what, name, t, dtype=torch.float32, word="fp32", *, rank=None, layout=None, numel=None, shape=None, nonempty=True,
           contiguous=False, device=None, other="the other operands", optional=False, oneshot=False):
    """ValueError unless `t` is a tensor of `dtype` -- of `rank`, not empty, contiguous, on `device`, of `numel` elements and of `shape`,
    each where asked for.  `optional`: None passes.  `word` is how the messages call the dtype, `layout` how they state the rank (`of rank
    2 [rows, inner]`), `other` whose device `device` is.

    Two wordings.  Stepwise (inputs): the first condition that fails, in the order above, gives the message -- `x must be an fp32 tensor,
    got ...`, `... must be of rank 2, got rank 3`, `... is empty`, `... must be contiguous`, `w_q is on meta, w_ref on cpu`, `... holds 5
    elements, expected 6`, `... has shape (4,), expected (3,)`.  `oneshot` (outputs, optional buffers): one message states the whole
    requirement, `out must be a contiguous fp32 [9, 4] on cuda:0, got (dtype, shape, device)` (the type's name for a non-tensor); an
    exact shape or count says whether the tensor is empty, so `nonempty` counts only without them."""
    if t is None and optional:
        return
    shape = None if shape is None else tuple(shape)
    is_t = torch.is_tensor(t)
    got = (t.dtype, tuple(t.shape), t.device) if is_t else type(t).__name__
    if oneshot:
        nonempty = nonempty and shape is None and numel is None
        if not (is_t and t.dtype == dtype and (rank is None or t.dim() == rank) and not (nonempty and t.numel() == 0)
                and (t.is_contiguous() or not contiguous) and (device is None or t.device == device)
                and (numel is None or t.numel() == numel) and (shape is None or tuple(t.shape) == shape)):
            where = "" if device is None else f" on {device}"
            raise ValueError(f"{what}: {name} must be {_want(word, rank, layout, numel, shape, nonempty, contiguous)}{where}, got {got}")
        return
    if not is_t or t.dtype != dtype:
        article = "a" if word.startswith("float") else "an"         # an fp32, an int32, a float64
        raise ValueError(f"{what}: {name} must be {article} {word} tensor, got {got[0] if is_t else got}")
    if rank is not None and t.dim() != rank:
        raise ValueError(f"{what}: {name} must be {layout or f'of rank {rank}'}, got rank {t.dim()}")
    if nonempty and t.numel() == 0:
        raise ValueError(f"{what}: {name} is empty: {got[1]}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")
    if device is not None and t.device != device:
        raise ValueError(f"{what}: {name} is on {t.device}, {other} on {device}")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{what}: {name} holds {t.numel()} elements, expected {numel}")
    if shape is not None and tuple(t.shape) != shape:
        raise ValueError(f"{what}: {name} has shape {got[1]}, expected {shape}")


def whole(what, name, v, lo=None, hi=None, want=None):
    """`v` as an int: a whole number (Python's or numpy's; not a bool) with lo <= v <= hi where they are given, else ValueError.  `want`:
    the requirement in the caller's words, in place of `a whole number >= lo` / `a whole number in lo .. hi`."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or (lo is not None and v < lo) or (hi is not None and v > hi):
        if want is None:
            want = "a whole number" + ("" if lo is None and hi is None else f" <= {hi}" if lo is None else f" >= {lo}" if hi is None
                                       else f" in {lo} .. {hi}")
        raise ValueError(f"{what}: {name} must be {want}, got {v!r}")
    return int(v)
