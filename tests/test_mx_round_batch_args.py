"""CPU checks of the batched learned-rounding step on the MX grids: include/rdo_ptq_mxroundbatch.h against `EXPORTS_MXROUNDBATCH` and the
built library, the refusals of the C entry (RDO_EINVAL without touching a device) and of `ops.mx_round_step_batch` on CPU tensors before a
pointer is taken."""
import ctypes as C
import os
import re

import pytest
import torch

from test_mx_conv_args import RDO_EINVAL, ROOT, no_library  # noqa: F401  (no_library is a fixture)

NAME = "rdo_mx_round_step_batch"


def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxroundbatch.h")).read()
    assert set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M)) == set(L.EXPORTS_MXROUNDBATCH) == {NAME}
    assert set(re.findall(r"\b(rdo_[a-z0-9_]+)\s*\(", hdr)) == {NAME} and '#include "rdo_ptq_mxround.h"' in hdr
    fn = L.lib().rdo_mx_round_step_batch
    assert fn.restype is C.c_int and len(fn.argtypes) == 11 and fn.argtypes[2] is C.c_float
    tables = [v for k, v in vars(L).items() if k.startswith("EXPORTS") and k != "EXPORTS_MXROUNDBATCH"]
    assert len(tables) >= 19 and not any(NAME in t for t in tables) and len(L.EXPORTS) == 124 and len(L.EXPORTS_MXROUND) == 4


def _item(L, ptr, **kw):
    geom = dict(numel=32 * 64, rows=32, kh=1, kw=1, cin=64)
    geom.update({k: kw.pop(k) for k in list(kw) if k in geom})
    f = dict(lo="p", gap="p", slabs="p", nsplit=2, alpha="p", adam_m="p", adam_v="p", wq="p", wd="p", wq_planes="p", wd_planes="p",
             wq_plane_scale=0.0, wd_plane_scale=4.0, lin_fwd_planes="p", lin_bwd_planes="p", lin_plane_scale=2.0)
    f.update(kw)
    it = L.MxRoundStepItem()
    it.d = L.AdaDesc(geom["numel"], geom["rows"], 16, 0, 0.0, 0.0, geom["kh"], geom["kw"], geom["cin"])
    for k, v in f.items():
        setattr(it, k, ptr[v].value if isinstance(v, str) else v)
    return it


BAD_ITEMS = [dict(numel=30 * 64 + 2, rows=1, cin=30 * 64 + 2), dict(numel=0), dict(rows=0), dict(cin=63), dict(lo=None), dict(gap=None),
             dict(slabs=None), dict(alpha=None), dict(adam_m=None), dict(adam_v=None), dict(wq=None), dict(nsplit=0), dict(lo="by4"), dict(gap="by4"),
             dict(slabs="by4"), dict(alpha="by4"), dict(adam_m="by4"), dict(adam_v="by4"), dict(wq="by4"), dict(wd="by4"), dict(wq_planes="odd"),
             dict(wd_planes="by4"), dict(lin_fwd_planes="odd"), dict(lin_bwd_planes="by4"), dict(wq_plane_scale=-1.0),
             dict(wd_plane_scale=float("inf")), dict(wd=None), dict(cin=0, kh=0, kw=0), dict(lin_plane_scale=0.0),
             dict(numel=48 * 64, rows=48), dict(numel=32 * 80, cin=80), dict(numel=32 * 9 * 64, kh=3, kw=3)]
BAD_CALLS = [dict(items=None), dict(n=0), dict(n=9), dict(sched=None), dict(it=None), dict(adv="p", shadow="q"), dict(shadow="p"), dict(sched="odd"),
             dict(it="odd"), dict(log="odd"), dict(adv="odd"), dict(shadow="odd"), dict(gather=dict(cache_q=None)), dict(gather=dict(B=0)),
             dict(gather=dict(per_image=6)), dict(gather=dict(C=24)), dict(gather=dict(out=None, out_planes=None)), dict(gather=dict(prob=1.5)),
             dict(gather=dict(n_iters=0)), dict(gather=dict(out="by4"))]


@pytest.mark.parametrize("item,call", [(i, {}) for i in BAD_ITEMS] + [({}, c) for c in BAD_CALLS])
def test_c_entry_refuses_bad_arguments_without_a_device(item, call):
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    base = (C.addressof(buf) + 15) & ~15
    ptr = {"p": C.c_void_p(base), "q": C.c_void_p(base + 16), "odd": C.c_void_p(base + 2), "by4": C.c_void_p(base + 4), None: C.c_void_p(None)}
    arr = (L.MxRoundStepItem * 2)(_item(L, ptr), _item(L, ptr, **item))
    a = dict(dict(items=arr, n=2, sched="p", it="p", log="p", adv=None, shadow=None, gather=None), **call)
    g = None
    if a["gather"] is not None:
        f = dict(dict(cache_q="p", cache_fp="p", idx_table="p", n_iters=4, B=2, batch_offset=0, per_image=16 * 32, C=32, prob=0.5, seed=1, out="p",
                      out_planes="p", out_scale=1.0, overflow_flag=None), **a["gather"])
        g = L.GatherDesc()
        for k, v in f.items():
            setattr(g, k, ptr[v].value if isinstance(v, str) or v is None else v)
        g = C.byref(g)
    word = lambda v: ptr[v] if isinstance(v, str) or v is None else v
    assert h.rdo_mx_round_step_batch(a["items"], a["n"], 1.0, 0.01, word(a["sched"]), word(a["it"]), word(a["log"]), word(a["adv"]),
                                     word(a["shadow"]), g, None) == RDO_EINVAL
    assert h.rdo_last_error().startswith(NAME.encode()), h.rdo_last_error()


def _good(ops, **kw):
    from hipops import _lib as L
    z = lambda *s, **k: torch.zeros(*s, **k)
    w = z(32, 1, 1, 64)
    planes = lambda: ops.H2(z(2, 32, 1, 1, 64, dtype=torch.int16), 4.0)
    it = dict(d=L.AdaDesc(w.numel(), 32, 16, 0, 0.0, 0.0, 1, 1, 64), lo=w, gap=w, slabs=z(2, 32, 1, 1, 64), alpha=w, m=w, v=w, wq=w, wd=z(64, 1, 1, 32),
              wq_planes=z(3, 32, 1, 1, 64, dtype=torch.int16), wd_planes=planes(), lin_fwd=planes(), lin_bwd=planes())
    it.update(kw)
    return it


@pytest.mark.parametrize("item,call,why", [
    ({}, dict(items=()), "items must be a list of 1 .. 8 dicts, got 0"), ({}, dict(items="x"), "items must be a list"),
    (dict(lo=torch.zeros(32, 64).double()), {}, "lo of item 1 must be an fp32 tensor"), (dict(gap=torch.zeros(32, 63)), {}, "gap of item 1 holds 2016 elements"),
    (dict(v=None), {}, "v of item 1 must be an fp32 tensor"), (dict(alpha=torch.zeros(64, 64)[:, ::2]), {}, "alpha of item 1 must be contiguous"),
    (dict(lo=torch.zeros(2, 3), gap=torch.zeros(6), alpha=torch.zeros(6), m=torch.zeros(6), v=torch.zeros(6), wq=torch.zeros(6)), {}, "no multiple of 4"),
    (dict(d=None), {}, "item 1: d must be an `ada_desc`"), (dict(wd=torch.zeros(5)), {}, "wd of item 1 must be 2048 contiguous fp32 elements"),
    (dict(slabs=torch.zeros(2, 2047)), {}, "slabs of item 1 must be \\[nsplit, ...\\] with 2048 elements a slab"),
    (dict(wq_planes=torch.zeros(2, 2048, dtype=torch.int16)), {}, "wq_planes of item 1 must be 6144 contiguous int16 elements"),
    (dict(wd_planes=torch.zeros(3, 2048)), {}, "wd_planes of item 1 must be 6144 contiguous int16 elements"),
    (dict(wd=None, lin_fwd=None, lin_bwd=None), {}, "wd_planes of item 1 needs wd"), (dict(lin_fwd=torch.zeros(2, 2048, dtype=torch.int16)), {}, "lin_fwd of item 1 must be an H2"),
    (dict(lin_bwd="scale"), {}, "lin_fwd and lin_bwd have the scales 4.0 and 8.0"), (dict(d="3x3"), {}, "Linear planes need a 1 x 1 layout"),
    (dict(d="flat"), {}, "need a descriptor with a conv layout"),
    ({}, dict(sched=torch.zeros(5, 3)), "sched must be \\[iters, 4\\]"), ({}, dict(iter_ptr=torch.zeros(1)), "iter_ptr must be an int32 tensor"),
    ({}, dict(round_log=torch.zeros(4, 32)), "round_log must be a contiguous fp32 \\[5, 32\\]"),
    ({}, dict(advance_iter="word", iter_shadow="word"), "advance_iter and iter_shadow are alternatives"),
    ({}, dict(iter_shadow="same"), "iter_shadow must be another word than iter_ptr"), ({}, dict(advance_iter=torch.zeros(2, dtype=torch.int32)), "advance_iter must be one int32 element"),
    ({}, dict(gather=dict(B=2)), "gather must be a dict with cache_q"), ({}, dict(gather="fp"), "gather idx_table must be \\[iters, 2\\]"),
    ({}, {}, "lo of item 0 is on cpu; there is no CPU path")])
def test_wrapper_refuses_malformed_arguments(no_library, item, call, why):
    from hipops import _lib as L
    ops = no_library
    item, call = dict(item), dict(call)
    if item.get("lin_bwd") == "scale":
        item["lin_bwd"] = ops.H2(torch.zeros(2, 2048, dtype=torch.int16), 8.0)
    if isinstance(item.get("d"), str):
        item["d"] = {"3x3": L.AdaDesc(2048, 32, 16, 0, 0.0, 0.0, 2, 1, 32), "flat": L.AdaDesc(2048, 32, 16, 0, 0.0, 0.0, 0, 0, 0)}[item["d"]]
    it = torch.zeros(1, dtype=torch.int32)
    k = dict(items=[_good(ops), _good(ops, **item)], grad_scale=1.0, round_weight=0.01, sched=torch.zeros(5, 4), iter_ptr=it, round_log=torch.zeros(5, 32))
    k.update({n: {"word": torch.zeros(1, dtype=torch.int32), "same": it}.get(v, v) if isinstance(v, str) and n != "items" else v for n, v in call.items()})
    if k.get("gather") == "fp":
        k["gather"] = dict(cache_q=torch.zeros(4, 8, 8, 16), cache_fp=torch.zeros(4, 8, 8, 16), idx_table=torch.zeros(5, 3, dtype=torch.int32), B=2,
                           prob=0.5, seed=3, out=torch.zeros(2, 8, 8, 16))
    with pytest.raises(ValueError, match=f"mx_round_step_batch: .*{why}"):
        ops.mx_round_step_batch(**k)
