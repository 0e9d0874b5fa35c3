"""CPU checks of the AdaRound step entries' argument validation: every refusal below returns a nonzero code and leaves its reason in
`rdo_last_error` before a pointer is dereferenced, the overflow word looked up or anything launched (the pointers here are host
memory that is never touched)."""
import ctypes as C

import torch


def _item(L, p, numel=64, rows=4, cin=16, lin=False, lin_scale=8.0):
    it = L.AdaStepItem()
    it.d = L.AdaDesc(numel, rows, 256, 0, 0.0, 0.0, 1 if cin else 0, 1 if cin else 0, cin)
    for name in ("w", "delta", "zp", "slabs", "alpha", "adam_m", "adam_v", "wq", "dalpha"):
        setattr(it, name, p)
    it.nsplit = 2
    if lin:
        it.lin_fwd_planes, it.lin_bwd_planes, it.lin_plane_scale = p, p, lin_scale
    return it


def test_step_batch_refuses_bad_arguments_before_touching_the_device():
    from hipops import _lib as L
    h = L.lib()
    host = torch.zeros(4096, dtype=torch.float32)
    p = host.data_ptr()

    def batch(items, mode=0, advance=None, shadow=None, sched=p, it=p):
        arr = (L.AdaStepItem * max(len(items), 1))(*items)
        return h.rdo_adaround_step_batch(arr, len(items), mode, 1.0, 0.01, sched, it, p, advance, shadow, None)

    def refused(rc, *words):
        assert rc != 0
        msg = h.rdo_last_error()
        assert all(w in msg for w in words), msg

    refused(batch([_item(L, p) for _ in range(9)]), b"rdo_adaround_step_batch", b"n <= 8")
    refused(batch([]), b"rdo_adaround_step_batch")
    refused(batch([_item(L, p)], mode=3), b"mode 3")
    refused(batch([_item(L, p)], sched=None), b"schedule")
    refused(batch([_item(L, p), _item(L, p, numel=66, rows=2, cin=0)]), b"numel 66 of item 1", b"multiple of 4")
    refused(batch([_item(L, p, numel=48 * 32, rows=48, cin=32, lin=True)]), b"item 0", b"blocks of 32")          # rows % 32 != 0
    refused(batch([_item(L, p, numel=32 * 48, rows=32, cin=48, lin=True)]), b"blocks of 32")                     # inner % 32 != 0
    refused(batch([_item(L, p, numel=32 * 32, rows=32, cin=32, lin=True, lin_scale=0.0)]), b"positive scale")
    refused(batch([_item(L, p)], advance=p, shadow=p), b"advance_iter and iter_shadow are alternatives")
    refused(batch([_item(L, p)], mode=1, shadow=p, it=None), b"iter_shadow needs iter_ptr")
    no_slabs = _item(L, p)
    no_slabs.slabs = None
    refused(batch([no_slabs]), b"item 0 has no gradient slabs")

    g = L.GatherDesc()
    g.cache_q = g.cache_fp = g.idx_table = g.out = p
    g.n_iters, g.B, g.batch_offset, g.per_image, g.C, g.prob, g.seed = 3, 2, 0, 64, 16, 0.5, 1
    arr = (L.AdaStepItem * 1)(_item(L, p))
    refused(h.rdo_adaround_step_batch_gather(arr, 1, 1, 1.0, 0.01, p, p, p, None, C.byref(g), None),
            b"rdo_adaround_step_batch_gather", b"fused step or an apply")                                         # mode 1 has no gather
    refused(h.rdo_adaround_step_batch_gather(arr, 1, 0, 1.0, 0.01, p, p, p, None, None, None), b"null gather descriptor")


def test_single_tensor_entry_refuses_bad_descriptors():
    from hipops import _lib as L
    h = L.lib()
    host = torch.zeros(64, dtype=torch.float32)
    p = host.data_ptr()

    def step(d, nsplit=1, slabs=p):
        return h.rdo_adaround_step(C.byref(d), p, p, p, slabs, nsplit, 1.0, 0.01, p, p, p, p, p, p, None, p, None, None, 0.0, 0.0, None)
    for d in (L.AdaDesc(63, 4, 256, 0, 0.0, 0.0, 0, 0, 0),            # numel not divisible by rows
              L.AdaDesc(64, 4, 2, 0, 0.0, 0.0, 0, 0, 0),              # n_levels
              L.AdaDesc(64, 4, 256, 0, 0.0, 0.0, 1, 1, 8)):           # conv layout that does not multiply out
        assert step(d) != 0 and b"rdo_adaround_step" in h.rdo_last_error()
    ok = L.AdaDesc(64, 4, 256, 0, 0.0, 0.0, 1, 1, 16)
    assert step(ok, nsplit=0) != 0 and step(ok, slabs=None) != 0 and b"null pointer" in h.rdo_last_error()
