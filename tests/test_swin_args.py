"""CPU checks of the transformer-path surface (csrc/swin.hip and the LayerNorm forward): the wrappers of hipops.ops refuse mismatched
operands with ValueError naming the wrapper before any pointer is taken or library call made (each such call would be an out-of-bounds
device access), and the C entry points return RDO_EINVAL with a message for null pointers and bad geometry without touching a device."""
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


def _t(*shape, dtype=torch.float32, device=None):
    return torch.zeros(*shape, dtype=dtype, device=device)


B, H, W, CH, HEADS, WS = 2, 8, 8, 16, 4, 4
N, WINDOWS = WS * WS, B * (H // WS) * (W // WS)


def _good():
    return dict(qkv=_t(B, H, W, 3 * CH), bias=_t(HEADS, N, N), probs=_t(WINDOWS, N, N, HEADS), out=_t(B, H, W, CH), dout=_t(B, H, W, CH),
                dqkv=_t(B, H, W, 3 * CH))


def test_attention_wrappers_refuse_mismatched_operands(no_library):
    ops = no_library
    d = ops.attn_desc(B, H, W, CH, HEADS, WS, 2)
    g = _good()
    meta = torch.zeros(HEADS, N, N, device="meta")
    fwd_bad = [
        dict(qkv=_t(B, H, W, 3 * CH - 1)), dict(qkv=_t(B - 1, H, W, 3 * CH)), dict(qkv=g["qkv"].double()), dict(qkv=_t(0)), dict(qkv=None),
        dict(bias=_t(HEADS - 1, N, N)), dict(bias=_t(HEADS, N, N - 1)), dict(bias=meta), dict(bias=g["bias"].half()), dict(bias=None),
        dict(probs=_t(WINDOWS - 1, N, N, HEADS)), dict(probs=_t(WINDOWS, N, N, HEADS + 1)), dict(probs=g["probs"].double()),
        dict(probs=torch.zeros(WINDOWS, N, N, HEADS, device="meta")),
        dict(out=_t(B, H, W, CH + 1)), dict(out=_t(B, H, W, 3 * CH)), dict(out=_t(0)), dict(out=g["out"].double()),
        dict(probs=None, compute_out=False),
    ]
    for kw in fwd_bad:
        a = dict(qkv=g["qkv"], bias=g["bias"], probs=g["probs"], out=g["out"])
        a.update(kw)
        with pytest.raises(ValueError, match="window_attention"):
            ops.window_attention(d, a.pop("qkv"), a.pop("bias"), **a)
    for kw in [dict(qkv=_t(B, H, W, 3 * CH + 1)), dict(qkv=g["qkv"].double()), dict(probs=_t(WINDOWS + 1, N, N, HEADS)), dict(probs=None),
               dict(probs=_t(0)), dict(out=_t(B, H, W, CH - 1)), dict(out=torch.zeros(B, H, W, CH, device="meta"))]:
        a = dict(qkv=g["qkv"], probs=g["probs"], out=g["out"])
        a.update(kw)
        with pytest.raises(ValueError, match="window_attention_pv"):
            ops.window_attention_pv(d, a["qkv"], a["probs"], a["out"])
    for kw in [dict(qkv=_t(B, H, W, CH)), dict(bias=_t(HEADS + 1, N, N)), dict(bias=None), dict(dout=_t(B, H, W, 3 * CH)), dict(dout=_t(B, H, W - 1, CH)),
               dict(dout=None), dict(dout=g["dout"].double()), dict(dqkv=_t(B, H, W, CH)), dict(dqkv=_t(B, H, W, 3 * CH, dtype=torch.float64)),
               dict(dqkv=torch.zeros(B, H, W, 3 * CH, device="meta"))]:
        a = dict(qkv=g["qkv"], bias=g["bias"], dout=g["dout"], dqkv=g["dqkv"])
        a.update(kw)
        with pytest.raises(ValueError, match="window_attention_bwd"):
            ops.window_attention_bwd(d, a["qkv"], a["bias"], a["dout"], a["dqkv"])


@pytest.mark.parametrize("geom", [(2, 8, 8, 18, 4, 4, 0),      # C % heads
                                  (2, 10, 8, 16, 4, 4, 0),     # H % window
                                  (2, 8, 10, 16, 4, 4, 0),     # W % window
                                  (1, 9, 9, 16, 4, 9, 0),      # 81 tokens
                                  (1, 8, 8, 130, 2, 4, 0),     # head dim 65
                                  (2, 8, 8, 16, 4, 4, 4),      # shift == window
                                  (2, 8, 8, 16, 4, 4, -1),
                                  (0, 8, 8, 16, 4, 4, 0), (2, 8, 8, 16, 0, 4, 0), (2, 8, 8, 16, 4, 0, 0)])
def test_attention_wrappers_refuse_bad_descriptors(no_library, geom):
    ops = no_library
    from hipops import _lib as L
    d = L.AttnDesc(*geom, 0.5)
    big = _t(1 << 16)
    with pytest.raises(ValueError, match="window_attention"):
        ops.window_attention(d, big, big)
    with pytest.raises(ValueError, match="window_attention_pv"):
        ops.window_attention_pv(d, big, big)
    with pytest.raises(ValueError, match="window_attention_bwd"):
        ops.window_attention_bwd(d, big, big, big)
    with pytest.raises(ValueError, match="window_attention"):
        ops.window_attention(None, big, big)


def test_layer_norm_wrappers_refuse_mismatched_operands(no_library):
    ops = no_library
    x, w, b, dy = _t(6, 16), _t(16), _t(16), _t(6, 16)
    for args, kw in [((x, _t(15), b), {}), ((x, w, _t(17)), {}), ((x, _t(16, 1), b), {}), ((x, w.double(), b), {}), ((x.double(), w, b), {}),
                     ((_t(0, 16), w, b), {}), ((None, w, b), {}), ((x, w, b), {"out": _t(6, 15)}), ((x, w, b), {"out": _t(16, 6)}),
                     ((x, w, b), {"out": torch.zeros(6, 16, device="meta")}), ((x, torch.zeros(16, device="meta"), b), {})]:
        with pytest.raises(ValueError, match="layer_norm"):
            ops.layer_norm(*args, **kw)
    for args, kw in [((x, x, _t(15), b), {}), ((x, x, w, _t(4, 4)), {}), ((x, _t(5, 16), w, b), {}), ((x, _t(96), w, b), {}),
                     ((x, x, w, b), {"sum_out": _t(6, 12)}), ((x, x, w, b), {"out": _t(7, 16)}), ((x, None, w, b), {"sum_out": _t(6, 16)}),
                     ((_t(6, 18), _t(6, 18), _t(18), _t(18)), {}),                    # C % 4
                     ((_t(2, 516), None, _t(516), _t(516)), {}),                      # C > 512
                     ((x, x.double(), w, b), {}), ((_t(0, 16), None, w, b), {})]:
        with pytest.raises(ValueError, match="add_layer_norm"):
            ops.add_layer_norm(*args, **kw)
    slabs = _t(8, 16)
    for name, vec in (("layer_norm_bwd", False), ("layer_norm_bwd_add", True)):
        fn = getattr(ops, name)
        bad = [((x, _t(15), dy), {"dx": _t(6, 16)}), ((x, w, _t(6, 15)), {"dx": _t(6, 16)}), ((x, w, _t(96)), {"dx": _t(6, 16)}),
               ((x, w, dy), {"dx": _t(5, 16)}), ((x, w, dy), {"dx": _t(6, 16), "dgamma_slabs": _t(8, 15)}),
               ((x, w, dy), {"dx": _t(6, 16), "dgamma_slabs": _t(8 * 16)}), ((x, w, dy), {"dx": _t(6, 16), "dgamma_slabs": _t(0, 16)}),
               ((x, w, dy), {"dgamma_slabs": slabs.double()}), ((x, w, dy), {}), ((x, w, None), {"dx": _t(6, 16)}),
               ((x, w, dy.double()), {"dx": _t(6, 16)}), ((_t(2, 516), _t(516), _t(2, 516)), {"dx": _t(2, 516)}),
               ((x, w, dy), {"dx": torch.zeros(6, 16, device="meta")})]
        for args, kw in bad:
            with pytest.raises(ValueError, match=name):
                fn(*args, **kw)
    e = _t(6, 16)
    for args, kw in [((x, w, dy, _t(6, 15)), {"dx": e}), ((x, w, dy, e, _t(5, 16)), {"dx": e}), ((x, w, dy, None, e), {"dx": e}),
                     ((x, w, dy, e), {"dgamma_slabs": slabs}), ((x, w, dy, e, e), {"dgamma_slabs": slabs}),
                     ((_t(6, 18), _t(18), _t(6, 18)), {"dx": _t(6, 18)})]:
        with pytest.raises(ValueError, match="layer_norm_bwd_add"):
            ops.layer_norm_bwd_add(*args, **kw)


def test_gelu_round_and_add3_refuse_unequal_counts(no_library):
    ops = no_library
    x = _t(100)
    for args, kw in [((x,), {"out": _t(99)}), ((x.double(),), {}), ((_t(0),), {}), ((None,), {}), ((x,), {"out": x.double()}),
                     ((x,), {"out": torch.zeros(100, device="meta")})]:
        with pytest.raises(ValueError, match="gelu"):
            ops.gelu(*args, **kw)
        with pytest.raises(ValueError, match="round_"):
            ops.round_(*args, **kw)
    for args in [(_t(99), x), (x, _t(101)), (x.double(), x), (x, x.half()), (None, x), (x, None), (x, x, _t(99)), (_t(0), _t(0))]:
        with pytest.raises(ValueError, match="gelu_bwd"):
            ops.gelu_bwd(*args)
    for args, kw in [((x, _t(99), x), {}), ((x, x, _t(104)), {}), ((x, x, x), {"out": _t(96)}), ((_t(102), _t(102), _t(102)), {}),
                     ((x, x.double(), x), {}), ((x, x, None), {}), ((_t(0), _t(0), _t(0)), {}), ((x, x, torch.zeros(100, device="meta")), {})]:
        with pytest.raises(ValueError, match="add3"):
            ops.add3(*args, **kw)


def test_well_formed_cpu_operands_reach_the_pointer_check():
    """the argument checks pass well-formed operands on: a CPU tensor is then refused by `_ptr` (no CPU path), still before any launch"""
    from hipops import ops
    d = ops.attn_desc(B, H, W, CH, HEADS, WS, 2)
    g = _good()
    x, w = _t(6, 16), _t(16)
    calls = [lambda: ops.window_attention(d, g["qkv"], g["bias"], probs=g["probs"]),
             lambda: ops.window_attention(d, g["qkv"], g["bias"], probs=g["probs"], compute_out=False),
             lambda: ops.window_attention_pv(d, g["qkv"], g["probs"]),
             lambda: ops.window_attention_bwd(d, g["qkv"], g["bias"], g["dout"], g["dqkv"]),
             lambda: ops.layer_norm(x, w, w), lambda: ops.layer_norm(x, None, None),
             lambda: ops.add_layer_norm(x, x, w, w, sum_out=_t(6, 16)), lambda: ops.add_layer_norm(x, None, None, None),
             lambda: ops.layer_norm_bwd(x, w, x, dx=_t(6, 16), dgamma_slabs=_t(3, 16)),
             lambda: ops.layer_norm_bwd_add(x, w, x, x, x, dx=_t(6, 16)), lambda: ops.layer_norm_bwd_add(x, None, x, dgamma_slabs=_t(1, 16)),
             lambda: ops.gelu(x), lambda: ops.gelu_bwd(x, x), lambda: ops.round_(x), lambda: ops.add3(x, x, x)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_c_abi_refuses_null_pointers_and_bad_geometry():
    """RDO_REQUIRE runs before any launch: the non-null arguments below are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))

    def refused(rc, name):
        assert rc == RDO_EINVAL, (name, rc)
        assert name.encode() in h.rdo_last_error(), (name, h.rdo_last_error())

    ok = L.AttnDesc(2, 8, 8, 16, 4, 4, 2, 0.5)
    bad = [L.AttnDesc(*g, 0.5) for g in [(2, 8, 8, 18, 4, 4, 0), (2, 10, 8, 16, 4, 4, 0), (2, 8, 10, 16, 4, 4, 0), (1, 9, 9, 16, 4, 9, 0),
                                         (1, 8, 8, 130, 2, 4, 0), (2, 8, 8, 16, 4, 4, 4), (2, 8, 8, 16, 4, 4, -1), (0, 8, 8, 16, 4, 4, 0),
                                         (2, 8, 8, 16, 0, 4, 0), (2, 8, 8, 16, 4, 0, 0)]]
    for d in bad:
        refused(h.rdo_window_attention_fwd(C.byref(d), p, p, p, p, None), "rdo_window_attention_fwd")
        refused(h.rdo_window_attention_pv(C.byref(d), p, p, p, None), "rdo_window_attention_pv")
        refused(h.rdo_window_attention_bwd(C.byref(d), p, p, p, p, None), "rdo_window_attention_bwd")
    refused(h.rdo_window_attention_fwd(None, p, p, p, p, None), "rdo_window_attention_fwd")
    for args in [(None, p, p, p), (p, None, p, p), (p, p, None, None)]:
        refused(h.rdo_window_attention_fwd(C.byref(ok), *args, None), "rdo_window_attention_fwd")
    for args in [(None, p, p), (p, None, p), (p, p, None)]:
        refused(h.rdo_window_attention_pv(C.byref(ok), *args, None), "rdo_window_attention_pv")
    for args in [(None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)]:
        refused(h.rdo_window_attention_bwd(C.byref(ok), *args, None), "rdo_window_attention_bwd")
    for args in [(None, p, p, 4, 16, 1e-5, p), (p, p, p, 4, 16, 1e-5, None), (p, p, p, 0, 16, 1e-5, p), (p, p, p, 4, 0, 1e-5, p)]:
        refused(h.rdo_layer_norm(*args, None), "rdo_layer_norm")
    for args in [(None, p, p, 4, 16, 1e-5, p, p, 1), (p, p, None, 4, 16, 1e-5, p, p, 1), (p, p, p, 0, 16, 1e-5, p, p, 1), (p, p, p, 4, 516, 1e-5, p, p, 1),
                 (p, p, p, 4, 16, 1e-5, None, None, 0), (p, p, p, 4, 16, 1e-5, p, p, 0)]:
        refused(h.rdo_layer_norm_bwd(*args, None), "rdo_layer_norm_bwd")
    odd = C.c_void_p(C.addressof(buf) + 4)
    for args in [(None, p, p, p, 4, 16, 1e-5, p, p), (p, p, p, p, 4, 16, 1e-5, p, None), (p, p, p, p, 4, 18, 1e-5, p, p), (p, p, p, p, 4, 516, 1e-5, p, p),
                 (p, None, p, p, 4, 16, 1e-5, p, p), (odd, p, p, p, 4, 16, 1e-5, p, p), (p, p, p, p, 4, 16, 1e-5, p, odd), (p, p, p, p, 0, 16, 1e-5, p, p)]:
        refused(h.rdo_add_layer_norm(*args, None), "rdo_add_layer_norm")
    for args in [(None, p, p, p, p, 4, 16, 1e-5, p, p, 1), (p, p, None, p, p, 4, 16, 1e-5, p, p, 1), (p, p, p, p, p, 4, 18, 1e-5, p, p, 1),
                 (p, p, p, None, p, 4, 16, 1e-5, p, p, 1), (p, p, p, p, None, 4, 16, 1e-5, None, p, 1), (p, p, p, None, None, 4, 16, 1e-5, None, None, 0),
                 (p, p, p, None, None, 4, 16, 1e-5, p, p, 0), (p, p, odd, None, None, 4, 16, 1e-5, p, p, 1)]:
        refused(h.rdo_layer_norm_bwd_add(*args, None), "rdo_layer_norm_bwd_add")
    for args in [(None, p, p, 8, p), (p, None, p, 8, p), (p, p, None, 8, p), (p, p, p, 8, None), (p, p, p, 0, p), (p, p, p, 6, p)]:
        refused(h.rdo_add3(*args, None), "rdo_add3")
    for name in ("rdo_gelu_fwd", "rdo_round"):
        for args in [(None, 8, p), (p, 8, None), (p, 0, p), (p, -1, p)]:
            refused(getattr(h, name)(*args, None), name)
    for args in [(None, p, 8, p), (p, None, 8, p), (p, p, 8, None), (p, p, 0, p)]:
        refused(h.rdo_gelu_bwd(*args, None), "rdo_gelu_bwd")
