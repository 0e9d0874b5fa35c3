"""CPU checks of the taped activation-quantised window attention: include/rdo_ptq_attnq.h declares exactly the entries of
`EXPORTS_ATTNQ` and no other table holds them, both C entries return RDO_EINVAL with a message that names them for every refusal
without touching a device, `ops.window_attention_pv_bwd` / `ops.window_attention_probs_bwd` refuse malformed operands with ValueError
before any pointer is taken, `args.act_learn_swin` is validated before any work, the default refusal of RSTB units names the switch, and
the float32 restatement of tests/attn_tape_reference.py stays finite against its own units (the ratio is printed: pytest -s)."""
import ctypes as C
import math
import os
import re
import types

import pytest
import torch

import attn_tape_reference as R
from oracle import attention_oracle as A

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rdo_window_attention_pv_bwd", "rdo_window_attention_probs_bwd"}


def test_header_declares_and_library_exports_the_entries():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_attnq.h")).read()
    declared = set(re.findall(r"^int(?:64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == NAMES == set(L.EXPORTS_ATTNQ)
    assert '#include "rdo_ptq_hip.h"' in hdr
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_BIAS, L.EXPORTS_BITS, L.EXPORTS_PACK, L.EXPORTS_SUBPEL, L.EXPORTS_ACTBITS)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    for path in os.listdir(os.path.join(ROOT, "include")):
        if path != "rdo_ptq_attnq.h":
            assert not NAMES & set(re.findall(r"\b(rdo_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", path)).read())), path
    assert len(L.EXPORTS) == 124


# ----------------------------------------------------------------------------- the C entries
GEOM = (1, 4, 4, 8, 2, 2, 1)                       # 16 pixels, 4 windows of 4 tokens, 2 heads of 4 channels


def _host_operands():
    """host buffers of the operand sizes of GEOM (never dereferenced: RDO_REQUIRE runs before any launch), far enough apart not to overlap"""
    g = A.Geom(*GEOM)
    pixels = g.B * g.H * g.W
    sizes = {"qkv": pixels * 3 * g.C, "probs": g.windows * g.N * g.N * g.heads, "dout": pixels * g.C}
    bufs = {k: (C.c_float * n)() for k, n in (("qkv", sizes["qkv"]), ("probs", sizes["probs"]), ("dout", sizes["dout"]),
                                              ("dprobs", sizes["probs"]), ("dqkv", sizes["qkv"]))}
    return bufs, {k: C.addressof(b) for k, b in bufs.items()}


def _desc(*geom, scale=0.5):
    from hipops import _lib as L
    return L.AttnDesc(*geom, scale)


BAD_GEOMETRIES = [(0, 4, 4, 8, 2, 2, 1), (1, 0, 4, 8, 2, 2, 1), (1, 4, -4, 8, 2, 2, 1), (1, 4, 4, 0, 2, 2, 1), (1, 4, 4, 8, 0, 2, 1),
                  (1, 4, 4, 8, 2, 0, 0), (1, 4, 4, 8, 3, 2, 1), (1, 4, 6, 8, 2, 4, 1), (1, 6, 4, 8, 2, 4, 1), (1, 18, 18, 8, 2, 9, 0),
                  (1, 4, 4, 8, 2, 2, 2), (1, 4, 4, 8, 2, 2, -1), (1, 4, 4, 130, 2, 2, 1)]


def test_c_entries_refuse_bad_arguments_without_a_device():
    from hipops import _lib as L
    h = L.lib()
    bufs, at = _host_operands()
    ok = _desc(*GEOM)

    def pv(d=ok, **kw):
        a = dict(qkv=at["qkv"], probs_q=at["probs"], dout=at["dout"], dprobs=at["dprobs"], dqkv=at["dqkv"])
        a.update(kw)
        return h.rdo_window_attention_pv_bwd(None if d is None else C.byref(d), a["qkv"], a["probs_q"], a["dout"], a["dprobs"], a["dqkv"], None)

    def pb(d=ok, **kw):
        a = dict(qkv=at["qkv"], probs=at["probs"], dprobs=at["dprobs"], dqkv=at["dqkv"])
        a.update(kw)
        return h.rdo_window_attention_probs_bwd(None if d is None else C.byref(d), a["qkv"], a["probs"], a["dprobs"], a["dqkv"], None)

    def refused(call, name, what, **kw):
        assert call(**kw) == RDO_EINVAL, (name, kw)
        msg = h.rdo_last_error().decode()
        assert name in msg and what in msg, (kw, msg)

    for call, name, operands in ((pv, "rdo_window_attention_pv_bwd", ("qkv", "probs_q", "dout", "dprobs", "dqkv")),
                                 (pb, "rdo_window_attention_probs_bwd", ("qkv", "probs", "dprobs", "dqkv"))):
        for op in operands:
            refused(call, name, "null pointer", **{op: None})
        refused(call, name, "null descriptor", d=None)
        for geom in BAD_GEOMETRIES:
            refused(call, name, "", d=_desc(*geom))
        # dqkv aliasing qkv: the same address, and a partial overlap from either side
        refused(call, name, "overlaps", dqkv=at["qkv"])
        refused(call, name, "overlaps", dqkv=at["qkv"] + 4)
        refused(call, name, "overlaps", dqkv=at["qkv"] - 4 * 300)              # (qkv holds 384 floats: the last 84 of dqkv lie inside it)
    # the other outputs and inputs of a call
    refused(pv, "rdo_window_attention_pv_bwd", "overlap", dprobs=at["probs"])
    refused(pv, "rdo_window_attention_pv_bwd", "overlap", dprobs=at["dout"] + 8)
    refused(pv, "rdo_window_attention_pv_bwd", "overlap", dprobs=at["dqkv"])
    refused(pv, "rdo_window_attention_pv_bwd", "overlap", dqkv=at["dout"])
    refused(pb, "rdo_window_attention_probs_bwd", "overlaps", dqkv=at["probs"])
    refused(pb, "rdo_window_attention_probs_bwd", "overlaps", dqkv=at["dprobs"])
    del bufs


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


def test_the_wrappers_refuse_malformed_operands(no_library):
    ops = no_library
    g = A.Geom(*GEOM)
    d = ops.attn_desc(*GEOM)
    qkv, dout = torch.zeros(g.B, g.H, g.W, 3 * g.C), torch.zeros(g.B, g.H, g.W, g.C)
    probs = torch.zeros(g.windows, g.N, g.N, g.heads)
    meta = torch.zeros(probs.shape, device="meta")
    pv_cases = [
        ((GEOM, qkv, probs, dout), {}, "expected an attn_desc"),
        ((ops.attn_desc(1, 4, 4, 8, 3, 2, 1), qkv, probs, dout), {}, "not divisible by heads"),
        ((ops.attn_desc(1, 18, 18, 8, 2, 9, 0), qkv, probs, dout), {}, "more than 64 tokens"),
        ((ops.attn_desc(1, 4, 4, 8, 2, 2, 2), qkv, probs, dout), {}, "shift=2"),
        ((d, qkv.double(), probs, dout), {}, "qkv must be an fp32 tensor"),
        ((d, None, probs, dout), {}, "qkv must be an fp32 tensor"),
        ((d, qkv[..., :-1], probs, dout), {}, "qkv holds"),
        ((d, qkv, probs[:-1], dout), {}, "probs_q holds"),
        ((d, qkv, probs.to(torch.float16), dout), {}, "probs_q must be an fp32 tensor"),
        ((d, qkv, meta, dout), {}, "probs_q is on meta"),
        ((d, qkv, probs, qkv), {}, "dout holds"),
        ((d, qkv, probs, None), {}, "dout must be an fp32 tensor"),
        ((d, qkv, probs, dout), dict(dprobs=probs[1:]), "dprobs holds"),
        ((d, qkv, probs, dout), dict(dprobs=meta), "dprobs is on meta"),
        ((d, qkv, probs, dout), dict(dqkv=dout), "dqkv holds"),
        ((d, qkv, probs, dout), dict(dqkv=qkv.long()), "dqkv must be an fp32 tensor"),
    ]
    for args, kw, what in pv_cases:
        with pytest.raises(ValueError, match=f"window_attention_pv_bwd: .*{what}"):
            ops.window_attention_pv_bwd(*args, **kw)
    pb_cases = [
        ((GEOM, qkv, probs, probs), {}, "expected an attn_desc"),
        ((ops.attn_desc(1, 4, 6, 8, 2, 4, 1), qkv, probs, probs), {}, "not divisible by window"),
        ((ops.attn_desc(1, 4, 4, 130, 2, 2, 1), qkv, probs, probs), {}, "head dims above 64"),
        ((d, qkv.double(), probs, probs), {}, "qkv must be an fp32 tensor"),
        ((d, dout, probs, probs), {}, "qkv holds"),
        ((d, qkv, None, probs), {}, "probs must be an fp32 tensor"),
        ((d, qkv, probs[:, :1], probs), {}, "probs holds"),
        ((d, qkv, probs, probs[:-1]), {}, "dprobs holds"),
        ((d, qkv, probs, probs.double()), {}, "dprobs must be an fp32 tensor"),
        ((d, qkv, probs, meta), {}, "dprobs is on meta"),
        ((d, qkv, probs, probs), dict(dqkv=dout), "dqkv holds"),
        ((d, qkv, probs, probs), dict(dqkv=torch.zeros(qkv.shape, device="meta")), "dqkv is on meta"),
    ]
    for args, kw, what in pb_cases:
        with pytest.raises(ValueError, match=f"window_attention_probs_bwd: .*{what}"):
            ops.window_attention_probs_bwd(*args, **kw)
    # well-formed operands pass the checks: the pointer conversion is the next thing that happens
    with pytest.raises(AssertionError, match="reached the library"):
        ops.window_attention_pv_bwd(d, qkv, probs, dout)
    with pytest.raises(AssertionError, match="reached the library"):
        ops.window_attention_probs_bwd(d, qkv, probs, probs.clone())


# ----------------------------------------------------------------------------- the switch
@pytest.mark.parametrize("flag", [1, 0, "yes", None, 1.0])
def test_act_learn_swin_is_validated_before_any_work(flag):
    from quantization import block_reconstruction, layer_reconstruction
    from quantization.recon import _pass_options, learn_act_ranges
    with pytest.raises(ValueError, match="act_learn_swin"):
        _pass_options(types.SimpleNamespace(act_mode="static", act_range="learned", act_learn_swin=flag))
    for recon in (layer_reconstruction, block_reconstruction):            # refused before the model, the unit or a device is looked at
        with pytest.raises(ValueError, match="act_learn_swin"):
            recon(None, None, "0", torch.zeros(2, 3, 64, 64), batch_size=2, iters=1, act_quant=True,
                  args=types.SimpleNamespace(task_loss=2.0, act_mode="static", act_range="learned", act_learn_swin=flag))
    with pytest.raises(ValueError, match="swin must be True or False"):
        learn_act_ranges(torch.nn.Identity(), torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4), 5, 1e-3, swin=flag)


def test_the_switch_defaults_to_off_and_is_read_as_a_bool():
    from quantization.recon import _pass_options
    assert _pass_options(None).act_learn_swin is False and _pass_options(types.SimpleNamespace()).act_learn_swin is False
    assert _pass_options(types.SimpleNamespace(act_learn_swin=True)).act_learn_swin is True


def test_the_default_refusal_mentions_rstb_and_names_the_switch():
    import lic
    from helpers import AQ, WQ
    from quantization import block_reconstruction
    from quantization.quant_block import QuantRSTB
    from quantization.recon import learn_act_ranges
    unit = QuantRSTB(lic.RSTB(dim=16, input_resolution=(8, 8), depth=2, num_heads=2, window_size=4, mlp_ratio=2.0), WQ, AQ)
    x = torch.zeros(2, 16, 8, 8)
    for kw in ({}, dict(swin=False)):
        with pytest.raises(NotImplementedError, match="RSTB") as e:
            learn_act_ranges(unit, x, x, 5, 1e-3, 2, **kw)
        assert "swin=True" in str(e.value) and "act_learn_swin" in str(e.value)
    for extra in ({}, dict(act_learn_swin=False)):
        args = types.SimpleNamespace(task_loss=2.0, act_mode="static", act_range="learned", **extra)
        with pytest.raises(NotImplementedError, match="RSTB") as e:       # before the model (None) or a device is looked at
            block_reconstruction(None, unit, "g_a1", torch.zeros(2, 3, 64, 64), batch_size=2, iters=1, act_quant=True, args=args)
        assert "act_learn_swin" in str(e.value)
    assert not unit.use_act_quant and not unit.use_weight_quant


# ----------------------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("geom", [(2, 8, 8, 48, 4, 4, 2), (1, 8, 8, 32, 2, 8, 4), (2, 3, 2, 10, 2, 1, 0)])
def test_the_float32_restatement_meets_its_own_units_within_a_printed_ratio(geom):
    g = A.Geom(*geom)
    inp = R.inputs(g, seed=sum(geom))
    assert inp["probs"].dtype == inp["probs_q"].dtype == inp["dprobs"].dtype == torch.float32
    assert inp["probs"].shape == inp["probs_q"].shape == inp["dprobs"].shape == (g.windows, g.N, g.N, g.heads)
    pv, pb, ratios = R.restatement_ratios(g, inp)
    print(f"\n{geom}: restatement err / (unit + floor) " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(math.isfinite(v) for v in ratios.values()), ratios
