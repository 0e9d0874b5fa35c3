"""CPU checks of the static activation quantiser's surface: the calibration arguments are validated before any work is done, frozen
ranges travel with the pickled quantiser, an artefact of an earlier version stays dynamic, `activation_state` exports a hand-frozen
model, and the data-parallel range reduction gives every rank the same MIN / MAX / SUM (gloo, world size 2)."""
import io
import os
import pickle
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

NEW_ATTRS = ("act_mode", "act_phase", "act_range", "act_err")


def _frozen(channels=3, bits=8, sites=(0,)):
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(n_bits=8, channel_wise=True, scale_method="max", act=True, dynamic_bits=bits, act_mode="static")
    for s in sites:
        lo = -torch.arange(1, channels + 1, dtype=torch.float32) - s
        q.act_range[s] = torch.cat([lo, -lo * 2])
    q.act_phase = "frozen"
    return q


def test_symbols_are_exported_and_validate_arguments():
    from hipops import _lib as L
    h = L.lib()
    for name in ("rdo_actquant_static", "rdo_actquant_observe", "rdo_actquant_search", "rdo_actquant_search_workspace"):
        assert name in L.EXPORTS
    assert h.rdo_actquant_static(None, 4, 4, 8, None, None, None) != 0
    assert h.rdo_actquant_observe(None, 4, None, None) != 0
    assert h.rdo_actquant_search(None, 4, 4, 8, None, None, None, None) != 0
    assert h.rdo_actquant_search_workspace(0) == 0 and h.rdo_actquant_search_workspace(192) >= 192 * 10


@pytest.mark.parametrize("kw", [dict(act_mode="nope"), dict(act_mode="Static"), dict(act_range="mse"), dict(act_mode="static", act_range="l1")])
def test_unknown_act_mode_or_range_is_refused_before_any_work(kw):
    from quantization import block_reconstruction, layer_reconstruction
    from quantization.recon import _act_args
    with pytest.raises(ValueError, match="act_"):
        _act_args(types.SimpleNamespace(**kw))
    for recon in (layer_reconstruction, block_reconstruction):            # refused before the model, the unit or a device is looked at
        with pytest.raises(ValueError, match="act_"):
            recon(None, None, "0", torch.zeros(2, 3, 64, 64), batch_size=2, iters=1, act_quant=True,
                  args=types.SimpleNamespace(task_loss=2.0, **kw))


def test_act_arguments_default_to_dynamic_max():
    from quantization.recon import _act_args
    assert _act_args(None) == ("dynamic", "max")
    assert _act_args(types.SimpleNamespace()) == ("dynamic", "max")
    assert _act_args(types.SimpleNamespace(act_mode="static", act_range="l2")) == ("static", "l2")
    from quantization.quantizer import UniformAffineQuantizer
    with pytest.raises(ValueError):
        UniformAffineQuantizer(act=True, act_mode="nope")
    with pytest.raises(ValueError):
        UniformAffineQuantizer(act=True).set_act_mode("nope")
    assert UniformAffineQuantizer(act=True).act_mode == "dynamic"


def test_frozen_quantiser_pickles_with_its_ranges():
    q = _frozen(channels=5, bits=10, sites=(0, 1))
    q2 = pickle.loads(pickle.dumps(q))
    buf = io.BytesIO()
    torch.save(q, buf)
    buf.seek(0)
    q3 = torch.load(buf, weights_only=False)
    for r in (q2, q3):
        assert r.act_mode == "static" and r.act_frozen() and r.dynamic_bits == 10 and sorted(r.act_range) == [0, 1]
        for s in (0, 1):
            assert torch.equal(r.act_range[s], q.act_range[s])
    # .to() moves the ranges like delta / zero_point (here: a dtype-preserving no-op move that still goes through _apply)
    moved = q.to("cpu")
    assert torch.equal(moved.act_range[1], q.act_range[1])


def test_static_quantiser_raises_instead_of_falling_back():
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(act=True, act_mode="static")
    assert not q.act_frozen()
    with pytest.raises(RuntimeError, match="no frozen range"):
        q(torch.zeros(1, 3, 4, 4), True)
    f = _frozen(channels=3)
    with pytest.raises(ValueError, match="3 channels"):
        f(torch.zeros(1, 4, 2, 2), True)                       # 4-D: channel = dim 1
    with pytest.raises(ValueError, match="3 channels"):
        f(torch.zeros(2, 7, 5), True)                          # 3-D: channel = last dim
    with pytest.raises(RuntimeError, match="no frozen range"):
        f(torch.zeros(1, 3, 2, 2), True, site=1)               # a place of the block that calibration never met
    q.act_observe()
    q.act_freeze()                                             # observed nothing: stays without a range
    assert not q.act_frozen() and q.act_phase == "idle"
    with pytest.raises(RuntimeError):
        q.act_search()


def test_quantiser_of_an_earlier_version_behaves_dynamic(monkeypatch):
    import quantization.quantizer as Q
    q = Q.UniformAffineQuantizer(act=True, dynamic_bits=10)
    for name in NEW_ATTRS:
        del q.__dict__[name]
    q = pickle.loads(pickle.dumps(q))
    assert not any(hasattr(q, n) for n in NEW_ATTRS) and not q.act_frozen()
    seen = []
    monkeypatch.setattr(Q, "ActQuantizer", lambda x, bits=8: seen.append(bits) or x)
    x = torch.zeros(1, 3, 2, 2)
    assert q(x, True) is x and seen == [10]                    # the dynamic call, with the quantiser's own width
    q.set_act_mode("static")                                   # ... and it can still be switched over
    assert q.act_phase == "idle" and q.act_range == {}
    with pytest.raises(RuntimeError, match="no frozen range"):
        q(x, True)


def test_activation_state_of_a_hand_frozen_model():
    import lic
    from quantization import QuantModel
    from quantization.export import activation_state
    torch.manual_seed(0)
    qnn = QuantModel(model=lic.Cheng2020Anchor(N=8), weight_quant_params={"n_bits": 8, "channel_wise": True, "scale_method": "max"},
                     act_quant_params={"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}, is_cheng=True)
    assert activation_state(qnn) == {} and len(qnn.act_ranges()) == 0
    qnn.set_act_mode("static")
    names = dict(qnn.act_quantizers())
    assert all(q.act_mode == "static" and not q.act_frozen() for q in names.values())
    blk = next(n for n in names if n.count(".") == 3)          # a block-level quantiser, e.g. model.g_a.0.act_quantizer
    q = names[blk]
    q.act_range = {0: torch.tensor([-1.0, -2.0, 3.0, 4.0]), 1: torch.tensor([0.5, 0.25, 0.125, 7.0, 8.0, 9.0])}
    q.act_phase = "frozen"
    st = activation_state(qnn)
    assert list(st) == [blk, blk + "#1"]
    assert st[blk]["channels"] == 2 and st[blk]["n_bits"] == 8 and st[blk + "#1"]["channels"] == 3
    assert st[blk]["lo"].tolist() == [-1.0, -2.0] and st[blk]["hi"].tolist() == [3.0, 4.0]
    assert st[blk + "#1"]["lo"].tolist() == [0.5, 0.25, 0.125] and st[blk + "#1"]["hi"].tolist() == [7.0, 8.0, 9.0]
    assert all(v["lo"].device.type == "cpu" and v["lo"].dtype == torch.float32 for v in st.values())
    qnn2 = pickle.loads(pickle.dumps(qnn))
    st2 = activation_state(qnn2)
    assert list(st2) == list(st) and all(torch.equal(st2[k]["hi"], st[k]["hi"]) and torch.equal(st2[k]["lo"], st[k]["lo"]) for k in st)
    qnn.set_act_mode("dynamic")
    assert activation_state(qnn) == {}


def test_freeze_after_search_shrinks_to_the_best_candidate_inside_the_max_range():
    """the C x 10 arg-min and the shrinking are torch ops: checked here on hand-made error sums"""
    from quantization.quantizer import UniformAffineQuantizer
    q = UniformAffineQuantizer(act=True, act_mode="static")
    lo = torch.tensor([-2.0, -1.0, 0.5, -4.0])
    hi = torch.tensor([2.0, 3.0, 1.5, -1.0])
    q.act_range = {0: torch.cat([lo, hi])}
    q.act_phase = "search"
    err = torch.ones(4, 10)
    err[0, 0] = 0.5                      # best = the max range itself
    err[1, 3] = err[1, 7] = 0.25         # a tie: the first minimum
    err[2, 2] = 0.1                      # lo > 0: scaling would move lo below the observed minimum
    err[3, 9] = 0.1                      # hi < 0: scaling would move hi above the observed maximum
    q.act_err = {0: err}
    q.act_freeze()
    r = q.act_range[0]
    s3, s2, s9 = torch.tensor(1.0 - 0.05 * 3, dtype=torch.float32), torch.tensor(1.0 - 0.05 * 2, dtype=torch.float32), \
        torch.tensor(1.0 - 0.05 * 9, dtype=torch.float32)
    assert q.act_frozen() and q.act_err == {}
    assert r[:4].tolist() == [-2.0, float(-1.0 * s3), 0.5, float(-4.0 * s9)]
    assert r[4:].tolist() == [2.0, float(3.0 * s3), float(1.5 * s2), -1.0]
    assert bool((r[:4] >= lo).all()) and bool((r[4:] <= hi).all()) and bool((r[:4] <= r[4:]).all())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_rank(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "rdo-ptq_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from quantization import dp
    g = torch.Generator().manual_seed(100 + rank)
    ranges = [torch.randn(2 * c, generator=g) for c in (3, 8)]
    sums = [torch.rand(c, 10, generator=g) for c in (3, 8)]
    mine = [t.clone() for t in ranges + sums]
    dp.reduce_act_stats(ranges=ranges, sums=sums)
    out_q.put((rank, mine, [t.clone() for t in ranges + sums]))
    dist.barrier()
    dist.destroy_process_group()


def test_range_reduction_over_two_gloo_ranks():
    from quantization import dp
    r = torch.tensor([1.0, 2.0, 3.0, 4.0])
    dp.reduce_act_stats(ranges=[r], sums=[r])                  # no process group: nothing happens
    assert r.tolist() == [1.0, 2.0, 3.0, 4.0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_rank, args=(rk, 2, port, q)) for rk in range(2)]
    for p in procs:
        p.start()
    got = dict((rk, (mine, red)) for rk, mine, red in (q.get(timeout=240) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (m0, r0), (m1, r1) = got[0], got[1]
    for i, c in enumerate((3, 8)):
        want = torch.cat([torch.minimum(m0[i][:c], m1[i][:c]), torch.maximum(m0[i][c:], m1[i][c:])])
        assert torch.equal(r0[i], want) and torch.equal(r1[i], want)
        assert torch.equal(r0[2 + i], m0[2 + i] + m1[2 + i]) and torch.equal(r1[2 + i], r0[2 + i])
