"""The RD report on the GPU: `ops.neg_log2_channel_sums` (rdo_neg_log2_channel_sums of csrc/entropy.hip) against the float64
restatement and the derived bound of tests/rate_channels_reference.py in both storages, its exact cases and its NaN containment, its
consistency with the ordered scalar sum; `QuantModel.rd_report` against a hand-made run on a toy Cheng2020 and a toy Lu2022, the state
it leaves behind, its batch rule and two data-parallel ranks.

The bound is derived from the kernel's summation structure, nothing in it is measured (see the reference module).  Share of the bound
the kernel used on an MI355X, NCHW | channels-last:
    (1, 1, 1)        0.038 | 0.038          (2, 192, 256)    0.119 | 0.106
    (1, 3, 5)        0.021 | 0.022          (512, 7, 1)      0.030 | 0.030
    (2, 7, 16)       0.070 | 0.079          (1536, 320, 1)   0.119 | 0.119
    (3, 5, 63)       0.042 | 0.046          (3, 5, 1000)     0.046 | 0.087
"""
import math
import os
import socket
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import rate_channels_reference as R

pytestmark = pytest.mark.gpu

LMBDA = 0.0483


# ----------------------------------------------------------------------------- 1. the kernel against float64
def _both(lik):
    """[outer, C, inner] CPU values -> [(layout name, 4-D cuda tensor, (outer, C, inner) the wrapper passes on)]"""
    outer, C, inner = lik.shape
    nchw, cl = R.as_nchw_and_channels_last(lik)
    return [("nchw", nchw.cuda(), (outer, C, inner)), ("channels-last", cl.cuda(), (outer * inner, C, 1))]


def _poison_workspaces(ops):
    for ws in ops._workspaces("neg_log2_channel_sums"):
        ws.fill_(float("nan"))


@pytest.mark.parametrize("outer,C,inner", R.SHAPES)
def test_kernel_stays_within_the_derived_bound(outer, C, inner):
    from hipops import ops
    lik = R.make_lik(outer, C, inner, seed=100 + outer + C + inner)
    assert float(lik.min()) == float(np.float32(1e-9)) and (lik.numel() < 4 or float(lik.max()) == 1.0)       # the planted elements
    bits, tot = R.channel_bits(lik, outer, C, inner)
    got, bounds = {}, {}
    for name, x, geom in _both(lik):
        if name == "channels-last" and inner > 1 and C > 1:
            assert not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
        runs = []
        for _ in range(3):                                 # the workspace holds NaN before every launch
            _poison_workspaces(ops)
            runs.append(ops.neg_log2_channel_sums(x).clone())
        torch.cuda.synchronize()
        assert ops._workspaces("neg_log2_channel_sums")
        r = runs[0]
        assert r.shape == (C,) and r.dtype == torch.float32 and r.is_cuda
        assert torch.equal(runs[1], r) and torch.equal(runs[2], r) and bool(torch.isfinite(r).all())
        got[name], bounds[name] = r.double().cpu(), R.channel_bound(*geom, tot)
        share = float(((got[name] - bits).abs() / bounds[name]).max())
        print(f"neg_log2_channel_sums {(outer, C, inner)} {name}: share of the derived bound {share:.3f} (D = {R.depth(*geom)})")
        assert share <= 1.0
        out = torch.full((C,), float("nan"), device="cuda")            # `out` is overwritten
        assert ops.neg_log2_channel_sums(x, out=out) is out and torch.equal(out, r)
    assert bool(((got["nchw"] - got["channels-last"]).abs() <= bounds["nchw"] + bounds["channels-last"]).all())


def test_a_strided_tensor_is_made_contiguous():
    from hipops import ops
    lik = R.make_lik(4, 6, 10, seed=9).reshape(4, 6, 5, 2).cuda()
    view = lik[:, :, :, ::2]
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(ops.neg_log2_channel_sums(view), ops.neg_log2_channel_sums(view.contiguous()))


# ----------------------------------------------------------------------------- 2. exact cases
def _exact(outer, C, inner):
    """lik = 2^-(1 + (index mod 7)) on the logical [outer, C, inner] index -> (values, the integer-valued channel sums)"""
    idx = torch.arange(outer * C * inner)
    lik = torch.pow(2.0, -(1.0 + (idx % 7).float())).reshape(outer, C, inner)
    return lik, (1 + idx % 7).reshape(outer, C, inner).sum((0, 2)).float()


@pytest.mark.parametrize("outer,C,inner", R.SHAPES)
def test_exact_cases_are_bit_equal(outer, C, inner):
    """every term is a small integer and every partial sum an integer below 2^24: each channel equals its integer sum bit for bit in
    both storages (a dropped or doubled element shows); a channel of ones gives exactly 0; a NaN stays in its channel"""
    from hipops import ops
    lik, want = _exact(outer, C, inner)
    assert float(want.max()) < 2 ** 24
    ones = C // 2
    lik[:, ones, :] = 1.0
    want[ones] = 0.0
    for name, x, _ in _both(lik):
        got = ops.neg_log2_channel_sums(x)
        assert torch.equal(got.cpu(), want), name
        assert float(got[ones]) == 0.0
    bad_c = C - 1
    poisoned = lik.clone()
    poisoned[outer // 2, bad_c, inner // 2] = float("nan")
    keep = torch.arange(C) != bad_c
    for name, x, _ in _both(poisoned):
        got = ops.neg_log2_channel_sums(x).cpu()
        assert bool(torch.isnan(got[bad_c])) and int(torch.isnan(got).sum()) == 1, name
        assert torch.equal(got[keep], want[keep]), name


# ----------------------------------------------------------------------------- 3. consistency with the ordered scalar
@pytest.mark.parametrize("outer,C,inner", [(3, 5, 63), (2, 192, 256), (1536, 320, 1)])
def test_channel_sums_add_up_to_the_ordered_scalar(outer, C, inner):
    from hipops import ops
    from test_entropy_reference import ordered_bound
    lik = R.make_lik(outer, C, inner, seed=7)
    _, tot = R.channel_bits(lik, outer, C, inner)
    x = lik.reshape(outer, C, inner, 1).cuda()
    per_channel = float(ops.neg_log2_channel_sums(x).double().sum())
    scalar = float(ops.neg_log2_sum_ordered(x))
    allowed = float(R.channel_bound(outer, C, inner, tot).sum()) + ordered_bound(lik.numel(), float(tot.sum()))
    print(f"sum of channel sums {per_channel!r} | ordered scalar {scalar!r} | allowed difference {allowed:.3e}")
    assert abs(per_channel - scalar) <= allowed


# ----------------------------------------------------------------------------- the models
def _cheng():
    """the toy Cheng2020 of the unit report's tests (N = 8, four 64^2 images: z is 1 x 1 there, the inner = 1 NCHW case), W8 forward done"""
    from test_gpu_unit_report import _toy
    qnn, cali, _, _ = _toy()
    return qnn, cali


def _lu2022():
    import lic
    from quantization import QuantModel
    torch.manual_seed(1005)
    cfg = dict(height=64, width=64, in_chans=3, embed_dim=16, latent_dim=32, window_size=8, mlp_ratio=2.0, qkv_bias=True,
               qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_checkpoint=False)
    model = lic.NIC(cfg)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if p_.dim() >= 2 and "entropy_bottleneck" not in n_:
                p_.copy_((torch.rand(p_.shape, generator=g) - 0.5) * 2 * (3.0 / p_[0].numel()) ** 0.5)
    model = model.cuda().eval()
    cali = torch.rand(2, 3, 64, 64, generator=g).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:1])
    return qnn, cali


def _mark_trained(unit):
    from quantization import BaseQuantBlock, QuantModule
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.trained = True


def _by_hand(qnn, images, batch, set_state):
    """the state set by hand, the model run batch for batch; bits formed with torch in float64 from the likelihood tensors, the squared
    error with ops.sq_diff_sum_ordered -> (bits {key: float64 [C]}, derived bound of the bits {key: [C]}, sse, derived bound of sse)"""
    from hipops import ops
    from test_entropy_reference import ordered_bound
    set_state()
    bits, bound, sse, sse_bound = OrderedDict(), {}, 0.0, 0.0
    with torch.no_grad():
        for i in range(0, images.shape[0], batch):
            x = images[i:i + batch].contiguous()
            out = qnn(x)
            for k, lik in out["likelihoods"].items():
                t = -torch.log2(lik.double())
                B, C, H, W = lik.shape
                geom = (B, C, H * W) if lik.is_contiguous() else (B * H * W, C, 1)
                assert lik.is_contiguous() or lik.is_contiguous(memory_format=torch.channels_last)
                b = R.channel_bound(*geom, t.abs().sum((0, 2, 3)).cpu())
                bits[k] = bits.get(k, 0) + t.sum((0, 2, 3)).cpu()
                bound[k] = bound.get(k, 0) + b
            xh = out["x_hat"].contiguous()
            sse += float(ops.sq_diff_sum_ordered(xh, x, 1.0, clamp01=True).double())
            sse_bound += ordered_bound(x.numel(), float(((xh.double().clamp(0, 1) - x.double()) ** 2).sum()))
    return bits, bound, sse, sse_bound


def _check_row(row, hand, pixels, lmbda, fp=None):
    bits, bound, sse, sse_bound = hand
    assert list(row["bits"]) == list(bits)
    for k in bits:
        got = row["bits"][k]
        assert got.dtype == torch.float64 and got.device.type == "cpu" and got.shape == bits[k].shape
        assert bool(((got - bits[k]).abs() <= bound[k]).all()), k
    assert abs(row["sse"] - sse) <= sse_bound
    # the derived fields: the same formulas on the report's own sums
    total = float(sum(b.sum() for b in row["bits"].values()))
    assert row["bits_total"] == total
    mse = row["sse"] / (3 * pixels)
    want = dict(bpp=total / pixels, mse=mse, psnr_db=-10.0 * math.log10(mse), loss=total / pixels + lmbda * 255.0 ** 2 * mse)
    for f, v in want.items():
        assert row[f] == pytest.approx(v, rel=1e-12, abs=0), f
    if fp is None:
        assert not any(k.startswith("d_") for k in row)
        return
    for k in bits:
        assert torch.equal(row["d_bits"][k], row["bits"][k] - fp["bits"][k])
    for f in ("bpp", "mse", "psnr_db", "loss"):
        assert row["d_" + f] == row[f] - fp[f], f


def _report_against_hand(qnn, images, act_quant, batch, names, want_batch):
    units = qnn.units()
    rep = qnn.rd_report(images, lmbda=LMBDA, act_quant=act_quant, batch=batch, units=names)
    n, _, H, W = images.shape
    assert list(rep) == ["fp", "all", "units", "n", "pixels", "lmbda", "act_quant", "additivity", "batch"]
    assert (rep["n"], rep["pixels"], rep["lmbda"], rep["act_quant"], rep["batch"]) == (n, n * H * W, LMBDA, act_quant, want_batch)
    assert list(rep["units"]) == [u for u in units if u in names]
    P = n * H * W
    _check_row(rep["fp"], _by_hand(qnn, images, want_batch, lambda: qnn.set_quant_state(False, False)), P, LMBDA)
    _check_row(rep["all"], _by_hand(qnn, images, want_batch, lambda: qnn.set_quant_state(True, act_quant)), P, LMBDA, rep["fp"])
    for name in names:
        def only(name=name):
            qnn.set_quant_state(False, False)
            units[name].set_quant_state(True, act_quant)
        _check_row(rep["units"][name], _by_hand(qnn, images, want_batch, only), P, LMBDA, rep["fp"])
    add = rep["additivity"]
    assert sorted(add) == ["all_d_loss", "sum_units_d_loss"] and add["all_d_loss"] == rep["all"]["d_loss"]
    assert add["sum_units_d_loss"] == float(sum(r["d_loss"] for r in rep["units"].values()))
    return rep


def _same_report(a, b, rel=0.0):
    """two reports hold the same numbers: rel = 0 the same bits; rel > 0 every sum and every field derived from one state's sums to
    `rel` relative (the differences d_* of nearly equal numbers are left to the rows' own checks)"""
    def same(x, y, what):
        if isinstance(x, dict):
            assert list(x) == list(y), what
            for k in x:
                if rel == 0 or not (k.startswith("d_") or k == "additivity"):
                    same(x[k], y[k], f"{what}.{k}")
        elif torch.is_tensor(x):
            assert x.dtype == y.dtype and x.shape == y.shape, what
            assert torch.equal(x, y) if rel == 0 else bool(((x - y).abs() <= rel * y.abs()).all()), what
        elif isinstance(x, float) and rel > 0:
            assert x == pytest.approx(y, rel=rel, abs=0), what
        else:
            assert x == y, what
    same(a, b, "report")


# ----------------------------------------------------------------------------- 4. the report against a hand-made run
def test_report_matches_a_hand_made_run_on_toy_cheng2020():
    """W8, batches of two 64^2 images: y is 4 x 4, z is 1 x 1 (channels-last views of the kernels' outputs; z the inner = 1 case)"""
    qnn, cali = _cheng()
    names = ["g_a.0", "h_s.2.0"]
    assert all(n in qnn.units() for n in names)
    rep = _report_against_hand(qnn, cali, False, 2, names, 2)
    assert list(rep["fp"]["bits"]) == ["y", "z"]
    assert rep["fp"]["bits"]["y"].numel() == 8 and rep["fp"]["bits_total"] > 0 and math.isfinite(rep["all"]["psnr_db"])
    # every unit, and 'all' does not depend on the selection
    full = qnn.rd_report(cali, lmbda=LMBDA, batch=2)
    assert list(full["units"]) == list(qnn.units())
    _same_report(full["all"], rep["all"])
    _same_report(full["fp"], rep["fp"])
    for n in names:
        _same_report(full["units"][n], rep["units"][n])
    assert full["additivity"]["sum_units_d_loss"] == float(sum(r["d_loss"] for r in full["units"].values()))
    print(f"toy Cheng2020 W8: bpp fp {full['fp']['bpp']:.5f} all {full['all']['bpp']:.5f}; additivity {full['additivity']}")


def test_report_matches_a_hand_made_run_on_toy_lu2022():
    """W8A8 with dynamic grids on two units marked trained (a layer unit and the first Swin unit): the batch is 1 whatever is asked"""
    qnn, cali = _lu2022()
    names = list(qnn.units())[:2]
    assert names == ["g_a0", "g_a1"]
    for n in names:
        _mark_trained(qnn.units()[n])
    rep = _report_against_hand(qnn, cali, True, 8, names, 1)
    assert rep["all"]["bits_total"] != rep["fp"]["bits_total"]


# ----------------------------------------------------------------------------- 5. state restored, 6. the batch rule
@pytest.fixture(scope="module")
def static_model():
    """the toy Cheng2020 with the layer unit g_a.6 calibrated W8A8 on frozen static ranges (act_range='max'): AdaRound alpha, frozen
    ranges and `trained` on that unit, every other unit untrained"""
    from test_gpu_unit_report import _calibrate
    (qnn, name, u, _, _, batch), = _calibrate(["6"], act_mode="static", act_range="max")
    assert name == "6" and batch == 4 and u.act_quantizer.act_frozen() and qnn.units()["g_a.6"] is u
    g = torch.Generator().manual_seed(13)
    return qnn, torch.rand(4, 3, 64, 64, generator=g).cuda()


def _mixed_state(qnn):
    units = list(qnn.units().values())
    qnn.set_quant_state(False, False)
    for k, u in enumerate(units):
        u.set_quant_state(True, k % 2 == 0)
    units[1].set_quant_state(False, True)
    flags = {(m.use_weight_quant, m.use_act_quant) for m in qnn.modules() if hasattr(m, "use_weight_quant")}
    assert {(True, False), (True, True), (False, True)} <= flags
    assert qnn.units()["g_a.6"].trained and not units[0].trained


def _state(qnn):
    """flags and `trained`, delta, zero point, alpha (where the rounding was learned) and `_weight_state()` of every module, the frozen
    ranges and the recorded statistics of its quantiser"""
    from quantization import BaseQuantBlock, QuantModule
    out = []
    for name, m in qnn.named_modules():
        if not isinstance(m, (QuantModule, BaseQuantBlock)):
            continue
        row = {"name": name, "flags": (m.use_weight_quant, m.use_act_quant, m.trained),
               "ranges": {k: r.clone() for k, r in m.act_quantizer.act_range.items()},
               "act_stats": sorted(getattr(m.act_quantizer, "act_stats", None) or {}), "unit_stats": getattr(m, "unit_stats", None)}
        if isinstance(m, QuantModule) and m.org_weight is not None:
            q = m.weight_quantizer
            row.update(inited=getattr(q, "inited", True), delta=q.delta.clone(), zp=q.zero_point.clone(), wstate=m._weight_state())
            if hasattr(q, "alpha"):
                row.update(alpha=q.alpha.detach().clone(), alpha_id=id(q.alpha), soft=q.soft_targets)
        out.append(row)
    return out


def test_the_model_is_left_as_it_was_found(static_model, monkeypatch):
    from test_gpu_unit_report import _same_state
    qnn, cali = static_model
    _mixed_state(qnn)
    before = _state(qnn)
    assert any("alpha" in r for r in before) and any(r["ranges"] for r in before) and any(r["flags"][2] for r in before)
    qnn.rd_report(cali, lmbda=LMBDA, act_quant=True, batch=4, units=["g_a.0", "g_a.6"])
    _same_state(before, _state(qnn))
    assert qnn.unit_report() == {} and qnn.act_report() == {}
    # the forward raises half-way: the third state's first batch
    u = qnn.units()["g_a.1"]
    calls, real = [0], u.forward

    def failing(*a, **k):
        calls[0] += 1
        if calls[0] == 3:
            raise RuntimeError("planted failure")
        return real(*a, **k)
    monkeypatch.setattr(u, "forward", failing)
    with pytest.raises(RuntimeError, match="planted failure"):
        qnn.rd_report(cali, lmbda=LMBDA, act_quant=True, batch=4, units=["g_a.0", "g_a.6"])
    assert calls[0] == 3
    monkeypatch.undo()
    _same_state(before, _state(qnn))


def test_static_frozen_ranges_keep_the_batch(static_model):
    qnn, cali = static_model
    qnn.set_quant_state(True, True)
    rep = qnn.rd_report(cali, lmbda=LMBDA, act_quant=True, batch=4, units=["g_a.6"])
    assert rep["batch"] == 4 and rep["act_quant"] is True and list(rep["units"]) == ["g_a.6"]
    # the frozen grid is applied: the unit's row differs from a weights-only one
    w_only = qnn.rd_report(cali, lmbda=LMBDA, act_quant=False, batch=4, units=["g_a.6"])
    assert w_only["batch"] == 4
    assert not torch.equal(rep["units"]["g_a.6"]["bits"]["y"], w_only["units"]["g_a.6"]["bits"]["y"])


def test_dynamic_grids_run_image_by_image():
    """two units of the synthesis transform marked trained, dynamic grids (behind the latents' rounding a perturbation shows in x_hat;
    in front of it the rounding may absorb it)"""
    qnn, cali = _cheng()
    names = ["g_s.0", "g_s.1"]
    for n in names:
        _mark_trained(qnn.units()[n])
    eight = qnn.rd_report(cali, lmbda=LMBDA, act_quant=True, batch=8, units=names)
    one = qnn.rd_report(cali, lmbda=LMBDA, act_quant=True, batch=1, units=names)
    assert eight["batch"] == 1 and one["batch"] == 1
    _same_report(eight, one)
    # without activation quantisation nothing depends on the batch's company: the batch asked for is used
    w_only = qnn.rd_report(cali, lmbda=LMBDA, act_quant=False, batch=8, units=names)
    assert w_only["batch"] == 8
    # and the dynamic grids are in the numbers
    assert all(eight["units"][n]["sse"] != w_only["units"][n]["sse"] for n in names) and eight["all"]["sse"] != w_only["all"]["sse"]


# ----------------------------------------------------------------------------- 7. two ranks on one GPU
DP_UNITS = ["g_a.0", "g_s.7.0"]


def _plain(rep, back=False):
    """the report with numpy arrays for tensors (they travel through the queue by value), and back"""
    if isinstance(rep, dict):
        return OrderedDict((k, _plain(v, back)) for k, v in rep.items())
    if back and isinstance(rep, np.ndarray):
        return torch.from_numpy(rep)
    return rep.numpy() if torch.is_tensor(rep) else rep


def _dp_rank(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "rdo-ptq_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        qnn, cali = _cheng()
        rep = qnn.rd_report(cali[:3], lmbda=LMBDA, act_quant=False, batch=1, units=DP_UNITS)
        out_q.put((rank, _plain(rep)))
        dist.barrier()
    except BaseException as e:          # the parent must not wait out its queue timeout for a rank that failed
        out_q.put(("error", f"rank {rank}: {e!r}"))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_return_the_report_of_one():
    """Two processes on cuda:0 over gloo on three images (rank 0: images 0 and 2, rank 1: image 1), batch 1: both return the same report,
    'n' and 'pixels' are global, and the sums are the single process's to 1e-12 relative (the per-image fp32 values are the same; only
    the float64 addition order differs)"""
    qnn, cali = _cheng()
    want = qnn.rd_report(cali[:3], lmbda=LMBDA, act_quant=False, batch=1, units=DP_UNITS)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_dp_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(2):
            rk, val = q.get(timeout=180)
            assert rk != "error", val
            got[rk] = _plain(val, back=True)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    _same_report(got[0], got[1])
    assert got[0]["n"] == 3 and got[0]["pixels"] == 3 * 64 * 64 and got[0]["batch"] == 1
    _same_report(got[0], want, rel=1e-12)
    for row in [got[0]["fp"], got[0]["all"]] + list(got[0]["units"].values()):
        assert row["bits_total"] == pytest.approx(float(sum(b.sum() for b in row["bits"].values())), rel=1e-12)
