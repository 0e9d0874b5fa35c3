"""The batched learned-rounding step on the MX grids (csrc/mx_round_batch.hip) on the GPU: bit for bit against `ops.mx_round_step` and the
split wrappers on copies of one state (the rounding loss against float64 at test_gpu_mx_round.py's 1e-5), one step against float64 at that
file's bounds, the carried gather against the stand-alone ones, and the engine with args.batch_step True and False."""
import functools
import types

import pytest
import torch

import mx_reference as R
import mx_round_reference as RR
from test_gpu_adaround_step import REPARAM, ROUND_WEIGHT, _counter, _dev_sched, _gamma_like, _log, guards_intact, sched_table
from test_gpu_mx_round import _kinks, _same_bits, restate_fp32, step_case, step_reference, tolerances

pytestmark = pytest.mark.gpu
# name: shape [rows, KH, KW, Cin] (a gamma: [C, C]), conv planes (None | 'h2' | 'bf16'), Linear planes, reparam
TENSORS = {"conv_h2": ((32, 3, 3, 32), "h2", False, False), "conv_bf16": ((48, 1, 1, 64), "bf16", False, False),
           "linear": ((64, 1, 1, 96), None, True, False), "gamma": ((32, 32), None, False, True), "odd": ((6, 1, 1, 10), None, False, False)}
BATCHES = {1: ["conv_h2"], 3: ["conv_bf16", "linear", "gamma"], 8: ["odd", "conv_h2", "gamma", "linear", "conv_bf16", "odd", "conv_h2", "gamma"]}
SENTINEL = {"alpha": 7.25, "m": -3.5, "v": 11.0}
OUT = ("alpha", "m", "v", "wq", "wd", "wq_planes", "wd_planes", "lin_fwd", "lin_bwd")


@functools.lru_cache(maxsize=None)
def tensor_case(name, fmt, slot):
    """CPU state of tensor `name` as tensor number `slot` of a batch: nsplit 1 or 3 by the slot, two pinned elements with sentinels in
    alpha, m and v"""
    shape, _, _, gamma = TENSORS[name]
    g = torch.Generator().manual_seed(100 * slot + len(name))
    w = (_gamma_like(shape[0], g) if gamma else 0.1 * torch.randn(shape, generator=g)).float()
    rows = shape[0]
    top = R.FORMATS[fmt][5] * float(torch.ldexp(torch.ones(()), R.quantize(w.reshape(rows, -1), fmt)["scales"][0, 0].int() - 127))
    w.view(-1)[0], w.view(-1)[5] = top, top if gamma else -top * (1 + 2.0 ** -20)          # +max X, just below -max X: the scale stays
    nb = RR.neighbours(w.reshape(rows, -1), fmt)
    lo, gap = nb["lo"].reshape(shape), nb["gap"].reshape(shape)
    pinned = gap == 0
    assert bool(pinned.view(-1)[0]) and bool(pinned.view(-1)[5]) and int(pinned.sum()) < w.numel() // 4
    nsplit = 1 if slot % 2 else 3
    state = {"pert": 3.0 * torch.randn(shape, generator=g), "m": 1e-3 * torch.randn(shape, generator=g),
             "v": (1e-3 * torch.randn(shape, generator=g)).pow(2), "slabs": 1e-2 * torch.randn((nsplit,) + shape, generator=g)}
    return types.SimpleNamespace(name=name, shape=shape, w=w, lo=lo, gap=gap, pinned=pinned, reparam=REPARAM if gamma else None, **state)


def device_item(c):
    """the item of `ops.mx_round_step_batch` for case c: alpha from `mx_round_init_alpha`, perturbed across both clamps of h"""
    from hipops import ops
    _, planes, lin, _ = TENSORS[c.name]
    lo, gap = c.lo.cuda(), c.gap.cuda()
    it = dict(d=ops.ada_desc(lo, reparam=c.reparam), lo=lo, gap=gap, slabs=c.slabs.cuda(), m=c.m.cuda(), v=c.v.cuda(), wq=torch.empty_like(lo),
              wd=torch.empty_like(lo), alpha=ops.mx_round_init_alpha(c.w.cuda(), lo, gap) + c.pert.cuda())
    assert bool((it["alpha"] > 2.5).any()) and bool((it["alpha"] < -2.5).any())
    for k, s in SENTINEL.items():
        it[k][c.pinned.cuda()] = s
    i16 = lambda n: torch.full((n,) + tuple(lo.shape), 0x5555, dtype=torch.int16, device="cuda")
    for k in (("wq_planes", "wd_planes") if planes else ()):
        it[k] = ops.H2(i16(2), 4.0) if planes == "h2" else i16(3)
    for k in (("lin_fwd", "lin_bwd") if lin else ()):
        it[k] = ops.H2(i16(2), 8.0)
    return it


def per_tensor_path(it, grad_scale, counter, log):
    """what the batched launch replaces for one tensor: the step with its transpose launch, then one split launch per plane buffer"""
    from hipops import ops
    ops.mx_round_step(it["d"], it["lo"], it["gap"], it["slabs"], grad_scale, ROUND_WEIGHT, _dev_sched(), counter, it["alpha"], it["m"], it["v"],
                      it["wq"], it["wd"], log)
    co, ci = it["lo"].shape[0], it["lo"].shape[-1]
    taps = tuple(it["lo"].shape[1:3]) if it["lo"].dim() == 4 else (1, 1)
    wq4, wd4 = it["wq"].reshape(co, *taps, ci), it["wd"].reshape(ci, *taps, co)
    for k, w4 in (("wq_planes", wq4), ("wd_planes", wd4)):
        if k in it:
            ops.split_h2_conv(w4, planes=it[k]) if isinstance(it[k], ops.H2) else ops.split_bf16x3(w4, it[k])
    for k, w4 in (("lin_fwd", wq4), ("lin_bwd", wd4)):
        if k in it:
            ops.split_h2_linear(w4, planes=it[k])


@pytest.mark.parametrize("counter,hand_over", [(0, False), (2, True)])          # a warm-up row (round_on = 0) and one behind it
@pytest.mark.parametrize("fmt", ["mxfp4", "mxfp8_e4m3"])
@pytest.mark.parametrize("n", sorted(BATCHES))
def test_batch_equals_the_per_tensor_path_bit_for_bit(n, fmt, counter, hand_over):
    from hipops import ops
    cases = [tensor_case(name, fmt, slot) for slot, name in enumerate(BATCHES[n])]
    got, want = [device_item(c) for c in cases], [device_item(c) for c in cases]
    start = [it["alpha"].cpu() for it in got]
    raw = lambda x: (lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t)(x.t if isinstance(x, ops.H2) else x)
    word, shadow, log = _counter(counter), _counter(-7), _log()
    ops.mx_round_step_batch(got, 0.5, ROUND_WEIGHT, _dev_sched(), word, log, **(dict(iter_shadow=shadow) if hand_over else dict(advance_iter=word)))
    word_ref, log_ref = _counter(counter), _log()
    for it in want:
        per_tensor_path(it, 0.5, word_ref, log_ref)
    ops.iter_advance(word_ref)
    torch.cuda.synchronize()
    assert (word.tolist(), shadow.tolist()) == (([counter], [counter + 1]) if hand_over else ([counter + 1], [-7])) and word_ref.tolist() == [counter + 1]
    loss = 0.0
    for c, a, b, alpha0 in zip(cases, got, want, start):
        for k in OUT:
            assert k not in a or torch.equal(raw(a[k]), raw(b[k])), (c.name, k)
        pin = c.pinned.cuda()
        assert all(bool((a[k][pin] == s).all()) for k, s in SENTINEL.items()), c.name           # a pinned element is never written
        assert torch.equal(a["wq"].cpu()[c.pinned], (c.lo if c.reparam is None else c.lo.clamp(min=REPARAM[0]) ** 2 - REPARAM[1])[c.pinned])
        ref = RR.step(c.lo, c.gap, alpha0, c.m, c.v, c.slabs.double().sum(0), sched_table()[counter], grad_scale=0.5, round_weight=ROUND_WEIGHT,
                      reparam=c.reparam)
        loss += float(ref["round_loss"])
    log = log.cpu().double()
    if float(sched_table()[counter, 1]):
        assert loss > 0 and abs(float(log[counter].sum()) - loss) <= 1e-5 * loss
    assert float(log.abs().sum() - log[counter].abs().sum()) == 0.0 and (float(sched_table()[counter, 1]) or float(log.abs().sum()) == 0.0)


@pytest.mark.parametrize("state,counter,grad_scale", [("mid", 2, 0.5), ("first", 4, 1.0), ("mid", 0, 0.5)])
@pytest.mark.parametrize("fmt", ["mxfp4", "mxfp8_e4m3"])
def test_one_batched_step_matches_float64(fmt, state, counter, grad_scale):
    """three cases of tests/test_gpu_mx_round.py (numel % 4 == 0; a conv, a many-slab 1 x 1, a gamma) in one launch, held to that file's bounds"""
    from hipops import ops
    from test_gpu_mx_round import make_item
    names = ["A40x2x3x36", "C32x1x1x96", "G64"]
    items = [make_item(step_case(nm, fmt), state) for nm in names]
    ops.mx_round_step_batch([{k: v for k, v in it.items() if k != "_bufs"} for it in items], grad_scale, ROUND_WEIGHT, _dev_sched(), _counter(counter),
                            _log())
    torch.cuda.synchronize()
    for nm, item in zip(names, items):
        c, ref = step_case(nm, fmt), step_reference(nm, fmt, state, counter, grad_scale)
        fp32 = restate_fp32(c, state, counter, grad_scale)
        h_err = float((fp32.pop("h").double() - ref["masks"]["h"]).abs()[c.live].max())
        tol = tolerances(c, ref, state, counter, grad_scale, h_err)
        keep = c.live & ~_kinks(c, ref)
        for k in ("alpha", "m", "v", "wq"):
            err = (item[k].cpu().double() - ref[k]).abs()
            share = float((err / tol[k].clamp(min=1e-300))[keep].max())
            e32 = float((fp32[k].double() - ref[k]).abs()[keep].max()) if k in fp32 else 0.0
            assert share <= 1.0 or 0.0 < (float(err[keep].max()) / e32 if e32 > 0 else 0.0) <= 2.0, (nm, k, share)
        co, ci, taps = c.shape[0], c.shape[-1], (tuple(c.shape[1:3]) if len(c.shape) == 4 else (1, 1))
        assert torch.equal(item["wd"].reshape(ci, *taps, co), item["wq"].reshape(co, *taps, ci).flip(1, 2).permute(3, 1, 2, 0).contiguous())
        guards_intact(item)


@pytest.mark.parametrize("planes", [False, True])
def test_carried_gather_equals_the_stand_alone_gather(planes):
    from hipops import ops
    g = torch.Generator().manual_seed(5)
    cq, cf = torch.randn(6, 9, 8, 32, generator=g).cuda(), torch.randn(6, 9, 8, 32, generator=g).cuda()       # 144 pixels: a ragged block of 64
    idx = torch.randint(0, 6, (5, 2), generator=g, dtype=torch.int32).cuda()
    make = lambda: (torch.full((2, 9, 8, 32), -5.0, device="cuda"), ops.h2_empty((2, 9, 8, 32), "cuda", 2.0) if planes else None)
    for counter in (1, 4):                                                        # 4: the last row, nothing may be written behind it
        out, pl = make()
        if pl is not None:
            pl.t.fill_(0x5555)
        item = device_item(tensor_case("odd", "mxfp4", 0))
        ops.mx_round_step_batch([item], 1.0, ROUND_WEIGHT, _dev_sched(), _counter(counter), _log(), iter_shadow=_counter(0),
                                gather=dict(cache_q=cq, cache_fp=cf, idx_table=idx, B=2, batch_offset=1, prob=0.5, seed=11, out=out, out_planes=pl))
        want, wpl = make()
        if counter == 4:
            assert bool((out == -5.0).all()) and (pl is None or bool((pl.t == 0x5555).all()))
            continue
        if planes:
            ops.gather_qdrop_h2(cq, cf, idx, _counter(counter + 1), 2, 0.5, 11, want, wpl, batch_offset=1)
            assert torch.equal(pl.t, wpl.t)
        else:
            ops.gather_qdrop(cq, cf, idx, _counter(counter + 1), 2, 0.5, 11, want, batch_offset=1)
        assert _same_bits(out, want)


def _calibrate(kind, batch_step, monkeypatch):
    """one unit of a toy Cheng2020 (32 channels, 16^2 / 8^2 maps, batch 2, 6 iterations) on mxfp4 with learned rounding -> alphas, hard
    weights, calls of the per-tensor entry"""
    import lic
    from hipops import ops
    from quantization import QuantModel, QuantModule, block_reconstruction, layer_reconstruction
    torch.manual_seed(1005)
    model = lic.Cheng2020Anchor(N=32).cuda().eval()
    cali = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(13)).cuda()
    params = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    qnn = QuantModel(model=model, weight_quant_params=params, act_quant_params=dict(params, leaf_param=False), is_cheng=True).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:2])
    name = {"rb": "g_a.3", "layer": "g_a.6"}[kind]
    unit = qnn.units()[name]
    qnn.set_weight_format({name: "mxfp4"}, rounding="learned")
    calls, real = [], ops.mx_round_step
    monkeypatch.setattr(ops, "mx_round_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(7)
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Cheng2020", batch_step=batch_step)
    (block_reconstruction if kind == "rb" else layer_reconstruction)(
        qnn, unit, name.split(".")[-1], cali_data=cali, batch_size=2, iters=6, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2),
        warmup=0.2, act_quant=False, opt_mode="mse", config=None, args=args)
    mods = [m for m in unit.modules() if isinstance(m, QuantModule) and m.org_weight is not None]
    return [m.weight_quantizer.alpha.clone() for m in mods], [m.weight_quantizer(m.weight).clone() for m in mods], len(calls)


@pytest.mark.parametrize("kind", ["layer", "rb"])
def test_engine_batched_and_per_tensor_steps_agree(kind, monkeypatch):
    alpha_b, hard_b, calls_b = _calibrate(kind, True, monkeypatch)
    monkeypatch.undo()
    alpha_p, hard_p, calls_p = _calibrate(kind, False, monkeypatch)
    assert calls_b == 0 and calls_p >= len(alpha_p) == len(alpha_b) >= 1
    assert all(_same_bits(a, b) for a, b in zip(alpha_b, alpha_p)) and all(_same_bits(a, b) for a, b in zip(hard_b, hard_p))
