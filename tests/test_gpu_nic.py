"""Lu2022 path end to end on the GPU against the reference's own model code (tests/golden/recon_nic.npz was produced by
models/nic_cvt.py:NIC + quantization/* of the reference): state-dict compatibility of lic.NIC, unit schedule of the surgery,
cache building for six units (convs, transposed convs, RSTBs incl. shifted windows and a single-token window), and stage-wise
W8 / W8A8 forwards of the calibrated model through the Quant* Swin wrappers (HIP attention / LayerNorm / GELU kernels)."""
import os

import numpy as np
import pytest
import torch

from helpers import AQ, WQ, T

pytestmark = pytest.mark.gpu
CFG = dict(height=64, width=64, in_chans=3, embed_dim=16, latent_dim=32, window_size=8, mlp_ratio=2.0, qkv_bias=True,
           qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_checkpoint=False)


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def build(golden_dir):
    import lic
    from quantization import QuantModel
    fx = np.load(os.path.join(golden_dir, "recon_nic.npz"))
    model = lic.NIC(CFG)
    state = {k[len("state/"):]: T(fx[k]) for k in fx.files if k.startswith("state/")}
    model.load_state_dict(state, strict=True)                 # parameter / buffer names are the reference's
    model = model.cuda().eval()
    return fx, model


def install_trained(fx, name, unit):
    from quantization import QuantModule
    from quantization.quantizer import AdaRoundQuantizer, to_rows
    inner = [("", unit)] if isinstance(unit, QuantModule) else \
        [(n + ".", m) for n, m in unit.named_modules() if isinstance(m, QuantModule)]
    for n, m in inner:
        alpha = T(fx[f"{name}/{n}alpha_final"]).cuda()
        np.testing.assert_array_equal(m.weight_quantizer.delta.reshape(-1).cpu().numpy(), fx[f"{name}/{n}delta"].reshape(-1))
        ada = AdaRoundQuantizer(uaq=m.weight_quantizer, round_mode="learned_hard_sigmoid", weight_tensor=m.org_weight.data,
                                alpha_rows=to_rows(alpha, tconv=m.if_tconv))
        ada.soft_targets = False
        m.weight_quantizer = ada


def test_nic_fp_model_matches_reference(golden_dir):
    fx, model = build(golden_dir)
    x = T(fx["cali"])[:2].cuda()
    with torch.no_grad():
        y = model.g_a(x)
        out = model(x)
    assert _rel(y.cpu(), T(fx["fp/y"])) < 2e-5
    assert _rel(out["x_hat"].cpu(), T(fx["fp/x_hat"])) < 1e-4


def test_nic_caches_and_quantised_forwards_match_reference(golden_dir):
    from quantization import BaseQuantBlock, QuantModel, QuantModule
    from quantization.utils import save_inp_oup_data
    fx, model = build(golden_dir)
    B = int(fx["meta"][4])
    qnn = QuantModel(model=model, weight_quant_params=WQ, act_quant_params=AQ).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    cali = T(fx["cali"]).cuda()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:B])
    order = [n for n, m in qnn.model.named_children() if isinstance(m, (QuantModule, BaseQuantBlock))]
    assert order == [str(s) for s in fx["full_order"]]
    wanted = [str(o) for o in fx["order"]]
    qnn.set_quant_state(True, False)
    qnn.model.g_s7.set_quant_state(True, False)
    for name in order:
        unit = getattr(qnn.model, name)
        if name in wanted:
            (inp_q, inp_fp), out = save_inp_oup_data(qnn, unit, cali, asym=True, act_quant=False, batch_size=2, input_prob=True)
            for got, key in ((inp_q, "inp_q"), (inp_fp, "inp_fp"), (out, "out")):
                ref = T(fx[f"{name}/{key}"])
                assert tuple(got.shape) == tuple(ref.shape), (name, key)
                assert _rel(got.cpu(), ref) < 5e-5, (name, key, _rel(got.cpu(), ref))
            install_trained(fx, name, unit)
            unit.set_quant_state(True, False)
            with torch.no_grad():
                xin = T(fx[f"{name}/inp_q"])[:2].cuda()
                y = unit(xin) if isinstance(unit, QuantModule) else unit(xin, tuple(xin.shape[2:4]))
            assert _rel(y.cpu(), T(fx[f"{name}/hard_out"])) < 5e-5, name
        for m in unit.modules():
            if isinstance(m, (QuantModule, BaseQuantBlock)):
                m.trained = True
    qnn.eval()
    for tag, aq in (("w8", False), ("w8a8", True)):
        qnn.set_quant_state(True, aq)
        qnn.model.g_s7.set_quant_state(True, False)
        h = cali[:2]
        with torch.no_grad():
            for coder in ("g_a", "g_s"):
                for name in [n for n in order if n.startswith(coder)]:
                    unit = getattr(qnn.model, name)
                    h = unit(h) if isinstance(unit, QuantModule) else unit(h, tuple(h.shape[2:4]))
                    ref = T(fx[f"{tag}/{name}"])
                    err = _rel(h.cpu(), ref)
                    if not aq:
                        assert err < 1e-4, (tag, name, err)
                    else:
                        # W8A8: each Swin block re-quantises its activations at seven points with dynamic 8-bit grids.  A value
                        # on a rounding boundary may land one level off (1/255 of the channel range); window attention then
                        # spreads that to the window's tokens and later quantisers flip more.  From identical inputs every
                        # single stage is exact or flips < 0.3 % of its elements (tools/nic_w8a8_stage_check.py); over a whole RSTB the
                        # deviation must stay well below one quantisation level on average
                        mean_dev = float((h.cpu() - ref).abs().mean() / ref.abs().max())
                        assert err < 3e-2 and mean_dev < 2e-3, (tag, name, err, mean_dev)
                    h = ref.cuda()
                if coder == "g_a":
                    h = T(fx[f"{tag}/y_hat"]).cuda()


@pytest.mark.parametrize("name,task_p", [("g_a0", 2.0), ("g_a1", 2.0), ("g_a7", 2.0), ("h_a3", 2.0), ("h_s1", 2.0), ("g_s7", 2.0),
                                         ("h_s1", 2.4), ("g_a7", 2.4), ("h_a3", 1.5)])
def test_tape_engine_nic_units_match_oracle(golden_dir, name, task_p):
    """Hot loop of the Lu2022 units on the HIP tape engine vs the oracle (pinned to the reference's block_/layer_reconstruction
    on the same caches): conv with a 7-stage FP tail, shifted-window RSTB with a 6-stage tail, RSTB with a round-only tail,
    single-token RSTB (plain rec == task), transposed conv with a tail, last transposed conv.  Same mini-batch indices and
    counter-RNG QDrop masks on both sides; tolerances as in test_gpu_engine.py."""
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    import test_oracle_golden as TG
    from oracle import rdo_oracle as O, swin_oracle as S
    from quantization import BaseQuantBlock, QuantModel, QuantModule
    from quantization.recon import fp_out, _unit_modules
    from quantization.quant_layer import _nhwc
    from quantization.swin_engine import TapeEngine
    from helpers import nhwc
    SEED = 1005
    fx, model = build(golden_dir)
    B, iters = int(fx["meta"][4]), int(fx["meta"][5])
    idx = fx[f"{name}/idx"]
    # --- oracle
    _, nic = TG._nic(golden_dir)
    unit_o = nic.stages[name]
    if isinstance(unit_o, S.RstbOracle):
        ops_o, fwd = unit_o.ops, (lambda ops_, x: unit_o(x))
    else:
        ops_o, fwd = {"layer": unit_o}, "layer"
    log = O.reconstruct_unit(fwd, ops_o, T(fx[f"{name}/inp_q"]), T(fx[f"{name}/inp_fp"]), T(fx[f"{name}/out"]), iters=iters,
                             batch_size=B, idx_stream=idx, mask_fn=lambda i, shape: O.qdrop_keep_mask_nhwc(SEED, i, shape, 0.5),
                             tail=nic.tail_of(name), task_p=task_p)
    # --- product
    qnn = QuantModel(model=model, weight_quant_params=WQ, act_quant_params=AQ).cuda().eval()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(T(fx["cali"])[:B].cuda())                       # scale init
    qnn.set_quant_state(False, False)
    order = [n for n, m in qnn.model.named_children() if isinstance(m, (QuantModule, BaseQuantBlock))]
    coder = [n for n in order if n.startswith(name[:3])]
    tail = [getattr(qnn.model, n) for n in coder[coder.index(name) + 1:]]
    tail_round = name.startswith("g_a")
    unit = getattr(qnn.model, name)
    kind, mods = _unit_modules(unit)
    out_c = T(fx[f"{name}/out"]).cuda()
    task_cache = _nhwc(fp_out(tail, out_c, tail_round)) if (tail or tail_round) else None
    eng = TapeEngine(kind, mods, nhwc(fx[f"{name}/inp_q"]), nhwc(fx[f"{name}/inp_fp"]), nhwc(fx[f"{name}/out"]),
                     tail=tail, tail_round=tail_round, task_cache=task_cache, batch_size=B, iters=iters, seed=SEED,
                     idx_table=torch.from_numpy(idx), task_p=task_p)
    eng.run()
    torch.cuda.synchronize()
    total, _, _ = eng.logs()
    # analysis-transform units end in round_ste: a latent within fp32 noise of x.5 rounds the other way on the GPU and moves
    # the task term by up to (2|d|+1)/(B*H*W) -- allow three such events; everything else is compared at 3e-4 relative
    atol = 3.0 * 3.0 / (task_cache.shape[0] and (B * task_cache.shape[1] * task_cache.shape[2])) if tail_round else 1e-7
    np.testing.assert_allclose(total.numpy(), np.array(log.total), rtol=3e-4, atol=atol)
    flips = tot = 0
    for k, op in ops_o.items():
        a_gpu = eng.alpha_of(k).cpu()
        assert a_gpu.shape == op.alpha.shape, (k, a_gpu.shape, op.alpha.shape)
        np.testing.assert_allclose(a_gpu.numpy(), op.alpha.numpy(), rtol=0, atol=2e-3, err_msg=k)
        flips += int(((a_gpu >= 0) != (op.alpha >= 0)).sum())
        tot += a_gpu.numel()
    assert flips <= 0.005 * tot, f"{flips}/{tot} rounding decisions differ"
    eng.finish()
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.trained = True
    unit.set_quant_state(True, False)
    with torch.no_grad():
        xin = T(fx[f"{name}/inp_q"])[:2]
        y = unit(xin.cuda()) if isinstance(unit, QuantModule) else unit(xin.cuda(), tuple(xin.shape[2:4]))
        y_ref = unit_o(xin)
    err = _rel(y.cpu(), y_ref)
    assert err < (5e-3 if flips else 5e-5), err


@pytest.mark.parametrize("name", ["g_a0", "g_a1", "h_s1", "g_a7"])
def test_tape_engine_first_iteration_gradient(golden_dir, name):
    """d(rec + task)/d alpha of the first iteration (rounding regulariser still off): tape engine (data-parallel op sequence,
    plan A only) against torch autograd through the oracle's unit + FP tail.  1e-4 of the largest gradient entry."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "nic_grad_check.py"), name],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rels = [float(l.split("rel")[1]) for l in out.stdout.splitlines() if " rel " in l]
    assert rels and max(rels) < 1e-4, out.stdout


@pytest.mark.parametrize("name", ["g_a1", "h_s1"])
def test_tape_engine_dp_split_equals_fused(golden_dir, name):
    """The data-parallel op sequence of the tape engine (plan A: forward/backward + rdo_adaround_grad into the flat bucket; plan B:
    rdo_adaround_apply) on one rank reproduces the fused rdo_adaround_step run bit for bit -- for an RSTB with a tail and a
    transposed-conv layer unit with a tail."""
    from quantization import BaseQuantBlock, QuantModel, QuantModule
    from quantization.recon import fp_out, _unit_modules
    from quantization.quant_layer import _nhwc
    from quantization.swin_engine import TapeEngine
    from helpers import nhwc
    res = []
    for split in (False, True):
        fx, model = build(golden_dir)
        B, iters = int(fx["meta"][4]), int(fx["meta"][5])
        qnn = QuantModel(model=model, weight_quant_params=WQ, act_quant_params=AQ).cuda().eval()
        qnn.set_quant_state(True, False)
        with torch.no_grad():
            qnn(T(fx["cali"])[:B].cuda())
        qnn.set_quant_state(False, False)
        order = [n for n, m in qnn.model.named_children() if isinstance(m, (QuantModule, BaseQuantBlock))]
        coder = [n for n in order if n.startswith(name[:3])]
        tail = [getattr(qnn.model, n) for n in coder[coder.index(name) + 1:]]
        tail_round = name.startswith("g_a")
        kind, mods = _unit_modules(getattr(qnn.model, name))
        task_cache = _nhwc(fp_out(tail, T(fx[f"{name}/out"]).cuda(), tail_round))
        eng = TapeEngine(kind, mods, nhwc(fx[f"{name}/inp_q"]), nhwc(fx[f"{name}/inp_fp"]), nhwc(fx[f"{name}/out"]), tail=tail,
                         tail_round=tail_round, task_cache=task_cache, batch_size=B, iters=iters, seed=7,
                         idx_table=torch.from_numpy(fx[f"{name}/idx"]), force_dp_split=split)
        eng.run()
        torch.cuda.synchronize()
        res.append(({n: eng.alpha_of(n).clone() for n in eng.ops}, eng.logs()[0]))
    for n in res[0][0]:
        torch.testing.assert_close(res[0][0][n], res[1][0][n], rtol=0, atol=0)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-6, atol=0)


def test_tail_weight_preparation_runs_eagerly_inside_a_recording():
    """A frozen tail op is built while the engine's plan is being RECORDED; the layouts derived from its weight (the phase weight of a
    transposed conv) must be computed there and then -- `fill_planes` splits them right after the recording, before any replay -- and
    must not become ops of the plan."""
    from hipops import ops
    from hipops.plan import Plan
    from quantization import QuantModule
    from quantization.swin_engine import _FpOp
    torch.manual_seed(0)
    qm = QuantModule(torch.nn.ConvTranspose2d(32, 48, 5, stride=2, padding=2, output_padding=1), WQ, AQ).cuda()
    plan = Plan()
    with plan.record():
        p = _FpOp(qm)
        assert p.tc_phase is not None
        want = None
        with Plan.eager():
            want = ops.tconv_expand(p.w, p.tc_phase)
        torch.cuda.synchronize()
        assert torch.equal(p.wp, want)                      # already there: nothing waits for a replay
    assert plan.num_ops == 0
    assert float(p.wp.abs().max()) > 0


@pytest.mark.parametrize("B,Ho,C", [(4, 64, 192), (2, 16, 32)])
def test_strided_conv_input_gradient_in_phase_form(B, Ho, C):
    """dgrad of conv(k = 3, s = 2, p = 1) = stride-1 conv of dy with the phase weight of the transposed conv + pixel shuffle (what the tape
    engine records for the tail's strided convs; the large shape runs on the split-precision kernel) against zero insertion + dense
    conv on the fp32 kernel, and both against torch."""
    from hipops import ops
    torch.manual_seed(1)
    K, s, pad = 3, 2, 1
    w = torch.randn(C, K, K, C, device="cuda") / (C * K * K) ** 0.5          # conv rows [Cout][KH][KW][Cin]
    dy = torch.randn(B, Ho, Ho, C, device="cuda")
    H = Ho * s
    opad = H - ((Ho - 1) * s - 2 * pad + K)
    ph = ops.TconvPhase.get(K, s, pad, opad, False, dy.device)
    assert ph is not None
    wbp = ops.tconv_expand(w.permute(3, 1, 2, 0).contiguous(), ph)
    planes = ops.split_bf16x3(wbp) if ops.uses_bf16x6(tuple(dy.shape), tuple(wbp.shape), 1, ph.pad) else None
    assert (planes is not None) == (C == 192)
    dp = ops.conv2d_fwd(dy, wbp, None, 1, ph.pad, wplanes=planes)
    dx = ops.pixel_shuffle(dp, s)
    q = K - 1 - pad
    Hu = (Ho - 1) * s + 1 + 2 * q + opad
    du = ops.zero_insert(dy, s, q, q, Hu, Hu)
    ref = ops.conv2d_fwd(du, w.permute(3, 1, 2, 0).flip(1, 2).contiguous(), None, 1, 0)
    assert dx.shape == ref.shape == (B, H, H, C)
    x = torch.zeros(B, C, H, H, device="cuda", dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(x, w.permute(0, 3, 1, 2).double(), None, s, pad)
    y.backward(dy.permute(0, 3, 1, 2).double())
    want = x.grad.permute(0, 2, 3, 1)
    scale = float(want.abs().max())
    assert float((dx.double() - want).abs().max()) <= 3e-6 * scale
    assert float((ref.double() - want).abs().max()) <= 3e-6 * scale


@pytest.mark.parametrize("name", ["g_a1", "g_a0", "h_s1", "g_s2"])
def test_rd_task_loss_mode_on_lu2022_units_matches_oracle(golden_dir, name):
    """loss_mode='rd' on the Lu2022 coders (missing 4): the task term of every iteration is
    lambda * 255^2 * MSE(x_hat, x) + bpp of the WHOLE NIC with the unit's soft-quantised output substituted (losses/losses.py:8-35; the
    call the reference sketches and comments out, layer_opt.py:146-148) -- the Swin blocks, convs, transposed convs and entropy models
    BEHIND the unit run under torch's tape on the HIP kernels (hipops.autograd: Linear, LayerNorm, window attention, GELU, likelihoods).
    Through the public layer_/block_reconstruction against `oracle.reconstruct_unit(task_fn=...)` running `swin_oracle.NicModelOracle` on
    the CPU: an RSTB in g_a (shifted windows; everything behind it incl. both entropy models is differentiated), the 5x5 stem, a
    transposed conv of h_s, an RSTB in g_s.  rec to 3e-4, task to 2e-3 relative (rounded latents: one flip moves the rate), alphas as
    in the lp tests."""
    import types
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    import test_oracle_golden as TG
    from oracle import lic_oracle as LO, rdo_oracle as O, swin_oracle as S
    from quantization import BaseQuantBlock, QuantModel, QuantModule, block_reconstruction, layer_reconstruction
    from quantization.recon import unit_seed
    fx, model = build(golden_dir)
    state = {k[len("state/"):]: T(fx[k]) for k in fx.files if k.startswith("state/")}
    B, iters, lmbda = 2, 6, 0.0483
    cali = T(fx["cali"])
    n_img = cali.shape[0]
    torch.manual_seed(1005)
    qnn = QuantModel(model=model, weight_quant_params=WQ, act_quant_params=AQ).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:B].cuda())
    unit = getattr(qnn.model, name)
    fn = layer_reconstruction if isinstance(unit, QuantModule) else block_reconstruction
    args = types.SimpleNamespace(lmbda=lmbda, task_loss=2.0, arch="Lu2022", loss_mode="rd")
    eng = fn(qnn, unit, name, cali_data=cali.cuda(), batch_size=B, iters=iters, weight=0.01, input_prob=0.5, lr=4e-5, asym=True,
             b_range=(20, 2), warmup=0.2, act_quant=False, opt_mode="mse", config=None, args=args)
    torch.cuda.synchronize()
    assert eng.rd is not None and eng.rd_path in ("graph", "host")
    rec, task, rnd, _ = eng.logs_terms()
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous().cpu()
    inp_q, inp_fp, out_fp = nchw(eng.cq), nchw(eng.cf), nchw(eng.co)
    idx = eng.idx.cpu().numpy()
    seed = unit_seed(name)
    # ---- oracle: the loop of reconstruct_unit with the RD task term through the oracle NIC
    mo = S.NicModelOracle({k: v.clone() for k, v in state.items()}, CFG)
    unit_o = mo.nic.stages[name]
    ops_o, fwd = (unit_o.ops, (lambda ops_, x: unit_o(x))) if isinstance(unit_o, S.RstbOracle) else ({"layer": unit_o}, "layer")
    LO.STE_ROUND = True
    try:
        def task_fn(out_quant, ix):
            x = cali[ix]
            o = mo.forward(x, substitute=(name, out_quant))
            n_pix = x.shape[0] * x.shape[2] * x.shape[3]
            bpp = sum((-torch.log2(v)).sum() for v in o["likelihoods"].values()) / n_pix
            return lmbda * 255 ** 2 * ((o["x_hat"] - x) ** 2).mean() + bpp
        log = O.reconstruct_unit(fwd, ops_o, inp_q, inp_fp, out_fp, iters=iters, batch_size=B, idx_stream=idx,
                                 mask_fn=lambda i, shape: O.qdrop_keep_mask_nhwc(seed, i, shape, 0.5), input_prob=0.5, weight=0.01,
                                 b_range=(20, 2), warmup=0.2, task_fn=task_fn)
    finally:
        LO.STE_ROUND = False
    np.testing.assert_allclose(rec.numpy(), np.array(log.rec), rtol=3e-4, atol=1e-7)
    np.testing.assert_allclose(task.numpy(), np.array(log.task), rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(rnd.numpy(), np.array(log.round), rtol=3e-4, atol=1e-7)
    flips = tot = 0
    for k, op in ops_o.items():
        a_gpu = eng.alpha_of(k).cpu()
        assert a_gpu.shape == op.alpha.shape, k
        far = ((a_gpu - op.alpha).abs() > 2e-3).float().mean()
        assert float(far) < 5e-3, (k, float(far))
        flips += int(((a_gpu >= 0) != (op.alpha >= 0)).sum())
        tot += a_gpu.numel()
    assert flips <= 0.005 * tot, f"{flips}/{tot} rounding decisions differ"
