"""Differentiable MS-SSIM: rdo_ssim_level_bwd / rdo_avg_pool2_bwd against float64 autograd of the oracle, the tracked
`losses.ms_ssim` / `RateDistortionLoss(metric='ms-ssim')`, the calibration engine's R + lambda*D mode with the MS-SSIM distortion
against the oracle loop, and the `args.rd_metric` surface of layer_/block_reconstruction."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
SEED = 1005
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.fixture
def oracle64(monkeypatch):
    """oracle.msssim_oracle with its window in float64 (the module builds it in float32), for float64 autograd references."""
    from oracle import msssim_oracle as MO
    win32 = MO.gaussian_window
    monkeypatch.setattr(MO, "gaussian_window", lambda *a, **k: win32(*a, **k).double())
    return MO


def _pair(planes, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(planes, H, W, generator=g)
    y = x + 0.05 * torch.randn(planes, H, W, generator=g)
    return x, y, g


@pytest.mark.parametrize("H,W", [(256, 256), (255, 257), (161, 161)])
def test_ssim_level_bwd_matches_float64_autograd(H, W):
    from hipops import ops
    from losses.losses import _MS_WINDOW
    from oracle import msssim_oracle as MO
    planes = 6
    x, y, g = _pair(planes, H, W, 11 + H + W)
    gs, gc = torch.randn(planes, generator=g), torch.randn(planes, generator=g)
    x64 = x.double()[None].requires_grad_(True)
    s, c = MO.ssim_level(x64, y.double()[None], MO.gaussian_window().double())
    assert float(c.detach().min()) > 0
    (ref,) = torch.autograd.grad((s[0] * gs.double()).sum() + (c[0] * gc.double()).sum(), x64)
    xd, yd, gsd, gcd = x.cuda(), y.cuda(), gs.cuda(), gc.cuda()
    d1 = ops.ssim_level_bwd(xd, yd, _MS_WINDOW, C1, C2, gsd, gcd)
    d2 = ops.ssim_level_bwd(xd, yd, _MS_WINDOW, C1, C2, gsd, gcd)
    torch.cuda.synchronize()
    assert _rel(d1, ref[0]) <= 1e-4, _rel(d1, ref[0])
    assert torch.equal(d1, d2)


@pytest.mark.parametrize("H,W", [(256, 256), (255, 257), (161, 161)])
def test_avg_pool2_bwd_is_the_exact_adjoint(H, W):
    from hipops import ops
    planes = 6
    x, _, g = _pair(planes, H, W, 5 + H * W)
    x64 = x.double()[None].requires_grad_(True)
    out = F.avg_pool2d(x64, 2, padding=(H % 2, W % 2))
    go = torch.randn(out.shape, generator=g)
    (ref,) = torch.autograd.grad(out, x64, go.double())
    gd = go[0].cuda()
    d1, d2 = ops.avg_pool2_bwd(gd, H, W), ops.avg_pool2_bwd(gd, H, W)
    torch.cuda.synchronize()
    assert torch.equal(d1.cpu(), ref[0].float())
    assert torch.equal(d1, d2)


def test_ms_ssim_is_differentiable_and_keeps_its_value(oracle64):
    from losses.losses import ms_ssim
    MO = oracle64
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 256, 256, generator=g)
    y = (x + 0.05 * torch.randn(x.shape, generator=g)).clamp(0, 1)
    xd, yd = x.cuda(), y.cuda()
    plain = ms_ssim(xd, yd)
    xt = xd.clone().requires_grad_(True)
    val = ms_ssim(xt, yd)
    assert val.grad_fn is not None
    (gx,) = torch.autograd.grad(val, xt)
    torch.cuda.synchronize()
    assert torch.equal(val.detach(), plain)
    x64 = x.double().requires_grad_(True)
    ref_val = MO.ms_ssim(x64, y.double())
    (ref,) = torch.autograd.grad(ref_val, x64)
    assert abs(float(val.detach()) - float(ref_val.detach())) < 1e-5
    assert _rel(gx, ref) <= 1e-4, _rel(gx, ref)


def _toy_cheng(N=8, seed=41):
    """The toy Cheng2020 of the RD engine tests (reference-model parameters, GDN gammas well conditioned, copied into the product)
    and calibration images of low contrast (0.45 + 0.1 U[0, 1))."""
    import lic
    from oracle import lic_oracle as LO
    torch.manual_seed(seed)
    ref = LO.Cheng2020Anchor(N=N).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name.endswith("gamma"):
                c = p.shape[0]
                p.copy_(torch.sqrt(0.1 * torch.eye(c) + 0.01 * torch.rand(c, c, generator=g) + 2.0 ** -36))
            elif p.dim() == 4 and "entropy_bottleneck" not in name:
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 2 * (3.0 / p[0].numel()) ** 0.5)
        # the last synthesis layer is tamed so that x_hat sits about 0.5 with a contrast of the order of sqrt(C2): with the low-contrast
        # calibration images of these tests every contrast-structure mean stays clearly positive, and the relu of MS-SSIM never cuts
        ref.g_s[7][0].weight.mul_(0.01)
        ref.g_s[7][0].bias.fill_(0.5)
    ref.context_prediction.mask.fill_(1.0)                     # the wrapper bypasses the mask
    prod = lic.Cheng2020Anchor(N=N).eval()
    sd = ref.state_dict()
    with torch.no_grad():
        for k, v in prod.state_dict().items():
            v.copy_(sd[k])
    return ref, prod, g


def _low_contrast(n, g):
    return 0.45 + 0.1 * torch.rand(n, 3, 192, 192, generator=g)


def test_rate_distortion_loss_ms_ssim_gradients(oracle64):
    """RateDistortionLoss(metric='ms-ssim') on a toy Cheng2020 output: lambda * (1 - MS-SSIM) + bpp with gradients to x_hat and every
    likelihood tensor, against float64 autograd of the same formula on the oracle's ms_ssim."""
    from losses.losses import RateDistortionLoss
    MO = oracle64
    _, prod, g = _toy_cheng()
    x = _low_contrast(2, g)
    with torch.no_grad():
        out = prod.cuda()(x.cuda())
    x_hat = out["x_hat"].detach().clamp(0, 1).requires_grad_(True)
    liks = {k: v.detach().requires_grad_(True) for k, v in out["likelihoods"].items()}
    lmbda = 12.0
    res = RateDistortionLoss(lmbda=lmbda, metric="ms-ssim")({"x_hat": x_hat, "likelihoods": liks}, x.cuda())
    assert set(res) >= {"loss", "bpp_loss", "mse_loss", "ms_ssim_loss"} and res["mse_loss"].grad_fn is None
    res["loss"].backward()
    torch.cuda.synchronize()
    xh64 = x_hat.detach().cpu().double().requires_grad_(True)
    l64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in liks.items()}
    n_pix = x.shape[0] * x.shape[2] * x.shape[3]
    ref = lmbda * (1 - MO.ms_ssim(xh64, x.double())) + sum((-torch.log2(v)).sum() for v in l64.values()) / n_pix
    ref.backward()
    # the value is the fp32 evaluation kernels' (rdo_ssim_level, rdo_neg_log2_sum): a few 1e-6 of MS-SSIM, times lambda
    assert abs(float(res["loss"]) - float(ref.detach())) <= 1e-4 * abs(float(ref.detach()))
    assert _rel(x_hat.grad, xh64.grad) <= 1e-4, _rel(x_hat.grad, xh64.grad)
    for k in liks:
        assert _rel(liks[k].grad, l64[k].grad) <= 1e-5, k


def _unit_of(qnn, path):
    unit = qnn.model
    for part in path.split("."):
        unit = unit[int(part)] if part.isdigit() else getattr(unit, part)
    return unit


@pytest.mark.parametrize("where", ["g_a.1", "g_s.2", "h_a.0"])
def test_rd_ms_ssim_mode_matches_oracle(where):
    """loss_mode='rd' with metric='ms-ssim': task term = lambda * (1 - MS-SSIM(x_hat, x)) + bpp of the whole toy Cheng2020 with the
    unit's soft-quantised output substituted; engine (captured-graph iteration) against the oracle loop on the CPU."""
    from helpers import AQ, WQ
    from oracle import msssim_oracle as MO
    from oracle import rdo_oracle as O
    from oracle import lic_oracle as LO
    from oracle.cheng_units import schedule
    from quantization import QuantModel
    from quantization.engine import UnitEngine
    from quantization.recon import _unit_modules
    n_img, B, iters, lmbda = 6, 2, 6, 12.0
    ref, prod, g = _toy_cheng()
    cali = _low_contrast(n_img, g)
    qnn = QuantModel(prod.cuda(), WQ, AQ, is_cheng=True).cuda().eval()
    qnn.set_quant_state(False, False)
    sched = {n: (k, o, m) for n, k, o, m in schedule(ref)}
    kind, ops_o, ref_mod = sched[where]
    seq, pos = where.split(".")
    unit = getattr(qnn.model, seq)[int(pos)]
    store = {}
    h = ref_mod.register_forward_hook(lambda m, i, o: store.update(inp=i[0].detach().clone(), out=o.detach().clone()))
    with torch.no_grad():
        ref(cali)
    h.remove()
    inp, out = store["inp"], store["out"]
    if kind == "layer" and ops_o["layer"].act == "lrelu":
        out = torch.nn.functional.leaky_relu(out, 0.01)
    inp_q = inp + 1e-3 * torch.randn(inp.shape, generator=g)
    idx = np.stack([np.random.RandomState(i).permutation(n_img)[:B] for i in range(iters)])

    LO.STE_ROUND = True
    try:
        def task_fn(out_quant, ix):
            x = cali[ix]
            fused_act = kind == "layer" and ops_o["layer"].act == "lrelu"
            hook_mod = getattr(ref, seq)[int(pos) + 1] if fused_act else ref_mod
            hk = hook_mod.register_forward_hook(lambda m, i, o: out_quant)
            try:
                o = ref(x)
            finally:
                hk.remove()
            n_pix = x.shape[0] * x.shape[2] * x.shape[3]
            bpp = sum((-torch.log2(v)).sum() for v in o["likelihoods"].values()) / n_pix
            xh = torch.nn.functional.leaky_relu(o["x_hat"], 0.01)     # the wrapped model's output
            return lmbda * (1 - MO.ms_ssim(xh, x)) + bpp
        log = O.reconstruct_unit(kind, ops_o, inp_q, inp, out, iters=iters, batch_size=B, idx_stream=idx,
                                 mask_fn=lambda i, shape: O.qdrop_keep_mask_nhwc(SEED, i, shape, 0.5), input_prob=0.5, weight=0.01,
                                 b_range=(20, 2), warmup=0.2, task_fn=task_fn)
    finally:
        LO.STE_ROUND = False

    k, mods = _unit_modules(unit)
    assert k == kind
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()
    eng = UnitEngine(k, mods, nh(inp_q), nh(inp), nh(out), batch_size=B, iters=iters, weight=0.01, b_range=(20, 2), warmup=0.2,
                     input_prob=0.5, seed=SEED, idx_table=torch.from_numpy(idx),
                     rd=dict(model=qnn, unit=unit, cali=cali.cuda(), lmbda=lmbda, metric="ms-ssim"))
    eng.run()
    torch.cuda.synchronize()
    assert eng.rd_path == "graph"
    rec, task, rd_, _ = eng.logs_terms()
    np.testing.assert_allclose(rec.numpy(), np.array(log.rec), rtol=3e-4, atol=1e-7)
    np.testing.assert_allclose(task.numpy(), np.array(log.task), rtol=2e-3)
    np.testing.assert_allclose(rd_.numpy(), np.array(log.round), rtol=2e-4, atol=1e-7)
    flips = tot = 0
    for n_, op in ops_o.items():
        a_gpu = eng.alpha_of(n_).cpu()
        far = ((a_gpu - op.alpha).abs() > 2e-3).float().mean()
        assert float(far) < 2e-2, (n_, float(far))
        flips += int(((a_gpu >= 0) != (op.alpha >= 0)).sum())
        tot += a_gpu.numel()
    assert flips <= 0.01 * tot


def test_rd_ms_ssim_graph_and_host_paths_agree(monkeypatch):
    """The MS-SSIM task term on the captured-graph iteration and on the host-driven one (RDO_RD_GRAPH=0): the same alphas and losses
    up to float rounding."""
    from helpers import AQ, WQ
    from quantization import QuantModel
    from quantization.engine import UnitEngine
    from quantization.recon import _unit_modules
    n_img, B, iters, lmbda = 4, 2, 6, 12.0
    cali = _low_contrast(n_img, torch.Generator().manual_seed(44)).cuda()
    idx = torch.from_numpy(np.stack([np.random.RandomState(i).permutation(n_img)[:B] for i in range(iters)]))
    res = {}
    for mode in ("graph", "host"):
        qnn = QuantModel(_toy_cheng()[1].cuda(), WQ, AQ, is_cheng=True).cuda().eval()
        qnn.set_quant_state(False, False)
        unit = _unit_of(qnn, "g_s.2")
        store = {}
        h = unit.register_forward_hook(lambda m, i, o: store.update(inp=i[0].detach().clone(), out=o.detach().clone()))
        with torch.no_grad():
            qnn(cali)
        h.remove()
        nh = lambda t: t.permute(0, 2, 3, 1).contiguous()
        inp, out = nh(store["inp"]), nh(store["out"])
        inp_q = inp + 1e-3 * torch.randn(inp.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        monkeypatch.setenv("RDO_RD_GRAPH", "0" if mode == "host" else "1")
        k, mods = _unit_modules(unit)
        eng = UnitEngine(k, mods, inp_q, inp, out, batch_size=B, iters=iters, weight=0.01, b_range=(20, 2), warmup=0.2, input_prob=0.5,
                         seed=SEED, idx_table=idx, rd=dict(model=qnn, unit=unit, cali=cali, lmbda=lmbda, metric="ms-ssim"))
        eng.run()
        torch.cuda.synchronize()
        assert eng.rd_path == mode
        res[mode] = ({n: eng.alpha_of(n).clone() for n in eng.ops}, [t.clone() for t in eng.logs_terms()[:3]])
    # not bit for bit: rdo_ssim_level (the evaluation forward, unchanged) sums each plane's means with one atomic per workgroup, so
    # the MS-SSIM value and the gradient scale it feeds back differ in the last bits from run to run
    for n in res["graph"][0]:
        torch.testing.assert_close(res["host"][0][n], res["graph"][0][n], rtol=0, atol=1e-5, msg=n)
    for a, b in zip(res["host"][1], res["graph"][1]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=0)


def test_reconstruction_with_rd_ms_ssim_metric():
    """`args.loss_mode = 'rd', args.rd_metric = 'ms-ssim'` through layer_/block_reconstruction on a toy Cheng2020; an unknown
    rd_metric and crops too small for five MS-SSIM scales are refused up front."""
    from quantization import QuantModel, block_reconstruction, layer_reconstruction
    model = _toy_cheng()[1].cuda()
    cali = _low_contrast(4, torch.Generator().manual_seed(8)).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq, is_cheng=True).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:2])
    args = types.SimpleNamespace(lmbda=12.0, task_loss=2.0, arch="Cheng2020", loss_mode="rd", rd_metric="ms-ssim")
    kwargs = dict(cali_data=cali, batch_size=2, iters=4, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2), warmup=0.2,
                  act_quant=False, opt_mode="mse", config=None, args=args)
    blk, lay = qnn.model.g_a[1], qnn.model.h_a[0]
    eng_b = block_reconstruction(qnn, blk, "1", **kwargs)
    eng_l = layer_reconstruction(qnn, lay, "0", **kwargs)
    for eng in (eng_b, eng_l):
        assert eng.rd is not None and eng.rd["metric"] == "ms-ssim" and eng.plan_rd is not None
        rec, task, rd_, _ = eng.logs_terms()
        assert torch.isfinite(rec).all() and torch.isfinite(task).all() and float(task.min()) > 0
    assert blk.trained and lay.trained
    with pytest.raises(ValueError, match="ms-ssim"):
        layer_reconstruction(qnn, qnn.model.h_a[4], "4", **dict(kwargs, args=types.SimpleNamespace(
            lmbda=12.0, task_loss=2.0, loss_mode="rd", rd_metric="nope")))
    with pytest.raises(ValueError, match="160"):
        layer_reconstruction(qnn, qnn.model.h_a[4], "4", **dict(kwargs, cali_data=cali[..., :64, :64]))
