"""Static per-channel activation quantisers on the GPU: the one-launch kernel against the dynamic kernel (bit for bit on the tensor it
was calibrated on), exact merging of observed ranges, clamping outside a frozen range, batch independence, the range search's error
sums against a float64 restatement, the quantiser / block surface, and the calibration flow of a toy Cheng2020 in static mode (with
the default, dynamic, flow unmoved)."""
import io
import math
import types

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

SHAPES = [(1, 192, 128, 96), (2, 1280, 5, 7), (1, 3, 33, 17), (4, 64, 64, 64), (1, 6, 1, 1)]


def _nhwc_input(shape, const_channel=True):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) * 3 + 0.5
    if const_channel:
        x[:, min(1, shape[1] - 1)] = 0.75
    return x.permute(0, 2, 3, 1).contiguous()


def _unaligned(x):
    """the same values behind a data pointer that is 4 bytes past a 16-byte boundary"""
    buf = torch.empty(x.numel() + 1, device=x.device, dtype=x.dtype)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _observed(ops, x, n_bits):
    rng = ops.act_range_init(x.shape[-1], x.device)
    dyn = ops.actquant_observe(x, rng, n_bits=n_bits)
    return rng, dyn


def _static_ref(x, lo, hi, n_bits):
    """fp32 CPU restatement of the static expression, x [..., C]"""
    R = float(2 ** n_bits - 1)
    rng = torch.clamp(hi - lo, min=1e-6)
    return torch.round(torch.clamp((x - lo) / rng, 0, 1) * R) / R * rng + lo


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n_bits", [4, 8, 10, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_static_equals_dynamic_on_the_tensor_it_was_calibrated_on(shape, n_bits):
    from hipops import ops
    x = _nhwc_input(shape).cuda()
    for xs in (x, _unaligned(x)):
        dyn = ops.actquant_perchannel(xs, n_bits=n_bits)
        rng, seen = _observed(ops, xs, n_bits)
        assert torch.equal(seen, dyn)                                   # while observing: what the dynamic quantiser returns
        C = shape[1]
        flat = x.reshape(-1, C).cpu()
        assert torch.equal(rng[:C].cpu(), flat.amin(0)) and torch.equal(rng[C:].cpu(), flat.amax(0))
        st = ops.actquant_static(xs, rng, n_bits=n_bits)
        assert torch.equal(st, dyn)                                     # no tolerance: the same expression on the same numbers
        assert torch.equal(ops.actquant_static(xs, rng, n_bits=n_bits), st)


def test_observed_ranges_merge_exactly():
    from hipops import ops
    g = torch.Generator().manual_seed(77)
    for C in (24, 6):
        batches = [torch.randn(b, 9, 11, C, generator=g) * (1 + b) + 0.1 * b for b in (1, 3, 2, 5)]
        rng = ops.act_range_init(C, "cuda")
        assert bool(torch.isinf(rng).all()) and bool((rng[:C] > 0).all()) and bool((rng[C:] < 0).all())
        for b in batches:
            out = ops.actquant_observe(b.cuda(), rng)
            assert torch.equal(out, ops.actquant_perchannel(b.cuda()))
        flat = torch.cat([b.reshape(-1, C) for b in batches])
        assert torch.equal(rng[:C].cpu(), flat.amin(0)) and torch.equal(rng[C:].cpu(), flat.amax(0))
    with pytest.raises(ValueError):
        ops.actquant_observe(batches[0].cuda(), ops.act_range_init(C + 1, "cuda"))


@pytest.mark.parametrize("n_bits", [6, 10, 16])
def test_clamping_outside_a_frozen_range(n_bits):
    from hipops import ops
    g = torch.Generator().manual_seed(n_bits)
    for shape in ((2, 6, 7, 24), (3, 5, 9, 7)):                          # vector and scalar path
        C = shape[-1]
        x = torch.randn(*shape, generator=g) * 3
        lo = -1.5 - 0.05 * torch.arange(C, dtype=torch.float32)
        hi = 1.0 + 0.03 * torch.arange(C, dtype=torch.float32)
        got = ops.actquant_static(x.cuda(), torch.cat([lo, hi]).cuda(), n_bits=n_bits).cpu()
        below, above = x < lo, x > hi
        assert int(below.sum()) > 10 and int(above.sum()) > 10
        assert torch.equal(got[below], lo.expand_as(x)[below])
        top = (hi - lo) + lo                                             # fl(fl(hi - lo) + lo), fp32
        assert torch.equal(got[above], top.expand_as(x)[above])
        inside = ~(below | above)
        ref = _static_ref(x, lo, hi, n_bits)
        diff = (got - ref).abs()
        step = ((hi - lo) / (2 ** n_bits - 1)).expand_as(x)
        frac = float((diff[inside] > 1e-6).float().mean())
        worst = float((diff / step)[inside].max())
        print(f"clamping n_bits={n_bits} shape={shape}: inside {int(inside.sum())}, >1e-6: {frac:.3e}, worst/step: {worst:.6f}")
        # a value within fp32 rounding of a grid boundary may land one level apart
        assert frac < 5e-3 and worst <= 1 + 1e-4


def test_static_is_batch_independent_and_works_in_place():
    from hipops import ops
    for shape in ((4, 16, 16, 192), (3, 7, 5, 6)):
        g = torch.Generator().manual_seed(sum(shape))
        x = (torch.randn(*shape, generator=g) * 2).cuda()
        C = shape[-1]
        rng = torch.cat([x.reshape(-1, C).amin(0) * 0.8, x.reshape(-1, C).amax(0) * 0.9]).contiguous()
        full = ops.actquant_static(x, rng)
        for i in range(shape[0]):
            assert torch.equal(full[i:i + 1], ops.actquant_static(x[i:i + 1].contiguous(), rng))
        y = x.clone()
        assert ops.actquant_static(y, rng, out=y) is y and torch.equal(y, full)
        with pytest.raises(ValueError):
            ops.actquant_static(x, rng[:-2])
        # ... unlike the dynamic quantiser, whose grid depends on what shares the batch
        assert not torch.equal(ops.actquant_perchannel(x)[0:1], ops.actquant_perchannel(x[0:1].contiguous()))


def _search_input(npix, C):
    g = torch.Generator().manual_seed(npix + C)
    z = torch.randn(npix, C, generator=g)
    x = z ** 3 * (0.25 + torch.arange(C) % 7) * 0.3
    x = torch.where(x < 0, x * 0.01, x)
    x[:, 1] = 0.75
    return x.float().contiguous()


def _search_ref64(x, lo, hi, n_bits):
    """float64 restatement: err[c][k] = sum_p (x - Q_k(x))^2 on the candidates lo * s_k | hi * s_k (fp32 numbers, as a frozen range is)"""
    R = float(2 ** n_bits - 1)
    xd = x.double()
    out = torch.zeros(x.shape[1], 10, dtype=torch.float64)
    for k in range(10):
        s = torch.tensor(1.0 - 0.05 * k, dtype=torch.float32)
        lk, hk = (lo * s).double(), (hi * s).double()
        rng = torch.clamp(hk - lk, min=1e-6)
        q = torch.round(torch.clamp((xd - lk) / rng, 0, 1) * R) / R * rng + lk
        out[:, k] = ((xd - q) ** 2).sum(0).cpu()
    return out


def _rel_err(got, ref):
    nz = ref != 0
    assert bool((got[~nz] == 0).all())
    return float(((got[nz] - ref[nz]).abs() / ref[nz]).max())


@pytest.mark.parametrize("n_bits", [4, 6, 8])
@pytest.mark.parametrize("npix,C", [(16384, 192), (1122, 24), (1024, 6), (35, 1280)])
def test_search_sums_match_float64(npix, C, n_bits):
    """Tolerance 1e-4 relative: the terms are non-negative, so an fp32 sum whose serial chains hold at most 1024 terms, plus the tree,
    is within about (1024 + 20) * 2^-24 = 6.2e-5 of the exact sum."""
    from hipops import ops
    x = _search_input(npix, C)
    lo, hi = x.amin(0), x.amax(0)
    ref = _search_ref64(x, lo, hi, n_bits)
    xc, rng = x.cuda(), torch.cat([lo, hi]).cuda()
    err = torch.zeros(C, 10, device="cuda")
    ops.actquant_search(xc, rng, err, n_bits=n_bits)
    again = torch.zeros(C, 10, device="cuda")
    ops.actquant_search(xc, rng, again, n_bits=n_bits)
    assert torch.equal(err, again)                                       # fixed reduction order: bit-identical from launch to launch
    got = err.cpu().double()
    worst = _rel_err(got, ref)
    print(f"search npix={npix} C={C} n_bits={n_bits}: largest relative error {worst:.3e}")
    assert worst <= 1e-4
    # arg-min: on every channel whose best and second-best float64 scores are more than 1e-4 (relative) apart
    srt = ref.sort(dim=1).values
    clear = (srt[:, 1] - srt[:, 0]) > 1e-4 * srt[:, 1]
    assert float((~clear).float().mean()) <= 0.10
    assert torch.equal(got.argmin(1)[clear], ref.argmin(1)[clear])
    print(f"   arg-mins: {sorted(set(ref.argmin(1).tolist()))}, channels left out: {int((~clear).sum())}")
    # accumulation: two batches (an uneven split, the second one behind an unaligned pointer) against one call on their concatenation
    cut = (npix * 3) // 8 + 1
    two = torch.zeros(C, 10, device="cuda")
    ops.actquant_search(xc[:cut].contiguous(), rng, two, n_bits=n_bits)
    ops.actquant_search(_unaligned(xc[cut:].contiguous()), rng, two, n_bits=n_bits)
    assert _rel_err(two.cpu().double(), got) <= 1e-4
    assert _rel_err(two.cpu().double(), ref) <= 1e-4


def test_search_closes_long_chains():
    """More than 1024 pixels per thread (one channel: all 256 lanes of all 256 workgroups walk the pixels): the running sums are closed
    every 1024 terms.  The float64 reference of this one is evaluated by torch on the device: 72 M values (288 MB in fp32) and their
    float64 temporaries, about 3 GB of device memory for the duration of the test."""
    from hipops import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    npix = 256 * 256 * 1100
    x = (torch.rand(npix, 1, generator=g, device="cuda") ** 2).contiguous()
    lo, hi = x.amin(0), x.amax(0)
    ref = _search_ref64(x, lo, hi, 8)
    err = torch.zeros(1, 10, device="cuda")
    ops.actquant_search(x, torch.cat([lo, hi]), err, n_bits=8)
    worst = _rel_err(err.cpu().double(), ref)
    print(f"search {npix} x 1: largest relative error {worst:.3e}")
    assert worst <= 1e-4


def test_evaluation_metrics_are_summed_in_a_fixed_order():
    """PSNR / bpp of `evaluate_images` go through the ordered reductions: the same bits on every call (the atomic forms, which the
    calibration losses keep, add their per-workgroup sums in the order the workgroups finish), and the same value as the atomic forms
    up to that reordering."""
    from hipops import ops
    from losses.losses import compute_bpp, compute_psnr
    g = torch.Generator().manual_seed(21)
    a, b = torch.rand(1, 3, 256, 384, generator=g), torch.rand(1, 3, 256, 384, generator=g)
    lik = {"y": torch.rand(1, 192, 16, 24, generator=g).clamp_min(1e-3), "z": torch.rand(1, 128, 4, 6, generator=g).clamp_min(1e-3)}
    ac, bc = a.cuda(), b.cuda()
    out = {"x_hat": ac, "likelihoods": {k: v.cuda() for k, v in lik.items()}}
    psnr, bpp = {compute_psnr(ac, bc) for _ in range(50)}, {compute_bpp(out) for _ in range(50)}
    assert len(psnr) == 1 and len(bpp) == 1
    mse64 = float(((a.double() - b.double()) ** 2).mean())
    bpp64 = float(sum(-torch.log2(v.double()).sum() for v in lik.values()) / (256 * 384))
    assert abs(psnr.pop() - (-10 * math.log10(mse64))) < 1e-4 and abs(bpp.pop() - bpp64) < 1e-5 * bpp64
    one = ops.sq_diff_sum_ordered(ac.reshape(-1), bc.reshape(-1), 1.0 / a.numel())
    assert abs(float(one) - float(ops.sq_diff_sum(ac.reshape(-1), bc.reshape(-1), 1.0 / a.numel()))) < 1e-5 * mse64
    acc = ops.sq_diff_sum_ordered(ac.reshape(-1), bc.reshape(-1), 1.0 / a.numel(), out=one.clone())      # out is accumulated into
    assert abs(float(acc) - 2 * float(one)) < 1e-6 * mse64


# ----------------------------------------------------------------------------- quantiser and block surface
def test_static_quantiser_through_4d_3d_2d_and_whole_tensor():
    from quantization.quantizer import ActQuantizer, UniformAffineQuantizer
    g = torch.Generator().manual_seed(3)
    cases = [(torch.randn(2, 12, 6, 7, generator=g) * 3, 12), (torch.randn(2, 9, 8, generator=g), 8), (torch.randn(5, 20, generator=g), 20),
             (torch.randn(40, generator=g), 1)]
    for bits in (8, 10):
        for x, C in cases:
            x = x.cuda()
            q = UniformAffineQuantizer(n_bits=8, channel_wise=True, scale_method="max", act=True, dynamic_bits=bits, act_mode="static")
            with pytest.raises(RuntimeError):
                q(x, True)                                               # not frozen: no silent fall-back to the dynamic grid
            q.act_observe()
            dyn = ActQuantizer(x, bits)
            assert torch.equal(q(x, True), dyn)
            q.act_freeze()
            assert q.act_frozen() and q.act_range[0].numel() == 2 * C and q.act_range[0].is_cuda
            out = q(x, True)
            assert out.shape == x.shape and torch.equal(out, dyn)
            if x.dim() > 1:
                with pytest.raises(ValueError):
                    q(torch.cat([x, x], dim=1 if x.dim() in (2, 4) else -1), True)     # channel count differs from the range
            # L2 search on the same tensor: the range shrinks inside the observed one
            q2 = UniformAffineQuantizer(act=True, dynamic_bits=bits, act_mode="static")
            q2.act_observe(); q2(x, True); q2.act_search()
            assert torch.equal(q2(x, True), dyn)                         # the max-range static output goes downstream
            q2.act_freeze()
            r, r0 = q2.act_range[0], q.act_range[0]
            assert bool((r[:C] >= r0[:C]).all()) and bool((r[C:] <= r0[C:]).all()) and bool((r[:C] <= r[C:]).all())
            q.cpu()
            assert not q.act_range[0].is_cuda


def test_attention_wrapper_keeps_two_ranges():
    import lic
    from helpers import AQ, WQ
    from quantization import BaseQuantBlock, QuantModule
    from quantization.quant_block import QuantRSTB, QuantWindowAttention
    from quantization.recon import calibrate_act_ranges
    torch.manual_seed(4)
    dim, heads = 16, 2
    unit = QuantRSTB(lic.RSTB(dim=dim, input_resolution=(8, 8), depth=2, num_heads=heads, window_size=4, mlp_ratio=2.0), WQ, AQ).cuda().eval()
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.trained = True
            m.act_quantizer.set_act_mode("static")
    x = torch.randn(3, dim, 8, 8).cuda()
    unit.set_quant_state(True, False)
    calibrate_act_ranges(unit, x, "max", batch=2)
    assert not unit.use_act_quant and not any(m.use_act_quant for m in unit.modules() if isinstance(m, (QuantModule, BaseQuantBlock)))
    attns = [m for m in unit.modules() if isinstance(m, QuantWindowAttention)]
    assert len(attns) == 2
    for a in attns:
        q = a.act_quantizer
        assert q.act_frozen() and sorted(q.act_range) == [0, 1]
        assert q.act_range[0].numel() == 2 * heads and q.act_range[1].numel() == 2 * dim
        lo, hi = q.act_range[0][:heads], q.act_range[0][heads:]
        assert bool((lo >= 0).all()) and bool((hi <= 1 + 1e-6).all())    # probabilities
    for m in unit.modules():
        if isinstance(m, (QuantModule, BaseQuantBlock)):
            m.use_weight_quant = m.use_act_quant = True
    with torch.no_grad():
        full, again = unit(x, (8, 8)), unit(x, (8, 8))
    assert bool(torch.isfinite(full).all()) and torch.equal(full, again)
    unit.residual_group.blocks[0].attn.act_quantizer.act_range.pop(1)             # a place without a range raises, no fall-back
    with pytest.raises(RuntimeError):
        unit(x, (8, 8))


# ----------------------------------------------------------------------------- calibration flow (toy Cheng2020)
def _toy(**extra):
    import lic
    from quantization import QuantModel
    torch.manual_seed(1005)
    N, n_img, B, iters = 8, 4, 2, 6
    model = lic.Cheng2020Anchor(N=N).cuda().eval()
    g = torch.Generator().manual_seed(13)
    cali = torch.rand(n_img, 3, 64, 64, generator=g).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq, is_cheng=True).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:B])
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Cheng2020", **extra)
    kwargs = dict(cali_data=cali, batch_size=B, iters=iters, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2),
                  warmup=0.2, act_quant=True, opt_mode="mse", config=None, args=args)
    qnn.set_quant_state(True, True)
    qnn.model.g_s[-1][0].set_quant_state(True, False)
    return qnn, cali, list(qnn.model.g_a.named_children()), kwargs, g, N


def _expect_ranges(unit, N):
    """every quantiser of a calibrated Cheng2020 block that the W8A8 forward applies is frozen with the right channel count; the
    others have no range"""
    from quantization import BaseQuantBlock, QuantModule
    sites = {"rbws": [0, 1], "rbu": [0, 1], "rb": [0, 1, 2]}[unit.unit_kind]
    q = unit.act_quantizer
    assert q.act_frozen() and sorted(q.act_range) == sites and all(q.act_range[s].numel() == 2 * N for s in sites)
    n = 0
    for m in unit.modules():
        if isinstance(m, QuantModule):
            q = m.act_quantizer
            if m.disable_act_quant or m.is_ps:
                assert q.act_range == {} and not q.act_frozen()
            else:
                c = m.org_weight.shape[0]
                assert q.act_frozen() and sorted(q.act_range) == [0] and q.act_range[0].numel() == 2 * c
                lo, hi = q.act_range[0][:c], q.act_range[0][c:]
                assert bool(torch.isfinite(q.act_range[0]).all()) and bool((lo <= hi).all())
                n += 1
        elif isinstance(m, BaseQuantBlock):
            assert m is unit
    assert n >= (1 if unit.unit_kind != "rb" else 0)             # (a ResidualBlock without a skip conv applies only its block-level points)


def _cache_pass_forward(units, x):
    """the cache passes (utils.set_mode) re-enable only the QuantModules of trained units: the block-level quantisers stay off"""
    for _, u in units:
        u.set_quant_state(True, True)
        u.use_act_quant = False
    with torch.no_grad():
        for _, u in units:
            x = u(x)
    return x


def test_main2_flow_with_static_activation_ranges():
    from quantization import BaseQuantBlock, QuantModule, block_reconstruction, layer_reconstruction
    from quantization.export import activation_state
    from quantization.utils import save_inp_oup_data
    from test_datasets import evaluate_images
    qnn, cali, units, kwargs, g, N = _toy(act_mode="static", timing=[])
    for name, u in units[:2]:
        block_reconstruction(qnn, u, name, **kwargs)
    for _, u in units[:2]:
        _expect_ranges(u, N)
    calibrated = {id(m) for _, u in units[:2] for m in u.modules()}
    rest = [m for m in qnn.modules() if isinstance(m, (QuantModule, BaseQuantBlock)) and id(m) not in calibrated]
    assert rest and all(m.act_quantizer.act_mode == "static" and m.act_quantizer.act_range == {} for m in rest)
    assert all("act_s" in t and t["act_s"] >= 0 for t in kwargs["args"].timing)
    # the third unit's quantised input, cached at batch 4, = the two calibrated blocks at batch 4 in the cache pass's state
    (inp_q, inp_fp), out_fp = save_inp_oup_data(qnn, units[2][1], cali, asym=True, act_quant=True, batch_size=4, input_prob=True)
    manual = _cache_pass_forward(units[:2], cali)
    torch.testing.assert_close(inp_q, manual, rtol=0, atol=0)
    assert float((inp_q - inp_fp).abs().max()) > 0

    def recon_rest(m: nn.Module, skip):
        for name, module in m.named_children():
            if module in skip:
                continue
            if isinstance(module, QuantModule):
                layer_reconstruction(qnn, module, name, **kwargs)
            elif isinstance(module, BaseQuantBlock):
                block_reconstruction(qnn, module, name, **kwargs)
            else:
                recon_rest(module, skip)
    recon_rest(qnn, {units[0][1], units[1][1]})
    mods = [m for m in qnn.modules() if isinstance(m, QuantModule) and m.org_weight is not None]
    assert all(m.trained and hasattr(m.weight_quantizer, "alpha") for m in mods)
    qnn.set_quant_state(True, True)
    qnn.model.g_s[-1][0].set_quant_state(True, False)
    imgs = [torch.rand(1, 3, 64, 64, generator=g)]
    psnr, bpp = evaluate_images(qnn.eval(), imgs, p=64)
    assert math.isfinite(psnr) and math.isfinite(bpp)
    st = activation_state(qnn)
    assert len(st) >= 20 and list(st) == list(qnn.act_ranges())
    assert all(v["lo"].numel() == v["channels"] == v["hi"].numel() and v["n_bits"] == 8 and bool((v["lo"] <= v["hi"]).all()) for v in st.values())
    buf = io.BytesIO()
    torch.save(qnn, buf)
    buf.seek(0)
    qnn2 = torch.load(buf, weights_only=False)
    st2 = activation_state(qnn2)
    assert list(st2) == list(st)
    for k in st:
        assert torch.equal(st[k]["lo"], st2[k]["lo"]) and torch.equal(st[k]["hi"], st2[k]["hi"]) and st[k]["n_bits"] == st2[k]["n_bits"]
    qnn2.set_quant_state(True, True)
    qnn2.model.g_s[-1][0].set_quant_state(True, False)
    with torch.no_grad():
        a, b = qnn(imgs[0].cuda()), qnn2(imgs[0].cuda())
    assert torch.equal(a["x_hat"], b["x_hat"]) and all(torch.equal(a["likelihoods"][k], b["likelihoods"][k]) for k in a["likelihoods"])
    psnr2, bpp2 = evaluate_images(qnn2.eval(), imgs, p=64)
    print(f"static W8A8 toy: psnr {psnr!r} / {psnr2!r}, bpp {bpp!r} / {bpp2!r}")
    assert (psnr2, bpp2) == (psnr, bpp)


def test_l2_ranges_lie_inside_the_max_ranges():
    from quantization import block_reconstruction
    from quantization.recon import calibrate_act_ranges
    from quantization.utils import save_inp_oup_data
    qnn, cali, units, kwargs, g, N = _toy(act_mode="static", act_range="l2")
    shrunk = total = one_sided = 0
    for name, u in units[:2]:
        (inp_q, _), _ = save_inp_oup_data(qnn, u, cali, asym=True, act_quant=True, batch_size=4, input_prob=True)
        block_reconstruction(qnn, u, name, **kwargs)
        _expect_ranges(u, N)
        quants = [m.act_quantizer for m in u.modules() if hasattr(m, "act_quantizer")]
        l2 = [{s: r.clone() for s, r in q.act_range.items()} for q in quants]
        calibrate_act_ranges(u, inp_q, "max", batch=4)                   # the max ranges over the same inputs
        for q, mine in zip(quants, l2):
            assert sorted(mine) == sorted(q.act_range)
            for s, r in mine.items():
                c = r.numel() // 2
                mx = q.act_range[s]
                assert bool((r[:c] >= mx[:c]).all()) and bool((r[c:] <= mx[c:]).all()) and bool((r[:c] <= r[c:]).all())
                shrunk += int(((r[:c] > mx[:c]) | (r[c:] < mx[c:])).sum())
                total += c
                one_sided += int(((mx[:c] > 0) | (mx[c:] < 0)).sum())     # channels whose frozen grid is the clipped candidate
            q.act_range = mine                                           # (put the l2 grid back for the next unit's cache)
    print(f"l2: {shrunk} of {total} channels shrank; {one_sided} of {total} do not straddle zero")


def _recon_all(qnn, kwargs):
    from quantization import BaseQuantBlock, QuantModule, block_reconstruction, layer_reconstruction
    visited = []

    def walk(m: nn.Module):
        for name, module in m.named_children():
            if isinstance(module, QuantModule):
                visited.append((name, module))
                layer_reconstruction(qnn, module, name, **kwargs)
            elif isinstance(module, BaseQuantBlock):
                visited.append((name, module))
                block_reconstruction(qnn, module, name, **kwargs)
            else:
                walk(module)
    walk(qnn)
    return visited


def test_static_schedule_on_toy_cheng2020_attn_w10a10():
    """BASELINE config 3 in miniature (Cheng2020-attn, W10A10) with static grids.  The reference's "last layer" rule trains every LAYER
    unit whose name holds a '7' without activation quantisation -- g_a[7] and convs inside the attention blocks here -- yet the cache
    passes of the units behind them and the W8A8 evaluation apply those quantisers: they must have been given a range too."""
    import lic
    from quantization import BaseQuantBlock, QuantModel, QuantModule
    from test_datasets import evaluate_images
    torch.manual_seed(1005)
    N, n_img, B, iters = 8, 8, 4, 6
    model = lic.Cheng2020Attention(N=N).cuda().eval()
    g = torch.Generator().manual_seed(9)
    cali = torch.rand(n_img, 3, 64, 64, generator=g).cuda()
    imgs = [torch.rand(1, 3, 64, 64, generator=g)]
    wq = {"n_bits": 10, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 10, "channel_wise": True, "scale_method": "max", "leaf_param": False, "dynamic_bits": 10}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq, is_cheng=True).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:B])
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Cheng2020", act_mode="static")
    kwargs = dict(cali_data=cali, batch_size=B, iters=iters, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2),
                  warmup=0.2, act_quant=True, opt_mode="mse", config=None, args=args)
    qnn.set_quant_state(True, True)
    qnn.model.g_s[-1][0].set_quant_state(True, False)
    visited = _recon_all(qnn, kwargs)                                   # every later unit's cache pass runs the calibrated prefix W10A10
    sevens = [m for name, m in visited if isinstance(m, QuantModule) and "7" in name and not m.disable_act_quant and not m.is_ps]
    assert len(sevens) >= 1 and isinstance(qnn.model.g_a[7], QuantModule) and qnn.model.g_a[7] in sevens
    for m in qnn.modules():
        if isinstance(m, QuantModule):
            q = m.act_quantizer
            if m.disable_act_quant or m.is_ps:
                assert q.act_range == {}
            else:
                assert q.act_frozen() and q.act_range[0].numel() == 2 * m.org_weight.shape[0] and q.dynamic_bits == 10
        elif isinstance(m, BaseQuantBlock):
            assert m.act_quantizer.act_frozen()
    qnn.set_quant_state(True, True)
    qnn.model.g_s[-1][0].set_quant_state(True, False)
    psnr, bpp = evaluate_images(qnn.eval(), imgs, p=64)
    assert math.isfinite(psnr) and math.isfinite(bpp)
    with torch.no_grad():
        full = qnn(cali)["x_hat"]
    assert bool(torch.isfinite(full).all())


def test_static_schedule_on_first_units_of_toy_lu2022():
    """A conv unit and a Swin (RSTB) unit of the Lu2022 coder in static mode, through the cache building of the unit behind them: the
    attention wrappers' two ranges, the nested blocks' quantisers and the conv's are all fixed, and the W8A8 prefix runs in batches."""
    import lic
    from quantization import BaseQuantBlock, QuantModel, QuantModule, block_reconstruction, layer_reconstruction
    from quantization.quant_block import QuantRSTB, QuantWindowAttention
    from quantization.utils import save_inp_oup_data
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
    n_img, B, iters = 8, 4, 6
    cali = torch.rand(n_img, 3, 64, 64, generator=g).cuda()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:B])
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Lu2022", act_mode="static")
    kwargs = dict(cali_data=cali, batch_size=B, iters=iters, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2),
                  warmup=0.2, act_quant=True, opt_mode="mse", config=None, args=args)
    units = [(n, m) for n, m in qnn.model.named_children() if isinstance(m, (QuantModule, BaseQuantBlock))]
    assert [n for n, _ in units[:3]] == ["g_a0", "g_a1", "g_a2"] and isinstance(units[1][1], QuantRSTB)
    for name, u in units[:2]:
        (layer_reconstruction if isinstance(u, QuantModule) else block_reconstruction)(qnn, u, name, **kwargs)
    assert units[0][1].act_quantizer.act_frozen()
    inner = [m for m in units[1][1].modules() if isinstance(m, (QuantModule, BaseQuantBlock))]
    attns = [m for m in inner if isinstance(m, QuantWindowAttention)]
    assert attns and all(sorted(a.act_quantizer.act_range) == [0, 1] and a.act_quantizer.act_range[0].numel() == 2 * a.num_heads
                         and a.act_quantizer.act_range[1].numel() == 2 * a.dim for a in attns)
    from quantization.quant_block import QuantBasicLayer
    for m in inner:                      # (a QuantBasicLayer only chains its blocks: its own quantiser is never applied)
        never = (isinstance(m, QuantModule) and m.disable_act_quant) or isinstance(m, QuantBasicLayer)
        assert m.act_quantizer.act_range == {} if never else m.act_quantizer.act_frozen(), type(m).__name__
    (inp_q, inp_fp), out_fp = save_inp_oup_data(qnn, units[2][1], cali, asym=True, act_quant=True, batch_size=4, input_prob=True)
    assert inp_q.shape == inp_fp.shape and bool(torch.isfinite(inp_q).all()) and float((inp_q - inp_fp).abs().max()) > 0


def test_default_flow_did_not_move():
    """`act_mode` absent and act_mode='dynamic' are the same flow: bit-identical alphas for the first two blocks and the identical
    third-unit cache (batch 1, as dynamic grids require)."""
    from quantization import QuantModule, block_reconstruction
    from quantization.utils import save_inp_oup_data
    runs = []
    for extra in ({}, {"act_mode": "dynamic"}):
        qnn, cali, units, kwargs, g, N = _toy(**extra)
        if extra:
            qnn.set_act_mode("static")          # the args decide in both directions: a model left static is switched back
        for name, u in units[:2]:
            block_reconstruction(qnn, u, name, **kwargs)
        (inp_q, inp_fp), out_fp = save_inp_oup_data(qnn, units[2][1], cali, asym=True, act_quant=True, batch_size=1, input_prob=True)
        alphas = [m.weight_quantizer.alpha.detach().clone() for _, u in units[:2] for m in u.modules()
                  if isinstance(m, QuantModule) and m.org_weight is not None]
        quants = [m.act_quantizer for m in qnn.modules() if hasattr(m, "act_quantizer")]
        assert all(q.act_mode == "dynamic" and q.act_range == {} for q in quants)
        runs.append((alphas, inp_q, inp_fp))
    (a0, q0, f0), (a1, q1, f1) = runs
    assert len(a0) == len(a1) > 0 and all(torch.equal(x, y) for x, y in zip(a0, a1))
    assert torch.equal(q0, q1) and torch.equal(f0, f1)
    assert float((q0 - f0).abs().max()) > 0
