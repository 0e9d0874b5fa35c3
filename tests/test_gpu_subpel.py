"""The r = 2 pixel shuffle of a sub-pixel conv (and its inverse in the backward pass) in the stores of the kernels that write the tensor
(include/rdo_ptq_subpel.h) against the launches it replaces: every conv output is the same K-ordered sum whatever row its weights sit in
and wherever it is stored, the splits use the same scales, so fp32 tensors and int16 planes must equal the shuffle launches' BIT FOR
BIT -- and an engine with the switch on must train the same alphas as one with it off.

Shapes: the plane kernels take a conv from 192 workgroup tiles x K splits on (rdo_conv2d_fwd_h2_supported), so a 16 x 16 map needs
B = 4 and 768 output channels to be on the plane path at all (the sub-pixel conv of Cheng2020's g_s.1: the K-split form); the other
cases are the smallest that reach the direct 256 x 192, 256 x 64 and 256 x 48 tiles, with 32 or 64 input channels where the gate allows it."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from hipops import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from hipops import _lib
    return _lib


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _group_planes(ops, planes, shape):
    """activation planes [2][C/16][pixels][16] of a tensor of `shape` with its channels regrouped: channel g * C/4 + c <- channel 4 c + g"""
    Cc = shape[-1]
    p = ops.group_rows(Cc).cuda()
    t = planes.t.permute(0, 2, 1, 3).reshape(2, -1, Cc)[:, :, p]
    return t.reshape(2, -1, Cc // 16, 16).permute(0, 2, 1, 3).contiguous()


# ---- shuffle store -------------------------------------------------------------------------------------------------------------------
# (x shape, Cout): split over K + second pass | direct 256 x 64 | direct 256 x 48 | direct 256 x 192 (odd batch)
SHUFFLE_CASES = [((4, 16, 16, 192), 768), ((2, 64, 64, 32), 768), ((4, 32, 32, 64), 768), ((3, 64, 64, 32), 768)]


@pytest.mark.parametrize("lrelu", [False, True])
@pytest.mark.parametrize("xs,cout", SHUFFLE_CASES)
def test_shuffle_store(ops, L, xs, cout, lrelu):
    g = _gen(5)
    B, H, W, Cin = xs
    w4 = (cout, 3, 3, Cin)
    assert ops.conv_h2_px_supported(xs, w4, 1, 1, L.STORE_SHUFFLE)
    x = torch.randn(xs, device="cuda", generator=g)
    w = torch.randn(w4, device="cuda", generator=g) / (3.0 * Cin ** 0.5)
    bias = torch.randn(cout, device="cuda", generator=g)
    p = ops.group_rows(cout).cuda()
    xp = ops.split_h2(x)
    wl = ops.split_h2_conv(w)
    wg = ops.split_h2_conv(w, scale=wl.scale, row_groups=4)
    assert torch.equal(wg.t, ops.split_h2_conv(w[p].contiguous(), scale=wl.scale).t)         # the set-up-time producer of group-ordered planes
    epi = L.EPI_LRELU if lrelu else L.EPI_NONE
    ops.h2_overflow(reset=True)
    sp = torch.empty(B, H, W, cout, device="cuda")
    ops.conv2d_fwd_h2(xp, xs, w4, wl, bias, 1, 1, epilogue=epi, out=sp)
    scale = ops.pow2_scale(sp.abs().max())
    ref = torch.empty(B, 2 * H, 2 * W, cout // 4, device="cuda")
    ref_p = ops.h2_empty(ref.shape, "cuda", scale)
    ops.pixel_shuffle_h2(sp, out=ref, out_planes=ref_p)
    out = torch.full_like(ref, float("nan"))
    out_p = ops.h2_empty(ref.shape, "cuda", scale)
    out_p.t.fill_(-1)
    ops.conv2d_fwd_h2_px(xp, xs, w4, wg, L.STORE_SHUFFLE, bias[p].contiguous(), 1, 1, epilogue=epi, out=out, out_planes=out_p)
    torch.cuda.synchronize()
    assert torch.equal(ref, torch.nn.functional.pixel_shuffle(sp.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))    # (the reference launch itself)
    assert torch.equal(out, ref)
    assert torch.equal(out_p.t, ref_p.t)
    assert not ops.h2_overflow(reset=True)
    # planes only (the form the engine asks for h1)
    only_p = ops.h2_empty(ref.shape, "cuda", scale)
    ops.conv2d_fwd_h2_px(xp, xs, w4, wg, L.STORE_SHUFFLE, bias[p].contiguous(), 1, 1, epilogue=epi, out_planes=only_p)
    assert torch.equal(only_p.t, ref_p.t)


# ---- unshuffle store -----------------------------------------------------------------------------------------------------------------
# (dy shape, Cout): split over K + second pass | direct 256 x 48 | direct 256 x 64 | direct 256 x 192 (odd batch)
UNSHUFFLE_CASES = [((4, 32, 32, 192), 192), ((4, 64, 64, 64), 192), ((5, 64, 64, 64), 128), ((3, 128, 128, 32), 192)]


@pytest.mark.parametrize("xs,cout", UNSHUFFLE_CASES)
def test_unshuffle_store(ops, L, xs, cout):
    """the dgrad of the 3 x 3 conv with its LeakyReLU mask read off the planes of h1 at the big-grid pixel"""
    g = _gen(7)
    B, H, W, Cin = xs
    w4 = (cout, 3, 3, Cin)
    assert ops.conv_h2_px_supported(xs, w4, 1, 1, L.STORE_UNSHUFFLE)
    dy = torch.randn(xs, device="cuda", generator=g)
    w = torch.randn(w4, device="cuda", generator=g) / (3.0 * Cin ** 0.5)
    h1 = torch.randn(B, H, W, cout, device="cuda", generator=g)
    dyp, wp, h1p = ops.split_h2(dy), ops.split_h2_conv(w), ops.split_h2(h1)
    ops.h2_overflow(reset=True)
    dh1 = torch.empty(B, H, W, cout, device="cuda")
    ops.conv2d_fwd_h2(dyp, xs, w4, wp, None, 1, 1, epilogue=L.EPI_LRELU_BWD, aux_planes=h1p, out=dh1)
    scale = ops.pow2_scale(dh1.abs().max())
    rshape = (B, H // 2, W // 2, 4 * cout)
    ref = torch.empty(rshape, device="cuda")
    ref_p = ops.h2_empty(rshape, "cuda", scale)
    ops.pixel_unshuffle2(dh1, ref, out_planes=ref_p)
    out = torch.full_like(ref, float("nan"))
    out_p = ops.h2_empty(rshape, "cuda", scale)
    out_p.t.fill_(-1)
    ops.conv2d_fwd_h2_px(dyp, xs, w4, wp, L.STORE_UNSHUFFLE, None, 1, 1, epilogue=L.EPI_LRELU_BWD, aux_planes=h1p, out=out, out_planes=out_p)
    torch.cuda.synchronize()
    p = ops.group_rows(4 * cout).cuda()
    assert torch.equal(out, ref[..., p])
    assert torch.equal(out_p.t, _group_planes(ops, ref_p, rshape))
    assert not ops.h2_overflow(reset=True)


# ---- GDN block: dL/dout as the planes of its unshuffle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("shape", [(1, 16, 16, 192), (3, 8, 24, 192)])
def test_gdn_dup_planes(ops, inverse, shape):
    g = _gen(11)
    B, H, W, Cc = shape
    gam = 0.1 * torch.eye(Cc, device="cuda") + 0.002 * torch.rand(Cc, Cc, device="cuda", generator=g)
    ws = ops.pow2_scale(gam.abs().max())
    fwd, bwd = ops.split_h2_linear(gam.contiguous(), scale=ws), ops.split_h2_linear(gam.t().contiguous(), scale=ws)
    beta = 0.5 + torch.rand(Cc, device="cuda", generator=g)
    c = torch.randn(shape, device="cuda", generator=g)
    res = torch.randn(shape, device="cuda", generator=g)
    tgt = torch.randn((5, H, W, Cc), device="cuda", generator=g)
    idx = torch.tensor([[0, 1, 2], [4, 2, 3]], dtype=torch.int32, device="cuda")[:, :B].contiguous()
    it = torch.ones(1, dtype=torch.int32, device="cuda")

    def run(px, dup_scale=1.0, dx_scale=1.0):
        o = dict(out=torch.full_like(c, float("nan")), t=torch.full_like(c, float("nan")), dx=torch.full_like(c, float("nan")),
                 dxp=ops.h2_empty(shape, "cuda", dx_scale), log=torch.zeros(2, 32, device="cuda"))
        if px:
            o["dup"] = ops.h2_empty((B, H // 2, W // 2, 4 * Cc), "cuda", dup_scale)
            o["dup"].t.fill_(-1)
            ops.gdn_fwd_bwd_px(c, fwd, bwd, beta, res, tgt, idx, it, 2.0, inverse, o["log"], o["t"], o["dup"], out=o["out"], dx=o["dx"],
                               dx_planes=o["dxp"])
        else:
            o["dout"] = torch.full_like(c, float("nan"))
            ops.gdn_fwd_bwd(c, fwd, bwd, beta, res, tgt, idx, it, 2.0, inverse, o["log"], o["t"], grad_out=o["dout"], out=o["out"], dx=o["dx"],
                            dx_planes=o["dxp"])
        return o

    ops.h2_overflow(reset=True)
    r = run(False)
    ops.h2_overflow(reset=True)
    s_dup, s_dx = ops.pow2_scale(r["dout"].abs().max()), ops.pow2_scale(r["dx"].abs().max())
    r, f = run(False, dx_scale=s_dx), run(True, s_dup, s_dx)
    rshape = (B, H // 2, W // 2, 4 * Cc)
    ref_p = ops.h2_empty(rshape, "cuda", s_dup)
    ops.pixel_unshuffle2(r["dout"], None, out_planes=ref_p)
    torch.cuda.synchronize()
    assert torch.equal(f["dup"].t, _group_planes(ops, ref_p, rshape))
    for k in ("out", "t", "dx"):
        assert torch.equal(f[k], r[k]), k
    assert torch.equal(f["dxp"].t, r["dxp"].t)
    assert float(f["log"][0].abs().sum()) == 0.0
    torch.testing.assert_close(f["log"][1].sum(), r["log"][1].sum(), rtol=1e-5, atol=0)
    assert not ops.h2_overflow(reset=True)
    # dup planes raise their own overflow words when their scale is outgrown
    flag = torch.zeros(2, dtype=torch.int32, device="cuda")
    big = ops.h2_empty(rshape, "cuda", s_dup * 2.0 ** 12, flag=flag)
    ops.gdn_fwd_bwd_px(c, fwd, bwd, beta, res, tgt, idx, it, 2.0, inverse, torch.zeros(2, 32, device="cuda"), torch.empty_like(c), big)
    torch.cuda.synchronize()
    assert int(flag[0]) != 0 and not ops.h2_overflow(reset=True)


# ---- AdaRound step with the rows in 4 groups ------------------------------------------------------------------------------------------------
def _step_state(ops, w4, nsplit, seed):
    g = _gen(seed)
    w = torch.randn(w4, device="cuda", generator=g) * 0.1
    d = ops.ada_desc(w, 256)
    delta, zp = ops.uaq_init_minmax(w.view(w4[0], -1), 256)
    alpha = ops.adaround_init_alpha(d, w, delta)
    alpha = alpha + 0.3 * torch.randn(w4, device="cuda", generator=g)
    st = dict(d=d, w=w, delta=delta, zp=zp, alpha=alpha, m=1e-3 * torch.randn(w4, device="cuda", generator=g),
              v=1e-6 * torch.rand(w4, device="cuda", generator=g), slabs=1e-2 * torch.randn((nsplit,) + w4, device="cuda", generator=g))
    return st, ops.pow2_scale(float((delta * 256).max()))


def _step_item(ops, st, pscale, slabs):
    w = st["w"]
    return dict(d=st["d"], w=w, delta=st["delta"], zp=st["zp"], slabs=slabs.contiguous(), alpha=st["alpha"].clone(), m=st["m"].clone(),
                v=st["v"].clone(), wq=torch.full_like(w, float("nan")), wd=torch.full_like(w, float("nan")),
                wq_planes=ops.H2(torch.full((2,) + tuple(w.shape), -1, dtype=torch.int16, device="cuda"), pscale),
                wd_planes=ops.H2(torch.full((2,) + tuple(w.shape), -1, dtype=torch.int16, device="cuda"), pscale))


STEP_KEYS = ("alpha", "m", "v", "wq", "wd")


def _run_step(ops, items, counter, **kw):
    sched = ops.make_sched(5, 0.4, (20, 2), device="cuda")
    it = torch.full((1,), counter, dtype=torch.int32, device="cuda")
    log = torch.zeros(5, 32, device="cuda")
    ops.adaround_step_batch(items, 1.0, 0.01, sched, it, log, **kw)
    torch.cuda.synchronize()
    return log


@pytest.mark.parametrize("counter", [0, 2])                    # a warm-up row (no rounding term) and one with b = 14
def test_step_rows_in_groups(ops, counter):
    shapes = [((768, 3, 3, 32), 5), ((64, 1, 1, 16), 17)]
    states = [_step_state(ops, w4, ns, 21 + k) for k, (w4, ns) in enumerate(shapes)]
    plain = [_step_item(ops, st, ps, st["slabs"]) for st, ps in states]
    log_p = _run_step(ops, plain, counter)
    grouped = [_step_item(ops, st, ps, st["slabs"][:, ops.group_rows(st["w"].shape[0]).cuda()]) for st, ps in states]
    log_g = _run_step(ops, grouped, counter, row_groups=[4, 4])
    for a, b in zip(plain, grouped):
        for k in STEP_KEYS:
            assert torch.equal(a[k], b[k]), k
        assert torch.equal(a["wd_planes"].t, b["wd_planes"].t)
        co, kh, kw, ci = a["w"].shape
        p = ops.group_rows(co).cuda()
        frag = lambda pl: pl.t.view(2, ci // 16, kh, kw, co, 16)
        assert torch.equal(frag(b["wq_planes"]), frag(a["wq_planes"])[:, :, :, :, p])
        assert torch.equal(b["wq_planes"].t, ops.split_h2_conv(a["wq"], scale=a["wq_planes"].scale, row_groups=4).t)
    torch.testing.assert_close(log_g.sum(1), log_p.sum(1), rtol=1e-5, atol=0)
    # one flagged item beside a plain one in the same launch
    mixed = [_step_item(ops, states[0][0], states[0][1], states[0][0]["slabs"]),
             _step_item(ops, states[1][0], states[1][1], states[1][0]["slabs"][:, ops.group_rows(64).cuda()])]
    _run_step(ops, mixed, counter, row_groups=[0, 4])
    for k in STEP_KEYS:
        assert torch.equal(mixed[0][k], plain[0][k]) and torch.equal(mixed[1][k], plain[1][k]), k
    assert torch.equal(mixed[0]["wq_planes"].t, plain[0]["wq_planes"].t) and torch.equal(mixed[1]["wq_planes"].t, grouped[1]["wq_planes"].t)


def test_step_all_zero_groups_is_the_gather_launch(ops):
    """row_groups = 0 everywhere, with the next mini-batch riding on the launch: what rdo_adaround_step_batch_gather leaves, byte for byte"""
    st, ps = _step_state(ops, (768, 3, 3, 32), 5, 31)
    g = _gen(33)
    cq, cf = torch.randn(6, 8, 8, 32, device="cuda", generator=g), torch.randn(6, 8, 8, 32, device="cuda", generator=g)
    idx = torch.stack([torch.randperm(6, generator=torch.Generator().manual_seed(k))[:4] for k in range(5)]).to(torch.int32).cuda()
    outs = []
    for rg in (None, [0]):
        item = _step_item(ops, st, ps, st["slabs"])
        x = torch.full((4, 8, 8, 32), float("nan"), device="cuda")
        xp = ops.h2_empty(x.shape, "cuda", 16.0)
        xp.t.fill_(-1)
        shadow = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        gather = dict(cache_q=cq, cache_fp=cf, idx_table=idx, B=4, batch_offset=0, prob=0.5, seed=77, out=x, out_planes=xp)
        log = _run_step(ops, [item], 2, iter_shadow=shadow, gather=gather, row_groups=rg)
        outs.append([item[k] for k in STEP_KEYS] + [item["wq_planes"].t, item["wd_planes"].t, x, xp.t, shadow, log])
    for a, b in zip(outs[0][:-1], outs[1][:-1]):
        assert torch.equal(a, b)
    torch.testing.assert_close(outs[1][-1].sum(1), outs[0][-1].sum(1), rtol=1e-5, atol=0)      # (the round-loss log: float atomics)
    assert int(outs[1][-2]) == 3 and not bool(torch.isnan(outs[1][-4]).any())


# ---- engine: the switch changes the plan and nothing else --------------------------------------------------------------------------------
def _block():
    import lic
    torch.manual_seed(3)
    return lic.ResidualBlockUpsample(192, 192, 2).cuda().eval()


def _unit():
    from quantization.quant_block import QuantRBU
    from quantization.recon import _unit_modules
    WQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    k, mods = _unit_modules(QuantRBU(_block(), WQ, dict(WQ, leaf_param=False)).cuda())
    assert k == "rbu"
    return mods


@pytest.mark.parametrize("hw,iters", [(16, 6), (32, 4)])       # the K-split launches | the direct 256 x 48 tiles and a K-split dgrad... of g_s.1 / g_s.3
def test_engine_switch_changes_the_plan_only(hw, iters, monkeypatch):
    """an RBU unit at N = 192, B = 4: RDO_SUBPEL_FUSED = 1 and 0 train the same alphas bit for bit; the pixel (un)shuffle launches are in
    the plan exactly when the switch is off; the losses agree to the rounding of their sums"""
    from quantization.engine import UnitEngine
    n_img, B = 6, 4
    g = torch.Generator().manual_seed(9)
    x = torch.rand(n_img, 192, hw, hw, generator=g).cuda()
    xq = x + 1e-2 * torch.randn(x.shape, generator=g).cuda()
    idx = torch.stack([torch.randperm(n_img, generator=g)[:B] for _ in range(iters)])
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        out = _block()(x)
    alphas, tags, losses, bufs = {}, {}, {}, {}
    for sw in ("1", "0"):
        monkeypatch.setenv("RDO_SUBPEL_FUSED", sw)
        eng = UnitEngine("rbu", _unit(), nh(xq), nh(x), nh(out), batch_size=B, iters=iters, seed=1005, idx_table=idx)
        eng.run()
        torch.cuda.synchronize()
        tags[sw] = [t for t, _, _ in eng.plan_a.op_info()]
        alphas[sw] = {n: eng.alpha_of(n).clone() for n in eng.ops}
        losses[sw] = eng.logs()
        bufs[sw] = set(eng.t)
        assert eng.h2_restarts == 0
    shuf = lambda tl: [t for t in tl if "shuffle" in t]
    assert not shuf(tags["1"]) and len(shuf(tags["0"])) == 4
    assert len(tags["0"]) == len(tags["1"]) + 4
    assert tags["1"].count("linear_h2_gdn") == 1 and sum(t.startswith("conv_fwd_h2_halo") for t in tags["1"]) == 4
    assert not bufs["1"] & {"sp", "up", "dout", "dh1"} and {"sp", "up", "dout", "dh1"} <= bufs["0"]
    for n in alphas["1"]:
        assert torch.equal(alphas["1"][n], alphas["0"][n]), n
    for a, b in zip(losses["1"], losses["0"]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=0)
