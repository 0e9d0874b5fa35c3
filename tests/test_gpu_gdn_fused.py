"""rdo_gdn_fwd_bwd -- the GDN / IGDN block of a unit (norm pool, loss tail, gamma'^T GEMM, dx) in one launch -- against the chain of
the four launches it replaces: linear_h2(square_input) -> loss_gdn_bwd -> linear_h2 -> gdn_bwd_dx_h2.  The tail launches of the chain (loss_gdn_bwd, gdn_bwd_dx_h2) are pinned to float64 formulas with stated error
bounds by test_gpu_tail_parity.py (reference: tail_reference.py, itself pinned to the oracle's f_gdn autograd by test_tail_reference.py),
linear_h2 to fp64 by test_gpu_h2.py and test_gpu_swin_kernels.py; the fused launch runs the same device
functions in the same order, so every fp32 output and the int16 planes must equal the chain's BIT FOR BIT.  Only the loss log is
summed in another order (float atomics): rtol 1e-5, the bar of test_loss_gdn_bwd_equals_unfused_chain."""
import pytest
import torch

pytestmark = pytest.mark.gpu
C = 192
N_TGT = 6


@pytest.fixture(scope="module")
def ops():
    from hipops import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from hipops import _lib
    return _lib


def _weights(ops, g):
    gam = 0.1 * torch.eye(C, device="cuda") + 0.002 * torch.rand(C, C, device="cuda", generator=g)
    scale = ops.pow2_scale(gam.abs().max())
    fwd = ops.split_h2_linear(gam.contiguous(), scale=scale)
    bwd = ops.split_h2_linear(gam.t().contiguous(), scale=scale)
    beta = 0.5 + torch.rand(C, device="cuda", generator=g)
    return fwd, bwd, beta


def _inputs(ops, B, H, W, seed, decades=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    fwd, bwd, beta = _weights(ops, g)
    c = torch.randn(B, H, W, C, device="cuda", generator=g)
    res = torch.randn(B, H, W, C, device="cuda", generator=g)
    tgt = torch.randn(N_TGT, H, W, C, device="cuda", generator=g)
    rows = torch.randperm(N_TGT, generator=torch.Generator().manual_seed(seed))
    assert B <= N_TGT
    idx = torch.stack([rows[:B], rows.flip(0)[:B]]).to(torch.int32).cuda()    # two rows of distinct targets; the launch must read row `it` = 1
    it = torch.ones(1, dtype=torch.int32, device="cuda")
    if decades:
        # token magnitudes over eight decades, some tokens all zero (the `plain` branch of the scale rule)
        mag = torch.logspace(-6, 2, B * H * W, device="cuda")[torch.randperm(B * H * W, device="cuda", generator=g)]
        c = c * mag.view(B, H, W, 1)
        c.view(-1, C)[::7] = 0.0
    return dict(c=c, res=res, tgt=tgt, idx=idx, it=it, fwd=fwd, bwd=bwd, beta=beta, g=g)


def _chain(ops, d, inverse, res, want_out, dx_scale):
    """the four launches; returns out, dout, t, dx, dx planes, log"""
    c = d["c"]
    norm = ops.linear_h2(c.view(-1, C), d["fwd"], d["beta"], square_input=True).view(c.shape)
    out = torch.empty_like(c) if want_out else None
    dout, t = torch.empty_like(c), torch.empty_like(c)
    log = torch.zeros(2, 32, device="cuda")
    ops.loss_gdn_bwd(c, norm, res, d["tgt"], d["idx"], d["it"], 2.0, inverse, log, dout, t=t, out=out)
    acc = ops.linear_h2(t.view(-1, C), d["bwd"], None).view(c.shape)
    dx = torch.empty_like(c)
    pl = ops.h2_empty(c.shape, "cuda", dx_scale)
    ops.gdn_bwd_dx_h2(dout, c, norm, acc, inverse, dx=dx, dx_planes=pl)
    return out, dout, t, dx, pl, log


def _targets_near_outputs(ops, d, inverse):
    """targets 1e-2 from the outputs (the decades case): the gradients then follow the token magnitudes"""
    c = d["c"]
    norm = ops.linear_h2(c.view(-1, C), d["fwd"], d["beta"], square_input=True).view(c.shape)
    o = c * (norm.sqrt() if inverse else norm.rsqrt()) + d["res"]
    tgt = d["tgt"]
    for b in range(c.shape[0]):
        tgt[int(d["idx"][1, b])] = o[b] * (1 + 1e-2 * torch.randn(o[b].shape, device="cuda", generator=d["g"]))


def _run_fused(ops, d, inverse, res, want_out, want_dout, dx_form, dx_scale):
    c = d["c"]
    out = torch.full_like(c, float("nan")) if want_out else None
    dout = torch.full_like(c, float("nan")) if want_dout else None
    t = torch.full_like(c, float("nan"))
    dx = torch.full_like(c, float("nan")) if dx_form in ("f32", "both") else None
    pl = ops.h2_empty(c.shape, "cuda", dx_scale) if dx_form in ("planes", "both") else None
    log = torch.zeros(2, 32, device="cuda")
    pub = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ops.iter_bind_publish(pub)
    ops.gdn_fwd_bwd(c, d["fwd"], d["bwd"], d["beta"], res, d["tgt"], d["idx"], d["it"], 2.0, inverse, log, t, grad_out=dout, out=out, dx=dx,
                    dx_planes=pl)
    assert not ops.iter_bind_publish(None)                             # the launch consumed the binding
    return out, dout, t, dx, pl, log, pub


def _check(ops, d, inverse, with_res=True, want_out=True, want_dout=True, dx_form="both"):
    res = d["res"] if with_res else None
    ops.h2_overflow(reset=True)
    # the chain first, on fp32 only, to learn the magnitude of dx: the planes' scale comes from the reference, as the engine's comes from a probe
    r_out, r_dout, r_t, r_dx, _, _ = _chain(ops, d, inverse, res, want_out, 1.0)
    ops.h2_overflow(reset=True)
    amax = r_dx[torch.isfinite(r_dx)].abs().max()
    scale = ops.pow2_scale(amax) if float(amax) > 0 else 1.0
    r_out, r_dout, r_t, r_dx, r_pl, r_log = _chain(ops, d, inverse, res, want_out, scale)
    out, dout, t, dx, pl, log, pub = _run_fused(ops, d, inverse, res, want_out, want_dout, dx_form, scale)
    torch.cuda.synchronize()
    assert torch.equal(t, r_t)
    if want_out:
        assert torch.equal(out, r_out)
    if want_dout:
        assert torch.equal(dout, r_dout)
    if dx is not None:
        assert torch.equal(dx, r_dx)
    if pl is not None:
        assert torch.equal(pl.t, r_pl.t)
    assert float(log[0].abs().sum()) == 0.0                             # row `it` = 1 of the log, nothing else
    torch.testing.assert_close(log[1].sum(), r_log[1].sum(), rtol=1e-5, atol=0)
    assert int(pub) == int(d["it"])
    assert not ops.h2_overflow(reset=True)
    return dict(t=t, dx=dx, pl=pl, scale=scale)


@pytest.mark.parametrize("inverse", [False, True])
def test_one_tile(ops, inverse):
    _check(ops, _inputs(ops, 1, 8, 8, 11 + inverse), inverse)


@pytest.mark.parametrize("inverse", [False, True])
def test_three_tiles_three_images(ops, inverse):
    """the target row changes from tile to tile inside the launch"""
    _check(ops, _inputs(ops, 3, 8, 8, 21 + inverse), inverse)


@pytest.mark.parametrize("inverse", [False, True])
def test_smallest_map_of_the_workload(ops, inverse):
    """B = 4, 32 x 32: 64 tiles, fewer than CUs"""
    _check(ops, _inputs(ops, 4, 32, 32, 31 + inverse), inverse)


def _ragged_shape():
    """tiles = B * H (W = 64): not a multiple of the launcher's workgroup count (one per CU), at least one workgroup walks three
    tiles and another two"""
    wgs = torch.cuda.get_device_properties(0).multi_processor_count
    B = 3
    H = (2 * wgs + 1 + B - 1) // B
    while (B * H) % wgs == 0 or B * H <= 2 * wgs:
        H += 1
    assert B * H > 2 * wgs and (B * H) % wgs != 0 and B * H < 3 * wgs
    return B, H, 64


@pytest.mark.parametrize("inverse", [False, True])
def test_ragged_multi_tile_and_repeatable(ops, inverse):
    B, H, W = _ragged_shape()
    d = _inputs(ops, B, H, W, 41 + inverse)
    first = _check(ops, d, inverse)
    for _ in range(2):                                                  # a late load is a race: three runs, identical bits
        _, _, t, dx, pl, _, _ = _run_fused(ops, d, inverse, d["res"], False, False, "both", first["scale"])
        assert torch.equal(t, first["t"]) and torch.equal(dx, first["dx"]) and torch.equal(pl.t, first["pl"].t)


@pytest.mark.parametrize("inverse", [False, True])
def test_token_magnitudes_over_decades(ops, inverse):
    d = _inputs(ops, 3, 16, 16, 51 + inverse, decades=True)
    _targets_near_outputs(ops, d, inverse)
    _check(ops, d, inverse)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("with_res,want_dout,want_out,dx_form", [
    (True, True, False, "f32"), (True, False, True, "planes"), (False, True, True, "both"), (False, False, False, "planes"),
    (True, False, False, "both"), (False, True, False, "f32")])
def test_output_forms(ops, inverse, with_res, want_dout, want_out, dx_form):
    _check(ops, _inputs(ops, 2, 8, 16, 61 + inverse), inverse, with_res=with_res, want_out=want_out, want_dout=want_dout, dx_form=dx_form)


@pytest.mark.parametrize("inverse", [False, True])
def test_dx_plane_overflow_flag(ops, inverse):
    """a dx-plane scale that is too large raises the sticky flag, and only then (`_check` asserts the flag stays down at a fitting scale)"""
    d = _inputs(ops, 1, 8, 8, 71 + inverse)
    fit = _check(ops, d, inverse)
    amax = float(fit["dx"].abs().max())
    too_large = 2.0 ** 17 / 2.0 ** torch.tensor(amax).log2().floor().item()       # amax * scale >= 2^17 > 65504
    ops.h2_overflow(reset=True)
    _run_fused(ops, d, inverse, d["res"], False, False, "planes", too_large)
    assert ops.h2_overflow(reset=True)


def test_supported_shapes(ops):
    assert ops.gdn_fwd_bwd_supported(64, 192) and ops.gdn_fwd_bwd_supported(65536, 192)
    assert not ops.gdn_fwd_bwd_supported(96, 192) and not ops.gdn_fwd_bwd_supported(64, 128) and not ops.gdn_fwd_bwd_supported(0, 192)


# ---- engine: the switch changes the plan and nothing else ---------------------------------------------------------------------------
def _block(kind):
    import lic
    torch.manual_seed(3)
    blk = lic.ResidualBlockWithStride(192, 192, stride=2) if kind == "rbws" else lic.ResidualBlockUpsample(192, 192, 2)
    return blk.cuda().eval()


def _unit(kind):
    from quantization.quant_block import QuantRBU, QuantRBWS
    from quantization.recon import _unit_modules
    WQ = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    unit = (QuantRBWS if kind == "rbws" else QuantRBU)(_block(kind), WQ, dict(WQ, leaf_param=False)).cuda()
    k, mods = _unit_modules(unit)
    assert k == kind
    return mods


@pytest.mark.parametrize("kind", ["rbws", "rbu"])
def test_engine_switch_changes_the_plan_only(kind, monkeypatch):
    """an RBWS and an RBU unit at N = 192 on 16^2 inputs, 6 iterations: RDO_GDN_FUSED = 1 and 0 train the same alphas bit for bit, and
    `linear_h2_gdn` is in the plan exactly when the switch is on.  (The 8^2 output of the RBWS is below the engine's default row
    threshold for the token-matrix GEMMs: lowered here, for both settings.)"""
    from quantization.engine import UnitEngine
    monkeypatch.setattr(UnitEngine, "LIN_GDN_MIN_ROWS", 64)
    n_img, B, iters = 6, 4, 6
    g = torch.Generator().manual_seed(9)
    x = torch.rand(n_img, 192, 16, 16, generator=g).cuda()
    xq = x + 1e-2 * torch.randn(x.shape, generator=g).cuda()
    idx = torch.stack([torch.randperm(n_img, generator=g)[:B] for _ in range(iters)])
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        out = _block(kind)(x)                                           # the unit's full-precision output, its target: ONE tensor for both runs
    alphas, tags = {}, {}
    for sw in ("1", "0"):
        monkeypatch.setenv("RDO_GDN_FUSED", sw)
        mods = _unit(kind)
        eng = UnitEngine(kind, mods, nh(xq), nh(x), nh(out), batch_size=B, iters=iters, seed=1005, idx_table=idx)
        eng.run()
        torch.cuda.synchronize()
        tags[sw] = [t for t, _, _ in eng.plan_a.op_info()]
        alphas[sw] = {n: eng.alpha_of(n).clone() for n in eng.ops}
    assert tags["1"].count("linear_h2_gdn") == 1 and "loss_gdn_bwd" not in tags["1"] and "gdn_bwd_dx" not in tags["1"]
    assert "linear_h2" not in tags["1"]
    assert "linear_h2_gdn" not in tags["0"] and tags["0"].count("linear_h2") == 2 and "loss_gdn_bwd" in tags["0"]
    for n in alphas["1"]:
        assert torch.equal(alphas["1"][n], alphas["0"][n]), n
