"""CPU checks of oracle/attention_oracle.py and oracle/rowops_oracle.py, the references tests/test_gpu_attention.py and
tests/test_gpu_swin_rowops.py hold the kernels of csrc/swin.hip to: the index-arithmetic reference equals the roll / window-partition
composition the older kernel test uses, its gradient equals float64 autograd through that composition, the float32 restatements stay within
one unit (the worst err / unit of every result is printed: these are the numbers the GPU bounds are 4 x of), and the LayerNorm / GELU
references equal torch.nn.functional in float64."""
import pytest
import torch
import torch.nn.functional as F

import attention_cases as AC
from oracle import attention_oracle as A
from oracle import rowops_oracle as R
from oracle import swin_oracle as S

F64 = torch.float64


def composition(qkv, table, g):
    """roll, window partition, softmax(q k^T scale + bias + mask) v, window reverse, roll back -> (out, probs [windows, heads, N, N], bias)"""
    B, H, W, C3 = qkv.shape
    C, heads, ws, shift, hd = g.C, g.heads, g.ws, g.shift, g.hd
    x = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift else qkv
    xw = x.view(B, H // ws, ws, W // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C3)
    B_, N, _ = xw.shape
    t = xw.reshape(B_, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * g.scale, t[1], t[2]
    attn = q @ k.transpose(-2, -1)
    bias = table[S.relative_position_index(ws).view(-1)].view(N, N, -1).permute(2, 0, 1)
    attn = attn + bias.unsqueeze(0)
    mask = S.shifted_window_mask(H, W, ws, shift)
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, heads, N, N) + mask.to(attn.dtype).unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    p = torch.softmax(attn, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(B_, N, C)
    o = o.view(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o, p, bias.contiguous()


SMALL = [(2, 8, 16, 8, 2, 8, 4),          # H == window with a shift, H != W, 64 tokens
         (1, 16, 8, 6, 2, 8, 1),          # shift 1
         (1, 8, 8, 8, 2, 8, 7),           # shift window - 1, one window per axis
         (1, 16, 16, 8, 2, 8, 0),
         (2, 12, 6, 8, 2, 6, 3),          # 36 tokens, W == window
         (1, 12, 18, 6, 3, 6, 5),
         (2, 8, 4, 6, 3, 4, 1),           # 16 tokens
         (1, 8, 12, 12, 3, 4, 3),
         (2, 4, 6, 4, 2, 2, 1),           # 4 tokens
         (2, 3, 2, 4, 2, 1, 0)]           # 1 token


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("geom", SMALL, ids=lambda c: "x".join(map(str, c)))
def test_index_arithmetic_reference_equals_the_roll_and_partition_composition(geom):
    g = A.Geom(*geom)
    gen = torch.Generator().manual_seed(sum(geom))
    qkv = (torch.randn(g.B, g.H, g.W, 3 * g.C, generator=gen, dtype=F64) * 1.5).requires_grad_(True)
    table = torch.randn((2 * g.ws - 1) ** 2, g.heads, generator=gen, dtype=F64)
    dout = torch.randn(g.B, g.H, g.W, g.C, generator=gen, dtype=F64)
    out_c, p_c, bias = composition(qkv, table, g)
    (grad_c,) = torch.autograd.grad(out_c, qkv, dout)
    ref = A.reference(g, qkv, bias, dout)
    assert _rel(ref["out"], out_c.detach()) < 1e-12
    assert _rel(ref["p"], p_c.detach()) < 1e-12
    assert _rel(ref["probs"], p_c.detach().permute(0, 2, 3, 1)) < 1e-12
    assert _rel(ref["dqkv"], grad_c) < 1e-12
    assert _rel(ref["dqkv_analytic"], grad_c) < 1e-12                         # the closed form the dqkv units are propagated through
    out_pv, _ = A.pv_reference(g, qkv, ref["probs"])
    assert _rel(out_pv, out_c.detach()) < 1e-12
    # the tables themselves: every pixel is exactly one token, and the regions are those of the composition's mask
    pix = A.token_pixels(g)
    assert sorted(pix.reshape(-1).tolist()) == list(range(g.B * g.H * g.W))
    mask = S.shifted_window_mask(g.H, g.W, g.ws, g.shift)
    if mask is not None:
        nW = mask.shape[0]
        assert torch.equal(A.mask_of(g).view(g.B, nW, g.N, g.N), mask.to(F64).unsqueeze(0).expand(g.B, -1, -1, -1))


@pytest.fixture(scope="module")
def ratios():
    return {}


@pytest.mark.parametrize("name", list(AC.PATH_CASES))
def test_float32_restatement_stays_within_its_units_on_trained_like_inputs(name, ratios):
    """worst err / unit of the float32 restatement for probs, out, pv and the three thirds of dqkv, printed per case (pytest -s); the
    references and the restatement are finite on the planted inputs, and the plants are what they claim to be"""
    g = A.Geom(*AC.PATH_CASES[name])
    qkv, bias, dout = AC.trained_like(g, seed=len(name) + g.C)
    ref = A.reference(g, qkv, bias, dout)
    r32 = A.restate32(g, qkv, bias, dout)
    for key in ("probs", "out", "dqkv", "u_probs", "u_out", "u_dqkv"):
        assert bool(torch.isfinite(ref[key]).all()), key
    for key in ("probs", "out", "dqkv"):
        assert bool(torch.isfinite(r32[key]).all()), key
    facts = AC.planted_rows(g, ref)
    if g.N >= 4:
        assert facts["one_hot_rows"] >= 1 and facts["tied_rows"] >= 1, facts
    if g.N >= 16 and g.heads >= 3:
        assert facts["max_abs_logit"] > 25, facts                              # the hot head's logits
    if g.windows >= 2 and g.heads >= 2:                                         # the all-zero window in the zero-bias head: uniform over each region
        p_last = ref["p"][-1, -1]
        reg = A.token_regions(g)[-1]
        size = (reg.unsqueeze(0) == reg.unsqueeze(1)).sum(1).to(F64)
        own = reg.unsqueeze(0) == reg.unsqueeze(1)
        assert float((p_last[own] - (1.0 / size).unsqueeze(1).expand(-1, g.N)[own]).abs().max()) < 1e-12
    if g.shift in (1, g.ws - 1) and g.ws > 2:                                   # the corner window holds a region of a single token
        reg = A.token_regions(g)[g.nwh * g.nww - 1]
        assert int(torch.bincount(reg).clamp_min(0)[torch.bincount(reg) > 0].min()) == 1
    pv_ref, pv_unit = A.pv_reference(g, qkv, r32["probs"])
    C = g.C
    got = {"probs": A.worst_ratio(r32["probs"], ref["probs"], ref["u_probs"], A.P_FLOOR),
           "out": A.worst_ratio(r32["out"], ref["out"], ref["u_out"]),
           "pv": A.worst_ratio(A.pv32(g, qkv, r32["probs"]), pv_ref, pv_unit),
           "dq": A.worst_ratio(r32["dqkv"][..., :C], ref["dqkv"][..., :C], ref["u_dqkv"][..., :C]),
           "dk": A.worst_ratio(r32["dqkv"][..., C:2 * C], ref["dqkv"][..., C:2 * C], ref["u_dqkv"][..., C:2 * C]),
           "dv": A.worst_ratio(r32["dqkv"][..., 2 * C:], ref["dqkv"][..., 2 * C:], ref["u_dqkv"][..., 2 * C:])}
    ratios[name] = got
    print(f"\n{name}: restatement err / unit " + "  ".join(f"{k} {v:.3f}" for k, v in got.items()) + f"  {facts}")
    # a unit is ONE rounding's worth; a sum of n terms rounds n - 1 times in the worst order, so no float32 evaluation of these
    # expressions needs more than max(N, hd) + 4 units.  Measured: the pv restatement, which adds a row's N terms one after the other
    # like its kernel, needs up to 12; the blocked matrix products of the other results about 1 (0.3 .. 1.1)
    for k, v in got.items():
        assert v <= max(g.N, g.hd) + 4, (name, k, v)


@pytest.mark.parametrize("rows,C", [(17, 4), (15, 7), (16, 65), (33, 192), (9, 320), (5, 512)])
def test_layer_norm_references_equal_torch_in_float64(rows, C):
    x, w, b, dy = AC.ln_inputs(rows, C, rows + C)
    x64 = x.to(F64).requires_grad_(True)
    w64 = w.to(F64).requires_grad_(True)
    y = F.layer_norm(x64, (C,), w64, b.to(F64), 1e-5)
    gx, gw = torch.autograd.grad(y, (x64, w64), dy.to(F64))
    f = R.layer_norm64(x, w, b)
    bw = R.layer_norm_bwd64(x, w, dy, nslabs=3)
    assert _rel(f["y"], y.detach()) < 1e-12
    assert _rel(bw["dx"], gx) < 1e-10                                        # (the constant row: dx is rounding noise of 1e-13 against 1e2)
    assert _rel(bw["dgamma"], gw) < 1e-12
    for order in ("wave64",) + (("group16",) if C % 4 == 0 else ()):
        ry = A.worst_ratio(R.layer_norm32(x, w, b, order=order)[0], f["y"], f["unit_y"])
        rdx = A.worst_ratio(R.layer_norm_bwd32(x, w, dy, order=order), bw["dx"], bw["unit_dx"])
        print(f"\nlayer_norm rows {rows} C {C} {order}: restatement err / unit  y {ry:.3f}  dx {rdx:.3f}")
        assert ry <= 1.0 and rdx <= 1.0
    assert bool((bw["bound_dgamma"] > 0).all()) and bool(torch.isfinite(bw["bound_dgamma"]).all())


def test_gelu_references_equal_torch_in_float64():
    v = AC.gelu_inputs(4099)
    v64 = v.to(F64).requires_grad_(True)
    y = F.gelu(v64)
    (gp,) = torch.autograd.grad(y.sum(), v64)
    y_ref, uy = R.gelu64(v)
    gp_ref, ug = R.gelu_grad64(v)
    # torch's float64 erf form cancels in the negative tail just as float32 does: it is held to ITS units (2^-53 in place of 2^-24;
    # 4 of them: the reference's erfc and torch's erf are both good to an ulp or two)
    assert A.worst_ratio(y.detach(), y_ref, uy * 2.0 ** -29 + 1e-300) <= 4.0
    assert A.worst_ratio(gp, gp_ref, ug * 2.0 ** -29 + 1e-300) <= 4.0
    ry = A.worst_ratio(R.gelu32(v), y_ref, uy)
    rg = A.worst_ratio(R.gelu_grad32(v), gp_ref, ug)
    print(f"\ngelu: restatement err / unit  gelu {ry:.3f}  gelu' {rg:.3f}")
    assert ry <= 1.0 and rg <= 1.0
    tail = v < -6
    assert bool((uy[tail] >= 0.5 * R.U * v[tail].abs().to(F64) * 0.99).all())   # absolute in u |v| where the value itself is 1e-10 and less
