"""Pins tests/wgrad_reference.py (the CPU reference of the fp32-input weight-gradient kernels) without a GPU:
  * `ref` is torch.nn.grad.conv2d_weight in float64 on every case of the table; the chunk / patch sums add up to the whole;
  * 'exact' family: max S < 2^24 and the float32 chain equals `ref` bit for bit;
  * admission of the bound: the reference's float32 products summed in two other orders (32-pixel blocks pairwise, then across blocks; chunk
    slabs sequentially, then the slabs) stay within 0.75 of `bound` with d = 0 on every 'randn' case -- a case that did not would be
    changed, not the bound;
  * the transposed-conv tables: the restated `tconv_phase` equals ops.TconvPhase (index tables are host-side: built on the CPU here), the
    fold of the phase conv's float64 gradient is the autograd dW of F.conv_transpose2d in both weight layouts."""
import numpy as np
import pytest
import torch

import wgrad_reference as R

U = R.U
NAMES = list(R.CASES)


def _ns_of(name):
    """slab counts to pin on the CPU: the given ones, and 3 for 'the library's own'"""
    kernel = R.CASES[name][9]
    if kernel.startswith("thincout"):
        B, H, W = R.CASES[name][:3]
        return [B * (H // 16) * (W // 16)]
    return sorted({3 if n is None else n for n in R.CASES[name][11]})


def test_table_covers_every_launch():
    kernels = {c[9] for c in R.CASES.values()}
    assert kernels == set(R.TAG_OF)
    for name, c in R.CASES.items():
        assert R.family_of(c[9]) in R.MAXNORM and (R.family_of(c[9]) == "h2" or R.family_of(c[9]) in R.D_OF), name


def test_chunks_partition_the_pixels():
    for M in (1, 25, 31, 32, 33, 36, 63, 72, 84, 240, 4096, 4128):
        for ns in (1, 2, 3, 5, 9, 28, 33, 64):
            for step in (8, 32):
                ch = R.chunks(M, ns, step)
                assert len(ch) == ns and ch[0][0] == 0 and ch[-1][1] == M
                assert all(a[1] == b[0] for a, b in zip(ch, ch[1:])) and all(m0 <= m1 for m0, m1 in ch)
                assert all(m0 % step == 0 or m0 == M for m0, _ in ch)
    assert R.chunks(36, 5, 8) == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 36)]
    assert R.chunks(72, 4) == [(0, 32), (32, 64), (64, 72), (72, 72)]
    p = R.thincout_patches(2, 16, 32)
    assert len(p) == 4 and int(p[1][0]) == 16 and int(p[2][0]) == 16 * 32 and torch.equal(torch.cat(p).sort().values, torch.arange(2 * 16 * 32))


@pytest.mark.parametrize("name", NAMES)
def test_ref_is_conv2d_weight_and_parts_add_up(name):
    B, H, W, Cin, Cout, K, s, p, sq, kernel, flags, _ = R.CASES[name]
    for family in R.FAMILIES:
        c = R.case(name, family)
        r, whole = c["ref"], c["ref"].part()
        x = c["x"].double().permute(0, 3, 1, 2)
        want = torch.nn.grad.conv2d_weight(x * x if sq else x, (Cout, Cin, K, K), c["dy"].double().permute(0, 3, 1, 2), stride=s, padding=p)
        want = want.permute(0, 2, 3, 1)
        scale = float(whole.S.max())
        assert float((whole.ref - want).abs().max()) <= 1e-13 * scale, (name, family)
        assert bool((whole.S >= whole.ref.abs() * (1 - 1e-12)).all())
        for ns in _ns_of(name):
            parts = [r.part(sel) for sel in R.slab_sets(name, ns)]
            assert float((sum(pt.ref for pt in parts) - whole.ref).abs().max()) <= 1e-13 * scale, (name, family, ns)
            assert float((sum(pt.S for pt in parts) - whole.S).abs().max()) <= 1e-13 * scale, (name, family, ns)
            for sel, pt in zip(R.slab_sets(name, ns), parts):
                if isinstance(sel, tuple) and sel[0] == sel[1]:
                    assert not bool(pt.ref.any()) and not bool(pt.S.any()) and pt.q == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_exact_family_is_exact_in_float32(name):
    r = R.case(name, "exact")["ref"]
    whole = r.part()
    assert float(whole.S.max()) < 2.0 ** 24, (name, float(whole.S.max()))
    frac0 = float((R.case(name, "exact")["x"] == 0).float().mean())
    assert 0.15 < frac0 < 0.35, (name, frac0)
    for sel in [None] + list(R.slab_sets(name, _ns_of(name)[-1])):
        pt = r.part(sel)
        assert pt.q == 0.0
        assert np.array_equal(r.chain32(sel).astype(np.float64), pt.ref.reshape(-1)[r.eidx].numpy()), name
        assert torch.equal(pt.ref.float().double(), pt.ref)


def _pairwise(v):
    """sum over axis 0 by halving (float32)"""
    while v.shape[0] > 1:
        if v.shape[0] % 2:
            v = np.concatenate([v, np.zeros_like(v[:1])])
        v = v[0::2] + v[1::2]
    return v[0]


@pytest.mark.parametrize("name", NAMES)
def test_randn_family_admits_the_bound(name):
    r = R.case(name, "randn")["ref"]
    whole = r.part()
    bnd = whole.bound(0).reshape(-1)[r.eidx].numpy()
    ref = whole.ref.reshape(-1)[r.eidx].numpy()
    P = r.products32()
    assert P.dtype == np.float32
    # 32-pixel blocks pairwise, then across blocks pairwise
    blocks = np.stack([_pairwise(P[i:i + 32]) for i in range(0, P.shape[0], 32)])
    a = _pairwise(blocks).astype(np.float64)
    # chunk slabs sequentially, then the slabs sequentially
    ns = _ns_of(name)[-1]
    b = np.zeros(P.shape[1], np.float32)
    for sel in R.slab_sets(name, ns):
        Ps = r.products32(sel)
        if Ps.shape[0]:
            b = b + np.cumsum(Ps, axis=0, dtype=np.float32)[-1]
    b = b.astype(np.float64)
    worst = max(float(np.max(np.abs(v - ref) / bnd)) for v in (a, b))
    print(f"  [{name}] q {whole.q:.2f}  other orders / bound {worst:.3f}")
    assert whole.q > 0 and worst <= 0.75, (name, whole.q, worst)
    # the slabs admit their own bounds too
    for sel in R.slab_sets(name, ns):
        pt = r.part(sel)
        Ps = r.products32(sel)
        if Ps.shape[0] == 0:
            continue
        v = _pairwise(Ps).astype(np.float64)
        w = float(np.max(np.abs(v - pt.ref.reshape(-1)[r.eidx].numpy()) / pt.bound(0).reshape(-1)[r.eidx].numpy().clip(1e-300)))
        assert w <= 0.75, (name, sel if isinstance(sel, tuple) else "patch", pt.q, w)


def test_scaled_channels_defeat_the_max_norm():
    """the 'randn' family: an error of the whole max-norm allowance in an element of the small corner is thousands of its bounds"""
    pt = R.case("f64v_tiles_2x3", "randn")["ref"].part()
    small = pt.bound(0)[0, :, :, 0].max()
    assert 3e-6 * float(pt.ref.abs().max()) > 1e3 * float(small)


# ---- transposed conv ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", R.TCONV_GEOMETRIES)
@pytest.mark.parametrize("flipped", [True, False])
def test_tconv_phase_is_the_library_table(geom, flipped):
    from hipops import ops
    K, s, p = geom
    lib, own = ops.TconvPhase(K, s, p, flipped, "cpu"), R.tconv_phase(K, s, p, flipped)
    assert (lib.pad, lib.Kp, lib.S2) == (own["pad"], own["Kp"], own["S2"])
    assert lib.inv.tolist() == own["inv"]
    assert sorted(set(own["inv"])) == sorted(own["inv"])                               # a gather: no phase element feeds two taps


@pytest.mark.parametrize("name", list(R.TCONV_CASES))
def test_tconv_fold_of_the_phase_gradient_is_autograd(name):
    K, s, p, op, flipped, ns = R.TCONV_CASES[name]
    Cout = R.TCONV_SHAPE[4]
    for family in R.FAMILIES:
        c = R.tconv_case(name, family)
        whole = c["ref"].part()
        got = R.fold(whole.ref, c["ph"], Cout, K)
        assert tuple(got.shape) == tuple(c["dw"].shape)
        assert float((got - c["dw"]).abs().max()) <= 1e-13 * float(whole.S.max()), (name, family)
        parts = torch.stack([c["ref"].part(sel).ref for sel in R.chunks(c["ref"].M, ns)])
        assert float((R.fold(parts, c["ph"], Cout, K).sum(0) - c["dw"]).abs().max()) <= 1e-13 * float(whole.S.max())
        if family == "exact":
            assert float(whole.S.max()) < 2.0 ** 24 and whole.q == 0.0
    # the other layout is the flipped one
    other = R.tconv_dw64(c["x"], c["dy"], K, s, p, op, not flipped)
    assert torch.equal(other.flip(1, 2), c["dw"])
