"""The unit-tail kernels -- gather_qdrop, lp2_loss_grad, lp_loss_grad (csrc/elementwise.hip) and every entry of csrc/fused_tail.hip --
against tests/tail_reference.py (a CPU reference pinned to the oracle's float64 autograd by tests/test_tail_reference.py), at the shapes
where their work splits can go wrong.  The rest of the suite compares the one-launch forms (rdo_gdn_fwd_bwd, the conv with the tail in its
epilogue) with the chain of these launches; this file is where that chain meets a reference from outside the library.

What is compared how:
  * gather, lp2, loss_act_bwd (+ split-K), the pixel (un)shuffles: torch.equal with the reference (IEEE add / sub / mul / compare only,
    files built with -ffp-contract=off);
  * planes: bit-equal to tail_reference.h2_planes of the fp32 output of the same launch;
  * loss_gdn_bwd, gdn_bwd_dx(_h2): float64 within the per-element bounds of tail_reference.gdn_bounds / gdn_dx64 (derived there; the inputs
    are admitted by test_tail_reference.py: the fp32 CPU chain stays within 0.75 of them);
  * lp_loss_grad: float64 at the bar of test_lp_loss_kernel_matches_autograd (rtol 2e-5, atol 1e-7), exactly 0 where d == 0;
  * the loss log: every slot of row `it` against the float64 sum over the elements of the workgroups that add into it (the work split is
    restated in `_slots_cm` / `_slots_pix`), relative (D + 4) * 2^-24 with D the additions a term passes through, counted from the code
    beside each case: 2 inside the quad (lp_kernel: none), the thread's accumulator, 6 shuffle steps, 3 cross-wave adds, the atomics of the
    workgroups that share the slot.  The 4: the square, the two scalings, the rounded 1 / npix.  All terms are non-negative, so this is
    a bound.  Rows of other iterations and slots nobody adds into stay exactly 0.

Every output is prefilled with NaN and followed (planes: also preceded; the two planes are adjacent, what overruns the first lands in
the second and fails the bit compare) by 64 sentinel elements that must survive the launch.

Not covered: the loss kernels of fused_tail.hip past the default tail_grid of 1024 workgroups -- the forced tail_grid = 1 walks the same
grid-stride loop at small shapes."""
import math

import pytest
import torch

import tail_reference as R

pytestmark = pytest.mark.gpu
U = R.U
NAN = float("nan")
SENT_F, SENT_H, NAN_H = 777.25, 0x5A5A, 0x7E00
# B,H,W = 3,5,7: M = 105 pixels = two 64-pixel blocks, the second with 41; 35 pixels per image, so image boundaries fall inside a block;
# C = 16 / 48 leave lanes of a 32-channel group idle.  2,8,8,192: one full production-width case.  1,2,2,16: the smallest.
PLANE_SHAPES = [(3, 5, 7, 16), (3, 5, 7, 48), (3, 5, 7, 64), (2, 8, 8, 192), (1, 2, 2, 16)]
CM_SHAPE = (3, 5, 7, 12)             # channel-major kernels only (no planes): 315 quads, second workgroup ragged, image boundaries inside
ALL_SHAPES = PLANE_SHAPES + [CM_SHAPE]
BIG = (3, 120, 100, 60)              # 540 000 quads > 2048 workgroups x 256: past kGridCap (rdo_common.h)
BIG_PLANES = (1, 724, 725, 16)       # 524 900 pixels = 8202 virtual blocks of 64 pixels x 1 channel group: past the plane forms' 8192
ITS = [0, 2]
COEF = 0.75
_id = lambda s: "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def ops():
    from hipops import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from hipops import _lib
    return _lib


def _tail_grid(L):
    return int(L.lib().rdo_get_tuning(b"tail_grid"))


@pytest.fixture(scope="module", autouse=True)
def _tail_grid_untouched(L):
    before = _tail_grid(L)
    yield
    assert _tail_grid(L) == before


@pytest.fixture(params=[None, 1], ids=["grid-default", "grid-1"])
def cap(request, ops, L):
    """the grid cap of the loss kernels of fused_tail.hip: the default, and 1 (one workgroup walks every block)"""
    if request.param is None:
        yield _tail_grid(L)
        return
    prev = ops.set_tuning("tail_grid", request.param)
    try:
        yield request.param
    finally:
        ops.set_tuning("tail_grid", prev)


# ---- guarded outputs ----------------------------------------------------------------------------------------------------------------------
class Guard:
    def __init__(self):
        self.bufs = []

    def f32(self, shape, fill=NAN):
        n = math.prod(shape)
        buf = torch.full((n + 64,), fill, device="cuda")
        buf[n:] = SENT_F
        self.bufs.append((buf, 0, n, SENT_F))
        return buf[:n].view(shape)

    def planes(self, ops, shape, scale, flag=None):
        n, Cc = 2 * math.prod(shape), shape[-1]
        buf = torch.full((n + 128,), SENT_H, dtype=torch.int16, device="cuda")
        buf[64:64 + n] = NAN_H
        self.bufs.append((buf, 64, 64 + n, SENT_H))
        return ops.H2(buf[64:64 + n].view(2, Cc // 16, n // 2 // Cc, 16), scale, flag)

    def check(self):
        for buf, lo, hi, s in self.bufs:
            assert bool((buf[:lo] == s).all()) and bool((buf[hi:] == s).all()), "a launch wrote outside its output"


def _word(ops):
    w = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    assert not ops.iter_bind_publish(w)
    return w


def _published(ops, w, it):
    assert int(w.item()) == it
    assert not ops.iter_bind_publish(None)          # the launch consumed the binding


def _it(it):
    return torch.tensor([it], dtype=torch.int32, device="cuda")


def _inputs(shape, seed, n_tgt=R.N_TARGETS):
    g = torch.Generator().manual_seed(seed * 1000 + shape[-1] + shape[1])
    return (torch.randn(*shape, generator=g), torch.randn(*shape, generator=g), torch.randn(n_tgt, *shape[1:], generator=g))


def _plant(t, values):
    """fixed positions of the flat tensor: first, inside, last"""
    pos = [0, t.numel() // 3 + 1, t.numel() - 1][:len(values)]
    t.view(-1)[pos] = torch.as_tensor(values, dtype=t.dtype)
    return pos


# ---- the loss log -------------------------------------------------------------------------------------------------------------------------
def _slots_cm(shape, g):
    """channel-major kernels: quad t of the flat tensor is walked by workgroup (t / 256) mod g, which adds into slot (workgroup mod 32)"""
    t = torch.arange(math.prod(shape)) // 4
    return (((t // 256) % g) % 32).view(shape)


def _slots_pix(shape, g):
    """pixel-major kernels: virtual block (pixel / 64) * ngroups + channel / 32, walked by workgroup (virtual block mod g)"""
    M, Cc = math.prod(shape[:-1]), shape[-1]
    vb = (torch.arange(M).view(M, 1) // 64) * ((Cc + 31) // 32) + torch.arange(Cc).view(1, Cc) // 32
    return ((vb % g) % 32).view(shape)


def _cm_grid(shape, cap):
    blocks = -(-(math.prod(shape) // 4) // 256)
    g = min(cap, blocks)
    return g, -(-blocks // g)           # workgroups, trips of a thread


def _pix_grid(shape, cap):
    M, Cc = math.prod(shape[:-1]), shape[-1]
    nvb = -(-M // 64) * -(-Cc // 32)
    g = min(cap, nvb)
    return g, -(-nvb // g)


def _check_log(log, it, slots, terms, D):
    """`terms`: float64, per element, already scaled; `slots`: the slot each element is added into"""
    assert (D + 4) * U <= 1e-5, D          # the bar the existing loss tests use; a case that does not meet it is too large
    got = log.detach().cpu().double()
    for r in range(got.shape[0]):
        if r != it:
            assert bool((got[r] == 0).all()), f"row {r} of another iteration was written"
    want = torch.zeros(32, dtype=torch.float64).index_add_(0, slots.reshape(-1), terms.reshape(-1))
    err = (got[it] - want).abs()
    assert bool((err <= (D + 4) * U * want).all()), (float((err / want.clamp_min(1e-300)).max()), (D + 4) * U)
    assert abs(float(got[it].sum()) - float(want.sum())) <= (D + 4) * U * float(want.sum())


# ---- gather + QDrop -----------------------------------------------------------------------------------------------------------------------
GATHER_GRID = [(p, off, seed) for p in (0.0, 0.5, 1.0) for off in (0, 5) for seed in (77, 0xDEADBEEF)]


@pytest.mark.parametrize("it", ITS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_gather_qdrop(ops, shape, it):
    B = shape[0]
    cq, cf, _ = _inputs((R.N_TARGETS,) + shape[1:], 1)
    idx = R.idx_table(B)
    cqd, cfd, idxd, itp = cq.cuda(), cf.cuda(), idx.cuda(), _it(it)
    for prob, off, seed in GATHER_GRID:
        G = Guard()
        out = G.f32(shape)
        w = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        ops.gather_qdrop(cqd, cfd, idxd, itp, B, prob, seed, out, batch_offset=off, iter_publish=w)
        assert torch.equal(out.cpu(), R.gather(cq, cf, idx, it, B, prob, seed, off)), (prob, off, seed)
        assert int(w.item()) == it
        G.check()


@pytest.mark.parametrize("it", ITS)
@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=_id)
def test_gather_qdrop_h2(ops, shape, it):
    B, scale = shape[0], 16.0
    cq, cf, _ = _inputs((R.N_TARGETS,) + shape[1:], 2)
    idx = R.idx_table(B)
    cqd, cfd, idxd, itp = cq.cuda(), cf.cuda(), idx.cuda(), _it(it)
    ops.h2_overflow(reset=True)
    for prob, off, seed in GATHER_GRID:
        ref = R.gather(cq, cf, idx, it, B, prob, seed, off)
        ref_pl = R.h2_planes(ref, scale)
        for with_out in (True, False):
            G = Guard()
            out = G.f32(shape) if with_out else None
            pl = G.planes(ops, shape, scale)
            w = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            ops.gather_qdrop_h2(cqd, cfd, idxd, itp, B, prob, seed, out, pl, batch_offset=off, iter_publish=w)
            if with_out:
                assert torch.equal(out.cpu(), ref), (prob, off, seed)
            assert torch.equal(pl.t.cpu(), ref_pl), (prob, off, seed, with_out)
            assert int(w.item()) == it
            G.check()
    assert not ops.h2_overflow(reset=True)


def test_gather_qdrop_past_the_fixed_grid_cap(ops):
    B, it = BIG[0], 2
    cq, cf, _ = _inputs((R.N_TARGETS,) + BIG[1:], 3)
    idx = R.idx_table(B)
    G = Guard()
    out = G.f32(BIG)
    ops.gather_qdrop(cq.cuda(), cf.cuda(), idx.cuda(), _it(it), B, 0.5, 0xDEADBEEF, out, batch_offset=5)
    assert torch.equal(out.cpu(), R.gather(cq, cf, idx, it, B, 0.5, 0xDEADBEEF, 5))
    G.check()


def test_gather_qdrop_h2_past_the_plane_grid_cap(ops):
    """8202 virtual blocks against the cap of 8192: the first ten are walked twice round the grid-stride loop (C = 16: the smallest tensor
    that gets there, 34 MB per fp32 copy)"""
    shape, it, scale = BIG_PLANES, 2, 16.0
    cq, cf, _ = _inputs((2,) + shape[1:], 4)
    idx = torch.tensor([[1], [0], [1]], dtype=torch.int32)
    G = Guard()
    out, pl = G.f32(shape), G.planes(ops, shape, scale)
    ops.gather_qdrop_h2(cq.cuda(), cf.cuda(), idx.cuda(), _it(it), 1, 0.5, 77, out, pl, batch_offset=1)
    ref = R.gather(cq, cf, idx, it, 1, 0.5, 77, 1)
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(pl.t.cpu(), R.h2_planes(ref, scale))
    G.check()


# ---- lp2 / lp -----------------------------------------------------------------------------------------------------------------------------
def _lp_case(shape, it, seed):
    pred, _, tgt = _inputs(shape, seed)
    idx = R.idx_table(shape[0])
    y = R.rows(tgt, idx, it, shape[0])
    pos = [0, pred.numel() // 3 + 1, pred.numel() - 1]
    pred.view(-1)[pos] = y.reshape(-1)[pos]              # d == 0 at the first, an inner and the last element
    return pred, tgt, idx, pos


@pytest.mark.parametrize("it", ITS)
@pytest.mark.parametrize("shape", ALL_SHAPES + [BIG], ids=_id)
def test_lp2_loss_grad(ops, shape, it):
    B, ppi = shape[0], shape[1] * shape[2]
    pred, tgt, idx, pos = _lp_case(shape, it, 5)
    G = Guard()
    grad, log = G.f32(shape), G.f32((3, 32), 0.0)
    w = _word(ops)
    ops.lp2_loss_grad(pred.cuda(), tgt.cuda(), idx.cuda(), _it(it), COEF, grad, log)
    _published(ops, w, it)
    ref, d = R.lp2(pred, tgt, idx, it, COEF)
    assert torch.equal(grad.cpu(), ref)
    assert bool((grad.cpu().view(-1)[pos] == 0).all())
    g, trips = _cm_grid(shape, 2048)
    # D = 2 (quad) + trips + 6 + 3 + workgroups per slot.  Small shapes: one trip, at most 7 workgroups: 2 + 1 + 9 + 1 = 13.
    # BIG: 2048 workgroups, 2 trips, 64 per slot: 2 + 2 + 9 + 64 = 77
    D = 2 + trips + 9 + -(-g // 32)
    assert D == (77 if shape == BIG else 13)
    _check_log(log, it, _slots_cm(shape, g), d.double() ** 2 * (COEF / (B * ppi)), D)
    G.check()


LP_CASES = [(s, p, it) for s in ALL_SHAPES for p in (1.0, 1.5, 3.0) for it in ITS] + [(BIG, 1.5, 2)]      # one case past the grid cap


@pytest.mark.parametrize("shape,p,it", LP_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_lp_loss_grad(ops, shape, p, it):
    B, ppi = shape[0], shape[1] * shape[2]
    c2, cp = (0.0, 1.0) if p == 3.0 else (0.75, 1.25)
    pred, tgt, idx, pos = _lp_case(shape, it, 6)
    predd, tgtd, idxd, itp = pred.cuda(), tgt.cuda(), idx.cuda(), _it(it)
    ref, _, _ = R.lp64(pred, tgt, idx, it, c2, cp, p)
    d = (pred - R.rows(tgt, idx, it, B)).double()
    t2, tp = c2 * d ** 2 / (B * ppi), cp * d.abs() ** p / (B * ppi)
    g, trips = _cm_grid(shape, 2048)
    # D = 4 * trips (one add per element) + 6 + 3 + workgroups per slot (+ 1 where both terms share one log: s2 + sp).
    # Small shapes: 4 + 9 + 1 (+ 1) = 14 / 15.  BIG: 8 + 9 + 64 (+ 1) = 81 / 82
    D = 4 * trips + 9 + -(-g // 32)
    assert D == (81 if shape == BIG else 14)
    slots = _slots_cm(shape, g)
    for two_logs in (False, True):
        G = Guard()
        grad, log, logp = G.f32(shape), G.f32((3, 32), 0.0), (G.f32((3, 32), 0.0) if two_logs else None)
        w = _word(ops)
        ops.lp_loss_grad(predd, tgtd, idxd, itp, c2, cp, p, grad, log, logp)
        _published(ops, w, it)
        got = grad.cpu()
        assert bool(torch.isfinite(got).all())
        torch.testing.assert_close(got.double(), ref, rtol=2e-5, atol=1e-7)       # the bar of test_lp_loss_kernel_matches_autograd
        assert bool((got.view(-1)[pos] == 0).all())
        if two_logs:
            _check_log(log, it, slots, t2, D)
            _check_log(logp, it, slots, tp, D)
        else:
            _check_log(log, it, slots, t2 + tp, D + 1)
        G.check()


# ---- activation + loss + activation backward ---------------------------------------------------------------------------------------------
CM_SUBSETS = [("out", "grad_out", "dpre"), ("grad_out",), ("dpre",), ("out", "dpre")]
PIX_SUBSETS = [("out", "grad_out", "dpre", "planes"), ("planes",), ("dpre", "planes"), ("out", "grad_out", "planes")]


def _act_case(shape, seed):
    pre, res, tgt = _inputs(shape, seed)
    _plant(pre, [0.0, -0.0, 0.0])                       # the kink of ReLU / LeakyReLU
    return pre, res, tgt, R.idx_table(shape[0])


def _loss_depth(pix, shape, cap):
    """-> (workgroups, D).  channel-major: 2 + trips + 9 + workgroups per slot; pixel-major: two quads per virtual block, 2 + 2 * trips + 9 +
    workgroups per slot.  The largest here: 2,8,8,192 under tail_grid = 1 -- 24 trips (2 + 24 + 9 + 1 = 36) and 12 virtual blocks (2 + 24 + 9 + 1 = 36)"""
    g, trips = (_pix_grid if pix else _cm_grid)(shape, cap)
    D = 2 + (2 if pix else 1) * trips + 9 + -(-g // 32)
    assert D <= 36
    return g, D


@pytest.mark.parametrize("it", ITS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_loss_act_bwd(ops, cap, shape, it):
    B, ppi, Cc = shape[0], shape[1] * shape[2], shape[-1]
    pre, res, tgt, idx = _act_case(shape, 7)
    pred, resd, tgtd, idxd, itp = pre.cuda(), res.cuda(), tgt.cuda(), idx.cuda(), _it(it)
    has_planes = Cc % 16 == 0
    res_pl = ops.H2(R.h2_planes(res, 32.0).cuda(), 32.0) if has_planes else None
    res_back = ops.h2_to_float(res_pl, shape).cpu() if has_planes else None     # (h1 + h2) / s: what the kernel adds
    first = True
    ops.h2_overflow(reset=True)
    for act in (0, 1, 2):
        for rkind in ("none", "fp32", "planes") if has_planes else ("none", "fp32"):
            ref = R.loss_act(pre, {"none": None, "fp32": res, "planes": res_back}[rkind], tgt, idx, it, COEF, act)
            scale = ops.pow2_scale(ref["dpre"].abs().max())
            ref_pl = R.h2_planes(ref["dpre"], scale) if has_planes else None
            terms = ref["d"].double() ** 2 * (COEF / (B * ppi))
            subsets = CM_SUBSETS + (PIX_SUBSETS if has_planes else [])
            for sub in subsets:
                pix = "planes" in sub or rkind == "planes"
                G = Guard()
                o = {k: (G.f32(shape) if k in sub else None) for k in ("out", "grad_out", "dpre")}
                pl = G.planes(ops, shape, scale) if "planes" in sub else None
                log = G.f32((3, 32), 0.0)
                w = _word(ops) if first else None
                ops.loss_act_bwd(pred, resd if rkind == "fp32" else None, tgtd, idxd, itp, COEF, act, log, out=o["out"], grad_out=o["grad_out"],
                                 dpre=o["dpre"], dpre_planes=pl, residual_planes=res_pl if rkind == "planes" else None)
                if first:
                    _published(ops, w, it)
                    first = False
                what = (act, rkind, sub)
                for k in ("out", "grad_out", "dpre"):
                    if o[k] is not None:
                        assert torch.equal(o[k].cpu(), ref[k]), (k,) + what
                if pl is not None:
                    if o["dpre"] is not None:        # the planes of the launch's own fp32 dpre
                        assert torch.equal(pl.t.cpu(), R.h2_planes(o["dpre"].cpu(), scale)), what
                    assert torch.equal(pl.t.cpu(), ref_pl), what
                g, D = _loss_depth(pix, shape, cap)
                _check_log(log, it, (_slots_pix if pix else _slots_cm)(shape, g), terms, D)
                G.check()
    assert not ops.h2_overflow(reset=True)


@pytest.mark.parametrize("it", ITS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_loss_act_bwd_splitk(ops, cap, shape, it):
    """hand-made partial sums [ks][B * per_image] (the entry takes any pointer): pre = ((0 + slab 0) + slab 1 + ...) + bias"""
    B, ppi, Cc = shape[0], shape[1] * shape[2], shape[-1]
    _, res, tgt, idx = _act_case(shape, 8)
    gen = torch.Generator().manual_seed(80 + Cc)
    tgtd, idxd, itp = tgt.cuda(), idx.cuda(), _it(it)
    first = True
    for ks in (2, 3, 5):
        part = torch.randn(ks, *shape, generator=gen)
        part.view(ks, -1)[:, [0, 9]] = torch.tensor([0.0, -0.0]).expand(ks, 2)          # sums to +0 whatever the signs
        for bias in (None, torch.randn(Cc, generator=gen)):
            act = ks % 3
            r = res if (ks + (bias is None)) % 2 else None
            pre = R.splitk_pre(part, bias)
            ref = R.loss_act(pre, r, tgt, idx, it, COEF, act)
            G = Guard()
            o = {k: G.f32(shape) for k in ("out", "grad_out", "dpre")}
            log = G.f32((3, 32), 0.0)
            w = _word(ops) if first else None
            ops.loss_act_bwd_splitk(part.cuda(), ks, None if bias is None else bias.cuda(), shape, None if r is None else r.cuda(), tgtd, idxd, itp,
                                    COEF, act, log, out=o["out"], grad_out=o["grad_out"], dpre=o["dpre"])
            if first:
                _published(ops, w, it)
                first = False
            for k in o:
                assert torch.equal(o[k].cpu(), ref[k]), (k, ks, bias is not None)
            g, D = _loss_depth(False, shape, cap)
            _check_log(log, it, _slots_cm(shape, g), ref["d"].double() ** 2 * (COEF / (B * ppi)), D)
            G.check()


# ---- GDN / IGDN epilogue + loss + dL/dnorm -------------------------------------------------------------------------------------------------
def _within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), (what, float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("it", ITS)
@pytest.mark.parametrize("shape,mag", R.GDN_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_loss_gdn_bwd(ops, cap, shape, mag, it):
    B, ppi, Cc = shape[0], shape[1] * shape[2], shape[-1]
    coef = 2.0
    c = R.gdn_inputs(shape, mag)
    idx = R.idx_table(B)
    xd, nd, resd, tgtd, idxd, itp = c["x"].cuda(), c["n"].cuda(), c["res"].cuda(), c["tgt"].cuda(), idx.cuda(), _it(it)
    y = R.rows(c["tgt"], idx, it, B)
    # (t fp32, t planes, out): the fp32 form with and without `out`, the plane form with t as planes, as both, and without `out`
    forms = [(True, False, True), (True, False, False)] + ([(False, True, True), (True, True, True), (True, True, False)] if Cc % 16 == 0 else [])
    first = True
    ops.h2_overflow(reset=True)
    for inverse in (False, True):
        for with_res in (False, True):
            r64 = R.loss_gdn64(c["x"], c["n"], c["res"] if with_res else None, c["tgt"], idx, it, coef, inverse)
            bnd = R.gdn_bounds(r64)
            scale = ops.pow2_scale(r64["t"].abs().max())
            terms = planes_of_t = None
            for t32, tpl, with_out in forms:
                G = Guard()
                out, gout = (G.f32(shape) if with_out else None), G.f32(shape)
                t = G.f32(shape) if t32 else None
                pl = G.planes(ops, shape, scale) if tpl else None
                log = G.f32((3, 32), 0.0)
                w = _word(ops) if first else None
                ops.loss_gdn_bwd(xd, nd, resd if with_res else None, tgtd, idxd, itp, coef, inverse, log, gout, t=t, t_planes=pl, out=out)
                if first:
                    _published(ops, w, it)
                    first = False
                what = (inverse, with_res, t32, tpl, with_out)
                if with_out:
                    _within(out.cpu(), r64["out"], bnd["out"], ("out",) + what)
                    if terms is None:            # the launch's own differences, its `out` being within the bound (module docstring)
                        terms = (out.cpu() - y).double() ** 2 * (coef / (B * ppi))
                _within(gout.cpu(), r64["grad_out"], bnd["grad_out"], ("grad_out",) + what)
                if t32:
                    _within(t.cpu(), r64["t"], bnd["t"], ("t",) + what)
                if tpl and t32:
                    planes_of_t = R.h2_planes(t.cpu(), scale)
                    assert torch.equal(pl.t.cpu(), planes_of_t), what
                g, D = _loss_depth(tpl, shape, cap)
                _check_log(log, it, (_slots_pix if tpl else _slots_cm)(shape, g), terms, D)
                G.check()
                if tpl and not t32:
                    only = pl.t.cpu()
            if Cc % 16 == 0:
                assert torch.equal(only, planes_of_t), (inverse, with_res, "planes-only launch")
    assert not ops.h2_overflow(reset=True)


@pytest.mark.parametrize("shape,mag", R.GDN_CASES + [(BIG, 1.0)], ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_gdn_bwd_dx(ops, shape, mag):
    """dx = g n^(-+1/2) + 2 x acc: the fp32 kernel of elementwise.hip, and rdo_gdn_bwd_dx_h2 as fp32, as fp32 + planes, as planes"""
    Cc = shape[-1]
    c = R.gdn_inputs(shape, mag)
    gd, xd, nd, ad = (c[k].cuda() for k in ("g", "x", "n", "acc"))
    ops.h2_overflow(reset=True)
    for inverse in (False, True):
        ref, bound = R.gdn_dx64(c["g"], c["x"], c["n"], c["acc"], inverse)
        scale = ops.pow2_scale(ref.abs().max())
        G = Guard()
        a, b = G.f32(shape), G.f32(shape)
        ops.gdn_bwd_dx(gd, xd, nd, ad, inverse, out=a)
        ops.gdn_bwd_dx_h2(gd, xd, nd, ad, inverse, dx=b)
        _within(a.cpu(), ref, bound, ("gdn_bwd_dx", inverse))
        _within(b.cpu(), ref, bound, ("gdn_bwd_dx_h2", inverse))
        if Cc % 16 == 0:
            dx, pl, pl2 = G.f32(shape), G.planes(ops, shape, scale), G.planes(ops, shape, scale)
            ops.gdn_bwd_dx_h2(gd, xd, nd, ad, inverse, dx=dx, dx_planes=pl)
            ops.gdn_bwd_dx_h2(gd, xd, nd, ad, inverse, dx_planes=pl2)
            _within(dx.cpu(), ref, bound, ("gdn_bwd_dx_h2 + planes", inverse))
            assert torch.equal(pl.t.cpu(), R.h2_planes(dx.cpu(), scale))
            assert torch.equal(pl2.t.cpu(), pl.t.cpu())
        G.check()
    assert not ops.h2_overflow(reset=True)


def test_gdn_bwd_dx_h2_past_the_plane_grid_cap(ops):
    shape = BIG_PLANES
    gen = torch.Generator().manual_seed(9)
    g, x, acc = (torch.randn(*shape, generator=gen) for _ in range(3))
    n = 0.5 + torch.rand(*shape, generator=gen) + 0.1 * x * x
    ref, bound = R.gdn_dx64(g, x, n, acc, False)
    scale = ops.pow2_scale(ref.abs().max())
    G = Guard()
    dx, pl = G.f32(shape), G.planes(ops, shape, scale)
    ops.gdn_bwd_dx_h2(g.cuda(), x.cuda(), n.cuda(), acc.cuda(), False, dx=dx, dx_planes=pl)
    _within(dx.cpu(), ref, bound, "dx")
    assert torch.equal(pl.t.cpu(), R.h2_planes(dx.cpu(), scale))
    G.check()


# ---- r = 2 pixel shuffle and its gradient --------------------------------------------------------------------------------------------------
SMALL_BHW = [(1, 1, 1), (2, 3, 5), (1, 9, 11)]      # (2,3,5) and (1,9,11): 30 and 99 small pixels, ragged last 32- and 64-pixel blocks


@pytest.mark.parametrize("Cl", [4, 12, 16, 48])     # channels of the LARGE tensor; planes from 16 on
@pytest.mark.parametrize("bhw", SMALL_BHW, ids=_id)
def test_pixel_shuffle_h2(ops, bhw, Cl):
    B, H, W = bhw
    x = torch.randn(B, H, W, 4 * Cl, generator=torch.Generator().manual_seed(Cl + H))
    ref = R.pixel_shuffle2(x)
    xd, shape, scale = x.cuda(), tuple(ref.shape), 16.0
    G = Guard()
    out = G.f32(shape)
    ops.pixel_shuffle_h2(xd, out=out)
    assert torch.equal(out.cpu(), ref)
    if Cl % 16 == 0:
        out2, pl, pl2 = G.f32(shape), G.planes(ops, shape, scale), G.planes(ops, shape, scale)
        ops.pixel_shuffle_h2(xd, out=out2, out_planes=pl)
        ops.pixel_shuffle_h2(xd, out_planes=pl2)
        assert torch.equal(out2.cpu(), ref)
        assert torch.equal(pl.t.cpu(), R.h2_planes(ref, scale)) and torch.equal(pl2.t.cpu(), pl.t.cpu())
    G.check()


@pytest.mark.parametrize("Cl", [4, 12, 16, 48])
@pytest.mark.parametrize("bhw", SMALL_BHW, ids=_id)
def test_pixel_unshuffle2(ops, bhw, Cl):
    B, H, W = bhw
    x = torch.randn(B, 2 * H, 2 * W, Cl, generator=torch.Generator().manual_seed(Cl + W))
    ref = R.pixel_unshuffle2(x)
    xd, shape, scale = x.cuda(), tuple(ref.shape), 16.0
    G = Guard()
    out = G.f32(shape)
    ops.pixel_unshuffle2(xd, out=out)
    assert torch.equal(out.cpu(), ref)
    # the small tensor has 4 Cl channels: planes exist for every Cl here
    out2, pl, pl2 = G.f32(shape), G.planes(ops, shape, scale), G.planes(ops, shape, scale)
    ops.pixel_unshuffle2(xd, out=out2, out_planes=pl)
    ops.pixel_unshuffle2(xd, out_planes=pl2)
    assert torch.equal(out2.cpu(), ref)
    assert torch.equal(pl.t.cpu(), R.h2_planes(ref, scale)) and torch.equal(pl2.t.cpu(), pl.t.cpu())
    G.check()


def test_pixel_shuffles_past_the_plane_grid_caps(ops):
    """shuffle: 8202 virtual blocks of 64 small pixels x 16 large channels (the fewest a plane form takes); unshuffle: blocks of 32 small
    pixels, 8225 of them at 4 large channels"""
    B, H, W, Cc = BIG_PLANES
    scale = 16.0
    x = torch.randn(B, H, W, 4 * Cc, generator=torch.Generator().manual_seed(10))
    ref = R.pixel_shuffle2(x)
    G = Guard()
    pl = G.planes(ops, tuple(ref.shape), scale)
    ops.pixel_shuffle_h2(x.cuda(), out_planes=pl)
    assert torch.equal(pl.t.cpu(), R.h2_planes(ref, scale))
    G.check()
    x = torch.randn(1, 1026, 1026, 4, generator=torch.Generator().manual_seed(11))        # 513 x 513 = 263 169 small pixels
    ref = R.pixel_unshuffle2(x)
    G = Guard()
    out, pl = G.f32(tuple(ref.shape)), G.planes(ops, tuple(ref.shape), scale)
    ops.pixel_unshuffle2(x.cuda(), out=out, out_planes=pl)
    assert torch.equal(out.cpu(), ref) and torch.equal(pl.t.cpu(), R.h2_planes(ref, scale))
    G.check()


# ---- the overflow words of the plane producers ---------------------------------------------------------------------------------------------
def _producers(ops, poison):
    """name -> launch(planes) -> the fp32 output of the same launch (CPU).  `poison`: one inf in the input that reaches one output"""
    shape, it = (3, 5, 7, 48), 2
    B = shape[0]
    inf = float("inf")
    pre, res, tgt = _inputs(shape, 11)
    cq, cf, _ = _inputs((R.N_TARGETS,) + shape[1:], 12)
    c = R.gdn_inputs(shape, 1.0)
    xs = torch.randn(3, 5, 7, 4 * 48, generator=torch.Generator().manual_seed(13))
    xu = torch.randn(3, 10, 14, 12, generator=torch.Generator().manual_seed(14))
    if poison:
        pre[1, 2, 3, 4] = cf[4, 1, 2, 3] = xs[1, 2, 3, 4] = xu[1, 2, 3, 4] = inf       # (cached image 4 is gathered once by row it = 2)
        c["x"][1, 2, 3, 4] = c["g"][1, 2, 3, 4] = inf
    idxd, itp, tgtd = R.idx_table(B).cuda(), _it(it), tgt.cuda()
    cu = {k: v.cuda() for k, v in c.items()}
    pred, cqd, cfd, xsd, xud = pre.cuda(), cq.cuda(), cf.cuda(), xs.cuda(), xu.cuda()
    log = torch.zeros(3, 32, device="cuda")

    def fresh(s):
        return torch.full(s, NAN, device="cuda")

    def gather(pl):
        out = fresh(shape)
        ops.gather_qdrop_h2(cqd, cfd, idxd, itp, B, 0.0, 77, out, pl)
        return out

    def loss_act(pl):
        out = fresh(shape)
        ops.loss_act_bwd(pred, None, tgtd, idxd, itp, COEF, 0, log, dpre=out, dpre_planes=pl)
        return out

    def loss_gdn(pl):
        out, gout = fresh(shape), fresh(shape)
        ops.loss_gdn_bwd(cu["x"], cu["n"], None, cu["tgt"], idxd, itp, COEF, False, log, gout, t=out, t_planes=pl)
        return out

    def gdn_dx(pl):
        out = fresh(shape)
        ops.gdn_bwd_dx_h2(cu["g"], cu["x"], cu["n"], cu["acc"], False, dx=out, dx_planes=pl)
        return out

    def shuffle(pl):
        out = fresh((3, 10, 14, 48))
        ops.pixel_shuffle_h2(xsd, out=out, out_planes=pl)
        return out

    def unshuffle(pl):
        out = fresh((3, 5, 7, 48))
        ops.pixel_unshuffle2(xud, out=out, out_planes=pl)
        return out

    return {"gather_qdrop_h2": (gather, shape), "loss_act_bwd": (loss_act, shape), "loss_gdn_bwd": (loss_gdn, shape), "gdn_bwd_dx_h2": (gdn_dx, shape),
            "pixel_shuffle_h2": (shuffle, (3, 10, 14, 48)), "pixel_unshuffle2": (unshuffle, (3, 5, 7, 48))}


PRODUCERS = ["gather_qdrop_h2", "loss_act_bwd", "loss_gdn_bwd", "gdn_bwd_dx_h2", "pixel_shuffle_h2", "pixel_unshuffle2"]


@pytest.mark.parametrize("name", PRODUCERS)
def test_overflow_words(ops, name):
    """An output H2 with its own flag words: word 0 = the fp32 bit pattern of the largest finite |x s| beyond fp16's 65504, word 1 = a
    non-finite value was met; the per-device default flag stays clear"""
    ops.h2_overflow(reset=True)

    def run(launch, shape, scale):
        flag = torch.zeros(2, dtype=torch.int32, device="cuda")
        out = launch(ops.h2_empty(shape, "cuda", scale, flag)).cpu()
        return out, [int(v) for v in flag.cpu()]

    launch, shape = _producers(ops, False)[name]
    out, words = run(launch, shape, 2.0 ** -10)
    assert words == [0, 0]
    big = ops.pow2_scale(out.abs().max()) * 1024.0       # the largest |x s| lands in (65536, 131072]
    out, words = run(launch, shape, big)
    assert words == [R.overflow_word(out, big), 0] and words[0] > 0x477FE000
    launch, shape = _producers(ops, True)[name]
    out, words = run(launch, shape, ops.pow2_scale(out.abs().max()))
    assert int((~torch.isfinite(out)).sum()) == 1
    assert words == [0, 1]
    assert not ops.h2_overflow(reset=True)
