"""Window attention kernels of csrc/swin.hip (forward with probabilities, probabilities only, probs @ v, backward) against the float64
reference of oracle/attention_oracle.py, per element, on every path the host can choose and through the persistent loop.

Every launch writes into NaN-filled outputs, which must come back finite everywhere: an element the kernel does not write cannot inherit a
right answer from an earlier allocation.  Every element obeys |got - ref| <= c * unit with the units of the oracle's docstring and
c = 4 x the worst err / unit of the oracle's float32 restatement ON THE SAME INPUTS (the allowance for
the hardware exponential, the MFMA summation order and one rounding more); probabilities get the additive floor 2^-126.  No element is left
out, and no bound comes from a kernel's output.  Inputs: tests/attention_cases.py (per-head temperatures, planted one-hot and tied rows, an
all-zero window, channel scales over two decades).  Each figure is printed before it is asserted (pytest -s)."""
import pytest
import torch

import attention_cases as AC
from oracle import attention_oracle as A

pytestmark = pytest.mark.gpu


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def _desc(g):
    from hipops import ops
    return ops.attn_desc(g.B, g.H, g.W, g.C, g.heads, g.ws, g.shift, g.scale)


class Case:
    """operands of one geometry on both devices, the float64 reference and the allowed multiples, computed once"""

    def __init__(self, geom, seed):
        self.g = g = A.Geom(*geom)
        self.qkv, self.bias, self.dout = AC.trained_like(g, seed)
        self.ref = A.reference(g, self.qkv, self.bias, self.dout)
        r32 = A.restate32(g, self.qkv, self.bias, self.dout)
        ref, C = self.ref, g.C
        self.thirds = {"dq": slice(0, C), "dk": slice(C, 2 * C), "dv": slice(2 * C, 3 * C)}
        self.r32 = {"probs": A.worst_ratio(r32["probs"], ref["probs"], ref["u_probs"], A.P_FLOOR),
                    "out": A.worst_ratio(r32["out"], ref["out"], ref["u_out"])}
        for k, sl in self.thirds.items():
            self.r32[k] = A.worst_ratio(r32["dqkv"][..., sl], ref["dqkv"][..., sl], ref["u_dqkv"][..., sl])
        assert all(v < float("inf") for v in self.r32.values()), self.r32          # reference and restatement finite on these inputs
        for k in ("s", "p", "u_s", "dqkv_analytic"):                                # (not needed below: a gigabyte at the persistent shapes)
            del ref[k]
        self.d = _desc(g)
        self.qc, self.bc, self.doc = self.qkv.cuda(), self.bias.cuda(), self.dout.cuda()

    def hold(self, what, got, ref, unit, r32, floor=0.0):
        assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not finite (never written?)"
        ratio = A.worst_ratio(got, ref, unit, floor)
        print(f"  {what}: err / unit  restatement {r32:.3f}  kernel {ratio:.3f}  allowed {4 * r32:.3f}")
        assert ratio <= 4 * r32, (what, ratio, 4 * r32)
        return ratio

    def forward(self):
        from hipops import ops
        g, ref = self.g, self.ref
        out, probs = _nan(g.B, g.H, g.W, g.C), _nan(g.windows, g.N, g.N, g.heads)
        ops.window_attention(self.d, self.qc, self.bc, out=out, probs=probs)
        self.hold("probs", probs, ref["probs"], ref["u_probs"], self.r32["probs"], A.P_FLOOR)
        self.hold("out", out, ref["out"], ref["u_out"], self.r32["out"])
        return out, probs

    def probs_only(self, probs):
        from hipops import ops
        only = torch.full_like(probs, float("nan"))
        assert ops.window_attention(self.d, self.qc, self.bc, probs=only, compute_out=False) is None
        assert torch.equal(only, probs)                                             # bit-equal (and therefore finite)

    def pv(self, probs):
        """probs @ v from the kernel's own probabilities as GIVEN data: reference and restatement are formed from the same float32 values"""
        from hipops import ops
        g = self.g
        ref, unit = A.pv_reference(g, self.qkv, probs.cpu())
        r32 = A.worst_ratio(A.pv32(g, self.qkv, probs.cpu()), ref, unit)
        out = _nan(g.B, g.H, g.W, g.C)
        ops.window_attention_pv(self.d, self.qc, probs, out=out)
        self.hold("pv", out, ref, unit, r32)
        return out

    def backward(self):
        from hipops import ops
        ref = self.ref
        dqkv = torch.full_like(self.qc, float("nan"))
        ops.window_attention_bwd(self.d, self.qc, self.bc, self.doc, dqkv=dqkv)
        assert bool(torch.isfinite(dqkv).all()), f"dqkv: {int((~torch.isfinite(dqkv)).sum())} elements not finite (never written?)"
        for k, sl in self.thirds.items():
            self.hold(k, dqkv[..., sl], ref["dqkv"][..., sl], ref["u_dqkv"][..., sl], self.r32[k])
        return dqkv


@pytest.mark.parametrize("name", list(AC.PATH_CASES))
def test_every_path_matches_float64_per_element(name):
    """forward with probs, compute_out=False, pv and backward of one host-side path each (the case's name says which)"""
    print(f"\n{name} {AC.PATH_CASES[name]}")
    c = Case(AC.PATH_CASES[name], seed=len(name) + AC.PATH_CASES[name][3])
    out, probs = c.forward()
    c.probs_only(probs)
    c.pv(probs)
    c.backward()


def _persistent_condition(g):
    """more items than can be resident: at most 8 workgroups of 256 threads fit a CU, so 2 x 8 x CUs + 8 items send every workgroup
    through the loop at least twice -- a condition, not a hope"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    need = 2 * 8 * cus + 8
    nitems = g.windows * g.heads
    assert nitems >= need, f"{nitems} items do not exceed twice the resident workgroups of {cus} CUs ({need} needed)"
    return nitems


def _smallest_batch(B0, H, W, C, heads, ws, shift):
    """the smallest B >= B0 that meets `_persistent_condition` (B0 is it on 256 CUs)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_image = (H // ws) * (W // ws) * heads
    return max(B0, -(-(2 * 8 * cus + 8) // per_image))


PERSISTENT = {
    "hd32_n64_shift4_xcd_order": (3, 128, 128, 192, 6, 8, 4),          # 768 windows: 4 608 items, the model's g_a / g_s shape
    "hd12_n16_shift2_plain_order_zero_lds": (1, 68, 68, 192, 16, 4, 2),  # 289 windows (not a multiple of 8): 4 624 items, zero_lds between items
    "hd3_scalar_xcd_order": (5, 64, 64, 48, 16, 8, 4),                 # 320 windows: 5 120 items on the scalar path
    "hd4_343_windows_uneven_rounds": (7, 56, 56, 64, 16, 8, 0),        # 5 488 items: workgroups end on different rounds
    # 11 heads: the grid is a multiple of 8 (and, with 256 CUs, of 256), so with 6 or 16 heads a workgroup meets the SAME head on every
    # round and a prefetch of the wrong head (`fetch(buf ^ 1, head)`) reads the right data; 11 divides no grid (`_head_changes`)
    "hd16_n64_11_heads_xcd_order": (6, 64, 64, 176, 11, 8, 4),         # 384 windows: 4 224 items
    "hd16_n16_11_heads_plain_order": (1, 80, 76, 176, 11, 4, 2),       # 380 windows (not a multiple of 8): 4 180 items
}


def _head_changes(g):
    """the head of a workgroup's next item differs from the current one's: the grid is per_cu x CUs rounded down to a multiple of 8 with
    per_cu <= 8, and a workgroup's items are `grid` apart (plain order) or `grid / 8` slots apart (XCD order) with the head fastest -- the
    head repeats only if `heads` divides that step, which a prime above 8 that does not divide CUs / 8 never does"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert g.heads > 8 and all(g.heads % f for f in range(2, g.heads)) and (cus // 8) % g.heads != 0, (g.heads, cus)


def test_persistent_loop_hd32_forward_backward_and_determinism():
    """every workgroup takes at least two items: the `more` branch, tables / fetch into the other buffer, the buffer flip, the closing
    barrier and the slot / heads walk of `attn_item`; three launches give the same bits"""
    from hipops import ops
    geom = PERSISTENT["hd32_n64_shift4_xcd_order"]
    c = Case((_smallest_batch(*geom),) + geom[1:], seed=32)
    print(f"\nhd32 persistent: {_persistent_condition(c.g)} items")
    out, probs = c.forward()
    dqkv = c.backward()
    g = c.g
    for _ in range(2):
        out2, probs2 = _nan(g.B, g.H, g.W, g.C), torch.full_like(probs, float("nan"))
        ops.window_attention(c.d, c.qc, c.bc, out=out2, probs=probs2)
        dqkv2 = torch.full_like(dqkv, float("nan"))
        ops.window_attention_bwd(c.d, c.qc, c.bc, c.doc, dqkv=dqkv2)
        assert torch.equal(out2, out) and torch.equal(probs2, probs) and torch.equal(dqkv2, dqkv)


@pytest.mark.parametrize("name", [n for n in PERSISTENT if not n.startswith("hd32")])
def test_persistent_loop_matches_float64_per_element(name):
    geom = PERSISTENT[name]
    if "uneven" not in name:
        geom = (_smallest_batch(*geom),) + geom[1:]
    c = Case(geom, seed=len(name))
    print(f"\n{name} {geom}: {_persistent_condition(c.g)} items")
    if "11_heads" in name:
        _head_changes(c.g)
    c.forward()
    c.backward()


def _off_by_one_float(t, misalign=True):
    """-> (a contiguous view of t's shape that starts one float past a 16-byte boundary, its buffer): 65 sentinel floats in front
    (64 + the one), 64 behind; `misalign=False`: 64 in front, the view 16-byte aligned"""
    front = 65 if misalign else 64
    buf = torch.full((front + t.numel() + 64,), SENTINEL, device="cuda", dtype=torch.float32)
    view = buf[front:front + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (view.data_ptr() % 16 == 4) == misalign and buf.data_ptr() % 16 == 0
    return view, buf, front


SENTINEL = -7.25


def _guards_untouched(buf, front, n):
    return bool((buf[:front] == SENTINEL).all()) and bool((buf[front + n:] == SENTINEL).all())


@pytest.mark.parametrize("which", ["all", "inputs_only", "outputs_only"])
@pytest.mark.parametrize("name", ["vec_it2_model_head_hd32", "vec_n16_hyper_hd12", "vec_n16_ndb_hd32"])
def test_misaligned_views_take_the_scalar_forms_and_give_the_same_bits(name, which):
    """qkv, dout (inputs) and out, dqkv (outputs) one float into a larger buffer: the vector loads / stores need 16-byte aligned pointers,
    so the host drops the prefetch path for misaligned inputs and the kernels fall back to 4-byte accesses for whichever pointer is
    misaligned.  Products and their order are the same: bit-equal to the aligned run.  64 sentinels on both sides stay untouched."""
    from hipops import ops
    c = Case(AC.PATH_CASES[name], seed=7)
    g = c.g
    out0, probs0 = c.forward()
    dqkv0 = c.backward()
    pv0 = c.pv(probs0)
    mis_in, mis_out = which in ("all", "inputs_only"), which in ("all", "outputs_only")
    qv, qbuf, qf = _off_by_one_float(c.qc, mis_in)
    dv, dbuf, df = _off_by_one_float(c.doc, mis_in)
    ov, obuf, of = _off_by_one_float(_nan(g.B, g.H, g.W, g.C), mis_out)
    gv, gbuf, gf = _off_by_one_float(torch.full_like(c.qc, float("nan")), mis_out)
    probs = torch.full_like(probs0, float("nan"))
    ops.window_attention(c.d, qv, c.bc, out=ov, probs=probs)
    assert torch.equal(ov, out0) and torch.equal(probs, probs0)
    ov.fill_(float("nan"))
    ops.window_attention_pv(c.d, qv, probs0, out=ov)
    assert torch.equal(ov, pv0)
    ops.window_attention_bwd(c.d, qv, c.bc, dv, dqkv=gv)
    assert torch.equal(gv, dqkv0)
    for buf, front, n in ((qbuf, qf, qv.numel()), (dbuf, df, dv.numel()), (obuf, of, ov.numel()), (gbuf, gf, gv.numel())):
        assert _guards_untouched(buf, front, n)
    assert torch.equal(qv, c.qc) and torch.equal(dv, c.doc)                         # the inputs themselves
