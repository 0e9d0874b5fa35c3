"""CPU-only checks of the entry points that put the r = 2 pixel shuffle of a sub-pixel conv into its producers' stores
(include/rdo_ptq_subpel.h): declared, exported, bound from a table of their own; the gates; arguments refused before any launch.
A unit tail cannot meet a store mode at all: rdo_conv2d_fwd_h2_tail has no such argument and rdo_conv2d_fwd_h2_px no tail."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDO_EINVAL = -22
NAMES = {"rdo_conv2d_fwd_h2_px_supported", "rdo_conv2d_fwd_h2_px", "rdo_split_h2_conv_px", "rdo_gdn_fwd_bwd_px_supported", "rdo_gdn_fwd_bwd_px",
         "rdo_adaround_step_batch_gather_px"}


def test_header_and_table_declare_the_same_names():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_subpel.h")).read()
    declared = set(re.findall(r"^int (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == NAMES == set(L.EXPORTS_SUBPEL)
    h = L.lib()
    others = set(L.EXPORTS) | set(L.EXPORTS_GDN) | set(L.EXPORTS_BIAS) | set(L.EXPORTS_BITS) | set(L.EXPORTS_PACK)
    for name in declared:
        assert hasattr(h, name) and name not in others
    main = open(os.path.join(ROOT, "include", "rdo_ptq_hip.h")).read()
    assert not any(re.search(r"\b%s\(" % n, main) for n in NAMES)
    assert len(L.EXPORTS) == 124


def _px(ops, xs, w, mode):
    return ops.conv_h2_px_supported(xs, w, 1, 1, mode)


def test_conv_gate():
    from hipops import _lib as L
    from hipops import ops
    S, U = L.STORE_SHUFFLE, L.STORE_UNSHUFFLE
    # the sub-pixel convs and dgrads of the three RBU units of Cheng2020 (N = 192, B = 4): direct 256 x 192, 256 x 48 and split over K
    for hw in (64, 32, 16):
        assert _px(ops, (4, hw, hw, 192), (768, 3, 3, 192), S)
        assert _px(ops, (4, 2 * hw, 2 * hw, 192), (192, 3, 3, 192), U)
    assert _px(ops, (2, 64, 64, 32), (768, 3, 3, 32), S) and _px(ops, (5, 64, 64, 64), (128, 3, 3, 64), U)      # 256 x 64 tiles
    # mode 0 is the plain gate; unknown modes are refused
    assert _px(ops, (4, 64, 64, 192), (768, 3, 3, 192), 0) and not _px(ops, (4, 64, 64, 192), (768, 3, 3, 192), 3)
    assert not _px(ops, (1, 16, 16, 32), (192, 3, 3, 32), 0)                       # not on the plane path at all
    # shuffle: Cout / 4 in whole records of 16 (Cout % 64 == 0) and in whole tiles of the launch
    assert not _px(ops, (4, 64, 64, 192), (96, 3, 3, 192), S)                      # Cout / 4 = 24
    assert not _px(ops, (4, 64, 64, 192), (160, 3, 3, 192), S)                     # Cout / 4 = 40
    assert not _px(ops, (4, 64, 64, 192), (320, 3, 3, 192), S)                     # Cout / 4 = 80: no multiple of the 64-channel tile
    # unshuffle: even H and W; odd sizes are not on the halo kernels (16 x 16 patches) in the first place
    assert not _px(ops, (4, 63, 64, 192), (192, 3, 3, 192), U) and not _px(ops, (4, 64, 33, 192), (192, 3, 3, 192), U)
    # other geometry than 3 x 3 / stride 1 / pad 1 has no halo kernel
    assert not ops.conv_h2_px_supported((4, 64, 64, 192), (768, 1, 1, 192), 1, 0, S)
    assert not ops.conv_h2_px_supported((4, 64, 64, 192), (768, 3, 3, 192), 2, 1, S)


def test_gdn_gate():
    from hipops import ops
    assert ops.gdn_fwd_bwd_px_supported((1, 16, 16, 192)) and ops.gdn_fwd_bwd_px_supported((4, 128, 128, 192))
    assert not ops.gdn_fwd_bwd_px_supported((1, 15, 16, 192)) and not ops.gdn_fwd_bwd_px_supported((4, 16, 18, 128))
    assert not ops.gdn_fwd_bwd_px_supported((1, 6, 6, 192))                        # 36 tokens: no whole tile of 64


def test_pixel_unshuffle2_refuses_odd_sizes():
    """[B,2H,2W,C] -> [B,H,W,4C]: an odd height or width has no r = 2 unshuffle (the wrapper used to drop the last row / column); refused
    before any pointer is taken, so a CPU tensor gets this far"""
    import pytest
    import torch
    from hipops import ops
    for shape in ((1, 5, 4, 16), (1, 4, 7, 16), (2, 3, 3, 4)):
        with pytest.raises(ValueError, match="pixel_unshuffle2"):
            ops.pixel_unshuffle2(torch.zeros(shape))
    with pytest.raises(RuntimeError, match="no CPU path"):       # even sizes pass the check and reach the operand check
        ops.pixel_unshuffle2(torch.zeros(1, 4, 6, 16), out=torch.zeros(1, 2, 3, 64))


def test_bad_arguments_are_refused_before_any_launch():
    from hipops import _lib as L
    from hipops import ops
    h = L.lib()
    p = C.c_void_p(4096)            # never dereferenced: every case below is refused on the host
    d = ops.conv_desc((4, 64, 64, 192), (768, 3, 3, 192), 1, 1)

    def conv(desc=d, pre=None, mode=1, out=p):
        return h.rdo_conv2d_fwd_h2_px(C.byref(desc), p, 1.0, p, 1.0, None, None, None, None, out, pre, None, 1.0, None, 0, mode, None)

    assert conv(pre=p) == RDO_EINVAL and b"rdo_conv2d_fwd_h2_px" in h.rdo_last_error()
    assert conv(mode=3) == RDO_EINVAL and conv(mode=-1) == RDO_EINVAL
    assert conv(desc=ops.conv_desc((4, 64, 64, 192), (320, 3, 3, 192), 1, 1)) == RDO_EINVAL
    assert conv(desc=ops.conv_desc((4, 64, 64, 192), (192, 3, 3, 192), 1, 1), mode=2, pre=p) == RDO_EINVAL
    assert conv(out=None) == RDO_EINVAL
    assert h.rdo_split_h2_conv_px(p, 770, 3, 3, 32, 1.0, p, 4, None) == RDO_EINVAL and b"rdo_split_h2_conv_px" in h.rdo_last_error()
    assert h.rdo_split_h2_conv_px(p, 768, 3, 3, 32, 1.0, p, 2, None) == RDO_EINVAL
    assert h.rdo_split_h2_conv_px(p, 768, 3, 3, 32, 3.0, p, 4, None) == RDO_EINVAL

    def gdn(dup=p, dup_scale=1.0, H=16, W=16, Cc=192):
        return h.rdo_gdn_fwd_bwd_px(p, p, p, 128.0, p, None, p, p, p, 1, H, W, Cc, 2.0, 1, None, dup, dup_scale, None, p, None, None, 1.0, None, None)

    for kw in (dict(dup=None), dict(dup=C.c_void_p(4100)), dict(dup_scale=3.0), dict(dup_scale=0.0), dict(H=15), dict(W=6, H=6), dict(Cc=128)):
        assert gdn(**kw) == RDO_EINVAL, kw
        assert b"rdo_gdn_fwd_bwd_px" in h.rdo_last_error()

    # rows in 4 groups: a conv layout in quads (the tile form), fp16 forward planes, not the gradient-only mode
    def step(rows=64, cin=16, mode=0, groups=4, planes=p, pscale=1.0):
        it = L.AdaStepItem()
        it.d = L.AdaDesc(rows * cin, rows, 256, 0, 0.0, 0.0, 1, 1, cin)
        it.w = it.delta = it.zp = it.slabs = it.alpha = it.adam_m = it.adam_v = it.wq = it.dalpha = 4096
        it.nsplit, it.wq_planes, it.wq_plane_scale = 1, (planes.value if planes else None), pscale
        rg = (C.c_int32 * 1)(groups)
        return h.rdo_adaround_step_batch_gather_px(C.byref(it), 1, mode, 1.0, 0.01, p, p, None, None, None, rg, None)

    for kw in (dict(mode=1), dict(groups=2), dict(rows=66, cin=16), dict(rows=64, cin=2), dict(pscale=0.0)):
        assert step(**kw) == RDO_EINVAL, kw
        assert b"rdo_adaround_step_batch_gather_px" in h.rdo_last_error()
