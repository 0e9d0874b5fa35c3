"""CPU-only checks of the one-launch GDN block's C entry points (include/rdo_ptq_gdn.h): declared, exported, bound; the shape
predicate; arguments refused before any launch."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDO_EINVAL = -22


def test_header_declares_and_library_exports_the_entries():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_gdn.h")).read()
    declared = set(re.findall(r"^int (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == {"rdo_gdn_fwd_bwd", "rdo_gdn_fwd_bwd_supported"} == set(L.EXPORTS_GDN)
    assert re.search(r"^int rdo_gdn_fwd_bwd\(const float\* c, const void\* fwd_planes, const void\* bwd_planes, float wscale,", hdr, re.M)
    h = L.lib()
    for name in declared:
        assert hasattr(h, name) and name not in L.EXPORTS


def test_supported_shapes():
    from hipops import _lib as L
    h = L.lib()
    for M in (64, 256, 4096, 16384, 65536, 32960):
        assert h.rdo_gdn_fwd_bwd_supported(M, 192) == 1
    for M, Cc in ((0, 192), (-64, 192), (96, 192), (65, 192), (64, 128), (64, 96), (64, 384), (2 ** 40, 192)):
        assert h.rdo_gdn_fwd_bwd_supported(M, Cc) == 0, (M, Cc)


def test_bad_arguments_are_refused_before_any_launch():
    from hipops import _lib as L
    h = L.lib()
    p = C.c_void_p(4096)            # never dereferenced: every case below is refused on the host

    def call(c=p, fwd=p, bwd=p, wscale=128.0, beta=p, tgt=p, idx=p, it=p, B=1, per_image=64 * 192, Cc=192, t=p, dx_planes=None, dx_scale=1.0):
        return h.rdo_gdn_fwd_bwd(c, fwd, bwd, wscale, beta, None, tgt, idx, it, B, per_image, Cc, 2.0, 0, None, None, t, None, dx_planes, dx_scale,
                                 None, None)

    bad = [dict(c=None), dict(fwd=None), dict(bwd=None), dict(beta=None), dict(tgt=None), dict(idx=None), dict(it=None), dict(t=None),
           dict(B=0), dict(per_image=0), dict(per_image=64 * 192 + 1), dict(Cc=0), dict(Cc=128, per_image=64 * 128), dict(per_image=96 * 192),
           dict(wscale=3.0), dict(wscale=0.0), dict(dx_planes=p, dx_scale=0.0), dict(c=C.c_void_p(4100))]
    for kw in bad:
        assert call(**kw) == RDO_EINVAL, kw
        assert b"rdo_gdn_fwd_bwd" in h.rdo_last_error()
