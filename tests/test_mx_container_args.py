"""CPU checks of the packed MX container: include/rdo_ptq_mxfile.h against `EXPORTS_MXFILE` and the built library, `rdo_mx_row_bytes`,
the refusals of the C entries (RDO_EINVAL without touching a device) and of the `ops` wrappers, the reference's own properties
(tests/mx_container_reference.py: it inverts itself and equals tests/mx_gemm_reference.py's packing on whole blocks), the on-grid
idempotence that lets a plain `MXQuantizer` stand on the loading side (tests/mx_reference.py over every grid value of every format as
the block maximum), and what `save_mx_packed` / `load_mx_packed` refuse without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mx_container_reference as F
import mx_gemm_reference as G
import mx_reference as R
from test_rd_report_args import _toy

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rdo_mx_row_bytes", "rdo_mx_pack_rows", "rdo_mx_unpack_dequant"}


# ----------------------------------------------------------------------------- the header, the exports
def test_header_matches_the_export_table_and_the_library():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_mxfile.h")).read()
    declared = set(re.findall(r"^int(?:32_t|64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == set(L.EXPORTS_MXFILE) == NAMES
    assert '#include "rdo_ptq_mx.h"' in hdr
    h = L.lib()
    others = (L.EXPORTS, L.EXPORTS_GDN, L.EXPORTS_BIAS, L.EXPORTS_BITS, L.EXPORTS_PACK, L.EXPORTS_SUBPEL, L.EXPORTS_ACTBITS, L.EXPORTS_ATTNQ,
              L.EXPORTS_MX, L.EXPORTS_MXROUND, L.EXPORTS_MXGEMM, L.EXPORTS_MXCONV, L.EXPORTS_MXTCONV)
    for name in declared:
        assert hasattr(h, name) and not any(name in table for table in others)
    assert [len(t) for t in others] == [124, 2, 4, 2, 3, 6, 2, 2, 4, 4, 5, 2, 2]


def test_row_bytes():
    from hipops import _lib as L
    h = L.lib()
    for fmt in R.NAMES:
        fid, bits = L.MX_FORMATS[fmt]
        assert bits == R.element_bits(fmt) == h.rdo_mx_format_bits(fid)
        for inner in (1, 5, 27, 31, 32, 33, 64, 75, 101, 288, 2 ** 31 + 1, 2 ** 45):
            assert h.rdo_mx_row_bytes(inner, fid) == -(-inner // 32) * 4 * bits == F.row_bytes(inner, fmt), (fmt, inner)
        assert h.rdo_mx_row_bytes(96, fid) * 3 == h.rdo_mx_packed_bytes(3, 96, fid)
        assert h.rdo_mx_row_bytes(2 ** 62 - 1, fid) == 2 ** 57 * 4 * bits             # (no overflow in the rounding up)
        assert h.rdo_mx_row_bytes(2 ** 63 - 1, fid) == (2 ** 58 * 4 * bits if bits < 8 else 0)      # 2^63 bytes are beyond int64_t
        for inner in (0, -1, -32):
            assert h.rdo_mx_row_bytes(inner, fid) == 0
    assert h.rdo_mx_row_bytes(32, -1) == 0 and h.rdo_mx_row_bytes(32, 5) == 0


def test_c_entries_refuse_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    odd = C.c_void_p(C.addressof(buf) + 2)

    def refused(fn, names, base, bad, who):
        for kw in bad:
            a = dict(base, **kw)
            assert fn(*[a[n] for n in names], None) == RDO_EINVAL, (who, kw)
            assert h.rdo_last_error().startswith(who.encode() + b": "), (who, kw, h.rdo_last_error())

    sizes = [dict(rows=0), dict(rows=-3), dict(inner=0), dict(inner=-32), dict(format=-1), dict(format=5),
             dict(rows=2 ** 31 - 1, inner=2 ** 40), dict(rows=2 ** 20, inner=2 ** 25 + 1)]
    refused(h.rdo_mx_pack_rows, ["codes", "rows", "inner", "format", "packed"], dict(codes=p, rows=3, inner=75, format=0, packed=p),
            [dict(codes=None), dict(packed=None), dict(packed=odd)] + sizes, "rdo_mx_pack_rows")
    refused(h.rdo_mx_unpack_dequant, ["packed", "scales", "rows", "inner", "format", "w", "codes"],
            dict(packed=p, scales=p, rows=3, inner=75, format=2, w=p, codes=p),
            [dict(packed=None), dict(scales=None), dict(w=None, codes=None), dict(packed=odd), dict(w=odd)] + sizes, "rdo_mx_unpack_dequant")


@pytest.fixture()
def no_library(monkeypatch):
    """any library call or pointer conversion after the argument checks fails the test"""
    from hipops import _lib as L
    from hipops import ops

    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(L, "lib", boom)
    monkeypatch.setattr(ops, "_ptr", boom)
    return ops


def test_wrappers_refuse_malformed_operands(no_library):
    ops = no_library
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    cases = [
        (ops.mx_pack_rows, (torch.zeros(3, 75), "mxfp4"), {}, "mx_pack_rows: codes must be an uint8 tensor"),
        (ops.mx_pack_rows, (u8(225), "mxfp4"), {}, "mx_pack_rows: .*rank 2"),
        (ops.mx_pack_rows, (u8(3, 150)[:, ::2], "mxfp4"), {}, "mx_pack_rows: .*contiguous"),
        (ops.mx_pack_rows, (u8(3, 75), "fp4"), {}, "mx_pack_rows: unknown MX format 'fp4'; the formats are"),
        (ops.mx_pack_rows, (u8(0, 75), "mxfp4"), {}, "mx_pack_rows: codes is empty"),
        (ops.mx_pack_rows, (u8(3, 75), "mxfp4"), {}, "mx_pack_rows: .*no CPU path"),
        (ops.mx_unpack_dequant, (torch.zeros(3, 48), u8(3, 3), 75, "mxfp4"), {}, "mx_unpack_dequant: packed must be an uint8 tensor"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 3), 75, "mxfp5"), {}, "mx_unpack_dequant: unknown MX format 'mxfp5'"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 3), 0, "mxfp4"), {}, "mx_unpack_dequant: inner"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 3), 75, "mxfp6_e2m3"), {}, "mx_unpack_dequant: packed is \\(3, 48\\); a row of inner 75 in mxfp6_e2m3 has 72 bytes"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 2), 75, "mxfp4"), {}, "mx_unpack_dequant: scales must be a contiguous uint8 \\[3, 3\\]"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 3), 75, "mxfp4"), dict(want=()), "mx_unpack_dequant: want must hold at least one"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 3), 75, "mxfp4"), dict(want="w"), "mx_unpack_dequant: want must be a sequence of names out of \\['w', 'codes'\\]"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 3), 75, "mxfp4"), dict(want=("w", "wq")), "mx_unpack_dequant: want must hold"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 3), 75, "mxfp4"), dict(want=("w", "w")), "mx_unpack_dequant: want must hold"),
        (ops.mx_unpack_dequant, (u8(3, 48), u8(3, 3), 75, "mxfp4"), dict(want=("w", "codes")), "mx_unpack_dequant: .*no CPU path"),
    ]
    for fn, args, kw, what in cases:
        with pytest.raises(ValueError, match=what):
            fn(*args, **kw)


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("fmt", R.NAMES)
def test_reference_inverts_itself_and_equals_the_operand_packing_on_whole_blocks(fmt):
    b = R.element_bits(fmt)
    for k, (rows, inner) in enumerate(F.SHAPES + ((2, 31), (2, 32), (1, 96))):
        codes, scales = F.random_case(rows, inner, fmt, seed=k)
        assert int(codes.max()) >= (1 << b) or b == 8                               # garbage in the upper bits
        assert (scales == 255).sum() == 1
        packed = F.pack_rows(codes, fmt)
        assert packed.shape == (rows, F.row_bytes(inner, fmt)) and packed.dtype == np.uint8
        low = codes & ((1 << b) - 1)
        assert (F.unpack_rows(packed, inner, fmt) == low).all()
        # the padding of a short last block is zero bits; a whole number of blocks has none
        pad = np.zeros((rows, R.blocks(inner) * 32), np.uint8)
        pad[:, :inner] = low
        assert (packed == G.pack(pad, fmt)).all()
        if inner % 32 == 0:
            assert (packed == G.pack(codes & ((1 << b) - 1), fmt)).all() and (G.unpack(packed, inner, fmt) == low).all()
        # element j of block kb at bits [j b, (j + 1) b) of the block's little-endian bit string
        for r, i in ((0, 0), (rows - 1, inner - 1), (rows // 2, inner // 2)):
            blk = packed[r, (i // 32) * 4 * b:(i // 32 + 1) * 4 * b]
            assert (int.from_bytes(blk.tobytes(), "little") >> ((i % 32) * b)) & ((1 << b) - 1) == int(low[r, i])
        w, c = F.decode_rows(packed, scales, inner, fmt)
        want = R.dequantize(torch.from_numpy(low), torch.from_numpy(scales), fmt).numpy()
        assert (c == low).all() and (w.view(np.uint32) == want.view(np.uint32)).all()
        nan = np.repeat(scales == 255, 32, axis=1)[:, :inner]
        assert nan.any() and np.isnan(w[nan]).all() and not np.isnan(w[~nan]).any()


# ----------------------------------------------------------------------------- on-grid idempotence
@pytest.mark.parametrize("fmt", R.NAMES)
def test_round_to_nearest_gives_an_on_grid_block_and_its_scale_back(fmt):
    """What `load_mx_packed` relies on (the docstring of quantization/mx_packed.py): a stored block -- grid values times 2^E whose largest
    magnitude is a grid value in [2^emax, max], or any grid value under E = -127 -- quantises to itself, scale byte included.  Every
    such largest value of the format, at several E with -127 and the largest E among them, in a whole block and in a short one."""
    _, eb, M, bias, emax, vmax = R.FORMATS[fmt]
    b = 1 + eb + M
    sign = 1 << (b - 1)
    mags = G.finite_codes(fmt)
    mags = mags[mags < sign]                                                        # magnitude codes 0 .. max code
    vals = G.decode_elements(mags, fmt)
    assert vals[0] == 0.0 and vals.max() == vmax and (np.diff(vals) > 0).all()      # the codes are monotone in the magnitude
    rng = np.random.default_rng(5)
    inner = 32 + 7
    counter_examples = []
    for E in (-127, -126, -100, -1, 0, 9, 127 - emax):
        tops = mags if E == -127 else mags[vals >= 2.0 ** emax]
        assert len(tops) == (len(mags) if E == -127 else 2 ** M - (fmt == "mxfp8_e4m3"))       # the top binade (E4M3: less its NaN)
        codes = np.zeros((len(tops), inner), np.uint8)
        for r, top in enumerate(tops):
            row = rng.integers(0, int(top) + 1, inner).astype(np.uint8)            # magnitudes <= the top's
            row[[3, 35]] = top                                                      # the maximum of either block
            codes[r] = row | (rng.integers(0, 2, inner).astype(np.uint8) * sign)
        scales = np.full((len(tops), 2), E + 127, np.uint8)
        w = R.dequantize(torch.from_numpy(codes), torch.from_numpy(scales), fmt)
        assert torch.isfinite(w).all()
        q = R.quantize(w, fmt)
        same_w = (q["wq"].numpy().view(np.uint32) == w.numpy().view(np.uint32)).all(axis=1)
        zero = tops == 0                                                            # an all-zero block: E = -127 on both sides
        same_s = (q["scales"].numpy() == scales).all(axis=1) | (zero & (q["scales"].numpy() == 0).all(axis=1) & (E == -127))
        nonzero = (codes & (sign - 1)) != 0                                         # (the code of a zero keeps only its sign)
        same_c = ((q["codes"].numpy() == codes) | ~nonzero).all(axis=1)
        counter_examples += [(fmt, E, int(t)) for t, ok in zip(tops, same_w & same_s & same_c) if not ok]
    assert counter_examples == []


# ----------------------------------------------------------------------------- save / load without a GPU
def _reference_file(qnn, path, fmt_of):
    """an MX container of a CPU model written by the references alone (tests/mx_reference.py, mx_container_reference.py)"""
    from collections import OrderedDict
    from quantization import QuantModule, packed_io
    from quantization.quantizer import to_rows
    entries, arrays = [], OrderedDict()
    mods = [(n, m) for n, m in qnn.named_modules() if isinstance(m, QuantModule) and m.org_weight is not None]
    for k, (name, m) in enumerate(mods):
        fmt = fmt_of(k)
        wr = to_rows(m.weight.detach(), m.if_tconv)
        wr = wr.reshape(wr.shape[0], -1)
        q = R.quantize(wr, fmt)
        sc = q["scales"].numpy().reshape(-1)
        arrays[f"{name}/packed"] = F.pack_rows(q["codes"].numpy(), fmt).view(np.uint32)
        arrays[f"{name}/scales"] = np.concatenate([sc, np.zeros(-sc.size % 4, np.uint8)]).view(np.uint32)
        e = OrderedDict(name=name, grid="mx", fmt=fmt, rounding="nearest", kind=m.kind, shape=list(m.weight.shape), tconv=bool(m.if_tconv),
                        rows=int(wr.shape[0]), inner=int(wr.shape[1]), trained=False, disable_act_quant=bool(m.disable_act_quant),
                        mx_activations=None, packed={"ref": f"{name}/packed"}, scales={"ref": f"{name}/scales"}, bias=None)
        if m.bias is not None:
            arrays[f"{name}/bias"] = m.bias.detach().numpy()
            e["bias"] = {"ref": f"{name}/bias"}
        entries.append(e)
    from quantization import BaseQuantBlock
    header = OrderedDict(container="mx", modules=[], mx_modules=entries, order=[n for n, _ in mods],
                         blocks=OrderedDict((n, False) for n, b in qnn.named_modules() if isinstance(b, BaseQuantBlock)),
                         act_quantizers=OrderedDict((n, {"act_mode": "dynamic", "dynamic_bits": 8}) for n, _ in qnn.act_quantizers()), totals={})
    packed_io.write_packed(path, header, arrays)
    return header


def _state(qnn):
    return [(k, v.clone()) for k, v in qnn.state_dict().items()], [(n, id(m.weight_quantizer)) for n, m in qnn.named_modules() if hasattr(m, "weight_quantizer")]


def _same_state(a, b):
    assert a[1] == b[1] and [k for k, _ in a[0]] == [k for k, _ in b[0]]
    for (k, s), (_, t) in zip(a[0], b[0]):
        assert s.dtype == t.dtype and s.shape == t.shape and torch.equal(s.reshape(-1).view(torch.uint8), t.reshape(-1).view(torch.uint8)), k


def test_save_and_load_refuse_without_a_gpu(tmp_path, no_library):
    from quantization import packed_io
    qnn = _toy("cheng")
    qnn.set_weight_format("mxfp4")
    path = os.path.join(tmp_path, "toy.rdomx")
    with pytest.raises(ValueError, match="save_mx_packed: module\\(s\\) \\['model.g_a.0.* are not on the GPU; there is no CPU path; nothing was written"):
        qnn.save_mx_packed(path)
    assert os.listdir(tmp_path) == []
    qnn.set_weight_format("int")
    before = _state(qnn)
    # no file, no container, a container of another kind
    with pytest.raises(OSError):
        qnn.load_mx_packed(path)
    with open(path, "wb") as f:
        f.write(b"RDOPACK1" + b"\0" * 5)
    with pytest.raises(ValueError, match="read_packed: .*wrong magic"):
        qnn.load_mx_packed(path)
    packed_io.write_packed(path, {"modules": [], "blocks": {}, "act_quantizers": {}, "totals": {}}, {})
    with pytest.raises(ValueError, match="load_mx_packed: .* is a packed checkpoint without \"container\": \"mx\": `load_packed` takes what `save_packed` wrote"):
        qnn.load_mx_packed(path)
    packed_io.write_packed(path, {"container": "mx", "modules": []}, {})
    with pytest.raises(ValueError, match="load_mx_packed: .*malformed header: KeyError\\('mx_modules'\\)"):
        qnn.load_mx_packed(path)
    # a file of the references for this very model fits: the one refusal left is the device
    header = _reference_file(qnn, path, lambda k: R.NAMES[k % 5])
    assert {e["inner"] % 32 for e in header["mx_modules"]} != {0}
    with pytest.raises(ValueError, match="load_mx_packed: module\\(s\\) \\['model.g_a.0.* are not on the GPU; there is no CPU path"):
        qnn.load_mx_packed(path)
    # ... and a trained target, or one that stands on MX quantisers, is refused before that
    first = next(m for m in qnn.modules() if hasattr(m, "weight_quantizer") and m.org_weight is not None)
    first.trained = True
    with pytest.raises(ValueError, match="load_mx_packed: the target holds trained module\\(s\\) \\['model.g_a.0"):
        qnn.load_mx_packed(path)
    first.trained = False
    qnn.set_weight_format({"h_s.8": "mxfp8_e4m3"})
    with pytest.raises(ValueError, match="load_mx_packed: the target holds MX quantiser\\(s\\) on module\\(s\\) \\['model.h_s.8"):
        qnn.load_mx_packed(path)
    qnn.set_weight_format("int")
    # every difference is listed: a model of another width, and entries that are wrong in themselves
    other = _toy("cheng")
    names = [e["name"] for e in header["mx_modules"]]
    edits = {0: dict(kind="linear"), 1: dict(fmt="mxfp5"), 2: dict(rows=1), 3: dict(tconv=True), 4: dict(mx_activations=["mxfp4", "fused"]),
             5: dict(name="model.g_a.77")}

    def edited(h):
        for k, kw in edits.items():
            h["mx_modules"][k].update(kw)
        h["order"][5] = "model.g_a.77"
        h["blocks"]["model.g_a.99"] = True
        return h
    hdr, arrays = packed_io.read_packed(path)
    for e in hdr["mx_modules"]:                                                     # back to plain references for the writer
        for f in ("packed", "scales", "bias"):
            if e[f] is not None:
                e[f] = {"ref": e[f]["ref"]}
    bad = os.path.join(tmp_path, "bad.rdomx")
    packed_io.write_packed(bad, edited({k: v for k, v in hdr.items() if k not in ("version", "crc32", "payload_bytes")}), arrays)
    with pytest.raises(ValueError, match="load_mx_packed: .* does not fit this model: ") as err:
        other.load_mx_packed(bad)
    text = str(err.value)
    for want in ("module 'model.g_a.77' is in the file only", f"module {names[5]!r} is in the model only",
                 f"module {names[0]!r}: kind 'linear' in the file", f"module {names[1]!r}: unknown MX format 'mxfp5'",
                 f"module {names[2]!r}: rows x inner 1 x ", f"module {names[3]!r}: rows x inner .* \\(tconv True\\) in the file",
                 f"module {names[4]!r}: mx_activations \\['mxfp4', 'fused'\\] is no pair", "blocks \\['model.g_a.99'\\] are on one side only"):
        assert re.search(want, text), want
    _same_state(before, _state(qnn))
