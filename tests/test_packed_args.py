"""CPU checks of the packed checkpoint: include/rdo_ptq_pack.h declares exactly the entries of `EXPORTS_PACK`, the C entries return
RDO_EINVAL with a message that names them for every refusal without touching a device, `rdo_pack_row_words` counts as stated,
`ops.weight_pack` / `ops.weight_unpack` refuse malformed operands with ValueError before any pointer is taken, `packed_io` round-trips
hand-made entries (the bit layout judged by the bit-string reference of tests/packed_reference.py) and refuses every corruption with its
reason, and `save_packed` refuses before anything is packed or written."""
import ctypes as C
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

from packed_reference import pack_rows, row_words, unpack_rows
from test_rd_report_args import _toy

RDO_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rdo_weight_pack", "rdo_weight_unpack", "rdo_pack_row_words"}


# ----------------------------------------------------------------------------- the header, the exports
def test_header_declares_and_library_exports_the_entries():
    from hipops import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rdo_ptq_pack.h")).read()
    declared = set(re.findall(r"^int(?:64_t)? (rdo_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == NAMES == set(L.EXPORTS_PACK)
    assert '#include "rdo_ptq_hip.h"' in hdr
    for name, value in (("MIN_BITS", L.PACK_MIN_BITS), ("MAX_BITS", L.PACK_MAX_BITS)):
        assert int(re.search(rf"^#define RDO_PACK_{name} (\d+)", hdr, re.M).group(1)) == value
    from quantization.quantizer import MAX_BITS
    assert (L.PACK_MIN_BITS, L.PACK_MAX_BITS) == (2, MAX_BITS)
    h = L.lib()
    for name in declared:
        assert hasattr(h, name)
        assert name not in L.EXPORTS and name not in L.EXPORTS_GDN and name not in L.EXPORTS_BIAS and name not in L.EXPORTS_BITS
    assert len(L.EXPORTS) == 124


# ----------------------------------------------------------------------------- the C entries
def test_c_entries_refuse_bad_arguments_without_a_device():
    """RDO_REQUIRE runs before any launch: the non-null arguments below are host addresses that are never dereferenced"""
    from hipops import _lib as L
    h = L.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    odd = C.c_void_p(C.addressof(buf) + 2)
    geometry = [dict(rows=0), dict(rows=-3), dict(inner=0), dict(inner=-40), dict(bits=1), dict(bits=17), dict(bits=0), dict(bits=-8),
                dict(bits=32), dict(packed=None), dict(packed=odd), dict(delta=None), dict(zp=None),
                dict(rows=2 ** 31 - 1, inner=2 ** 30, bits=2),           # W = 2^26: rows * W above 2^40 words
                dict(rows=1, inner=2 ** 36, bits=16)]                    # W above 2^31 - 1

    def pack(**kw):
        a = dict(w=p, alpha=None, delta=p, zp=p, rows=3, inner=40, bits=5, packed=p)
        a.update(kw)
        return h.rdo_weight_pack(*[a[n] for n in ("w", "alpha", "delta", "zp", "rows", "inner", "bits", "packed")], None)

    def unpack(**kw):
        a = dict(packed=p, delta=p, zp=p, rows=3, inner=40, bits=5, levels=p, wq=p)
        a.update(kw)
        return h.rdo_weight_unpack(*[a[n] for n in ("packed", "delta", "zp", "rows", "inner", "bits", "levels", "wq")], None)

    for kw in geometry + [dict(w=None)]:
        assert pack(**kw) == RDO_EINVAL, kw
        assert b"rdo_weight_pack" in h.rdo_last_error(), kw
    for kw in geometry + [dict(levels=None, wq=None), dict(levels=None, delta=None), dict(levels=None, zp=None)]:
        assert unpack(**kw) == RDO_EINVAL, kw
        assert b"rdo_weight_unpack" in h.rdo_last_error(), kw


def test_row_words():
    from hipops import _lib as L
    from hipops import ops
    words = L.lib().rdo_pack_row_words
    for (inner, bits), want in {(1, 2): 1, (16, 2): 1, (17, 2): 2, (13, 5): 3, (1728, 3): 162, (32, 16): 16}.items():
        assert words(inner, bits) == want == row_words(inner, bits) == ops.pack_row_words(inner, bits), (inner, bits)
    for args in ((0, 5), (-1, 5), (40, 1), (40, 17), (40, 0), (40, -3), (2 ** 36, 16), (2 ** 62, 2)):
        assert words(*args) == 0, args
    assert words((2 ** 31 - 1) * 2, 16) == 2 ** 31 - 1 and words((2 ** 31 - 1) * 2 + 1, 16) == 0


# ----------------------------------------------------------------------------- the wrappers
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


def _t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_weight_pack_refuses_malformed_operands(no_library):
    ops = no_library
    w, d, z = _t(3, 40), _t(3), _t(3)
    cases = [
        ((w.double(), d, z, 5), {}, "w_rows must be an fp32 tensor"),
        ((None, d, z, 5), {}, "w_rows must be an fp32 tensor"),
        ((_t(120), d, z, 5), {}, "rank 2"),
        ((_t(3, 4, 10), d, z, 5), {}, "rank 2"),
        ((_t(0, 40), _t(0), _t(0), 5), {}, "empty"),
        ((_t(3, 0), d, z, 5), {}, "empty"),
        ((_t(3, 80)[:, ::2], d, z, 5), {}, "contiguous"),
        ((_t(40, 3).t(), d, z, 5), {}, "contiguous"),
        ((w, d, z, 1), {}, "whole number in 2 .. 16"),
        ((w, d, z, 17), {}, "whole number in 2 .. 16"),
        ((w, d, z, 5.0), {}, "whole number in 2 .. 16"),
        ((w, d, z, True), {}, "whole number in 2 .. 16"),
        ((w, d, z, "5"), {}, "whole number in 2 .. 16"),
        ((w, d, z, None), {}, "whole number in 2 .. 16"),
        ((w, _t(4), z, 5), {}, "delta must be a contiguous fp32 \\[3\\]"),
        ((w, _t(3, 1), z, 5), {}, "delta must be a contiguous fp32 \\[3\\]"),
        ((w, d, _t(2), 5), {}, "zp must be a contiguous fp32 \\[3\\]"),
        ((w, d.double(), z, 5), {}, "delta must be a contiguous fp32"),
        ((w, d, _t(6)[::2], 5), {}, "zp must be a contiguous fp32"),
        ((w, d, torch.zeros(3, device="meta"), 5), {}, "zp must be a contiguous fp32"),
        ((w, 0.1, z, 5), {}, "delta must be a contiguous fp32"),
        ((w, d, z, 5), {"alpha_rows": _t(3, 41)}, "alpha_rows must be a contiguous fp32 \\[3, 40\\]"),
        ((w, d, z, 5), {"alpha_rows": _t(2, 40)}, "alpha_rows must be a contiguous fp32 \\[3, 40\\]"),
        ((w, d, z, 5), {"alpha_rows": _t(3, 40).double()}, "alpha_rows must be a contiguous fp32"),
        ((w, d, z, 5), {"out": _t(3, 7, dtype=torch.int32)[:, :6]}, "out must be a contiguous int32"),
        ((w, d, z, 5), {"out": _t(3, 7)}, "out must be a contiguous int32 \\[3, 7\\]"),
        ((w, d, z, 5), {"out": _t(3, 6, dtype=torch.int32)}, "out must be a contiguous int32 \\[3, 7\\]"),
        ((torch.zeros(2 ** 31 - 1, 2 ** 30, device="meta"), torch.zeros(2 ** 31 - 1, device="meta"), torch.zeros(2 ** 31 - 1, device="meta"), 2),
         {}, "2\\^40 words"),
        ((w, d, z, 5), {}, "no CPU path"),
        ((w, d, z, np.int64(16)), {"alpha_rows": _t(3, 40)}, "no CPU path"),          # numpy integers count
        ((_t(1, 1), _t(1), _t(1), 2), {"out": _t(1, 1, dtype=torch.int32)}, "no CPU path"),
    ]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=f"weight_pack: .*{what}"):
            ops.weight_pack(*args, **kw)


def test_weight_unpack_refuses_malformed_operands(no_library):
    ops = no_library
    i32 = torch.int32
    pk, d, z = _t(3, 7, dtype=i32), _t(3), _t(3)                                      # 40 codes of 5 bits: 200 bits, W = 7
    cases = [
        ((pk.float(), d, z, 40, 5), {}, "packed must be an int32 tensor"),
        ((None, d, z, 40, 5), {}, "packed must be an int32 tensor"),
        ((pk.long(), d, z, 40, 5), {}, "packed must be an int32 tensor"),
        ((_t(21, dtype=i32), d, z, 40, 5), {}, "rank 2"),
        ((_t(0, 7, dtype=i32), _t(0), _t(0), 40, 5), {}, "empty"),
        ((_t(3, 14, dtype=i32)[:, ::2], d, z, 40, 5), {}, "contiguous"),
        ((pk, d, z, 40, 1), {}, "bits must be a whole number in 2 .. 16"),
        ((pk, d, z, 40, 17), {}, "bits must be a whole number in 2 .. 16"),
        ((pk, d, z, 40, 5.0), {}, "bits must be a whole number in 2 .. 16"),
        ((pk, d, z, 40, False), {}, "bits must be a whole number in 2 .. 16"),
        ((pk, d, z, 0, 5), {}, "inner must be a whole number >= 1"),
        ((pk, d, z, 40.0, 5), {}, "inner must be a whole number >= 1"),
        ((pk, d, z, True, 5), {}, "inner must be a whole number >= 1"),
        ((pk, d, z, 45, 5), {}, "W = 8 words a row"),
        ((pk, d, z, 38, 5), {}, "W = 6 words a row"),
        ((pk, d, z, 40, 6), {}, "W = 8 words a row"),
        ((pk, d, z, 40, 5), {"levels": False, "dequant": False}, "one of them True"),
        ((pk, d, z, 40, 5), {"levels": 1}, "must be True or False"),
        ((pk, _t(4), z, 40, 5), {}, "delta must be a contiguous fp32 \\[3\\]"),
        ((pk, d, _t(3, 1), 40, 5), {}, "zp must be a contiguous fp32 \\[3\\]"),
        ((pk, None, z, 40, 5), {}, "delta must be a contiguous fp32"),
        ((pk, d, None, 40, 5), {}, "zp must be a contiguous fp32"),
        ((pk, None, z, 40, 5), {"dequant": False}, "delta must be a contiguous fp32"),    # given, they must fit
        ((pk, d, torch.zeros(3, device="meta"), 40, 5), {}, "zp must be a contiguous fp32"),
        ((pk, d, z, 40, 5), {"levels_out": _t(3, 40)}, "levels_out must be a contiguous int32 \\[3, 40\\]"),
        ((pk, d, z, 40, 5), {"levels_out": _t(3, 39, dtype=i32)}, "levels_out must be a contiguous int32 \\[3, 40\\]"),
        ((pk, d, z, 40, 5), {"wq_out": _t(3, 40, dtype=i32)}, "wq_out must be a contiguous fp32 \\[3, 40\\]"),
        ((pk, d, z, 40, 5), {"wq_out": _t(3, 80)[:, ::2]}, "wq_out must be a contiguous fp32"),
        ((pk, d, z, 40, 5), {"levels": False, "levels_out": _t(3, 40, dtype=i32)}, "levels_out is given but levels is False"),
        ((pk, None, None, 40, 5), {"dequant": False, "wq_out": _t(3, 40)}, "wq_out is given but dequant is False"),
        ((pk, d, z, 40, 5), {}, "no CPU path"),
        ((pk, None, None, 40, 5), {"dequant": False}, "no CPU path"),
        ((pk, d, z, np.int64(40), np.int32(5)), {"levels": False}, "no CPU path"),
    ]
    for args, kw, what in cases:
        with pytest.raises(ValueError, match=f"weight_unpack: .*{what}"):
            ops.weight_unpack(*args, **kw)


# ----------------------------------------------------------------------------- the container
def _entries(seed=3):
    """two hand-made modules (a 5-bit [3, 13] one with a bias, a 16-bit per-tensor [1, 7] one without), a block, a frozen quantiser with
    two sites and a dynamic one -> (header entries, arrays, the levels)"""
    g = np.random.default_rng(seed)
    levels = {"a": g.integers(0, 32, (3, 13)), "b": g.integers(0, 65536, (1, 7))}
    levels["a"][0, :3], levels["b"][0, -1] = (31, 0, 31), 65535
    arrays = {"a/packed": pack_rows(levels["a"], 5), "a/delta": g.random((3, 1), dtype=np.float32), "a/zero_point": np.float32([[3], [0], [17]]),
              "a/bias": g.standard_normal(3).astype(np.float32), "b/packed": pack_rows(levels["b"], 16),
              "b/delta": np.float32(0.25).reshape(()), "b/zero_point": np.float32(9).reshape(()),
              "q/range/0": np.float32([-1, -2, 3, 4]), "q/range/1": np.float32([0.5, 7])}
    mods = [dict(name="a", kind="linear", shape=[3, 13], tconv=False, rows=3, inner=13, n_bits=5, rounding="adaround", trained=True,
                 disable_act_quant=False, packed={"ref": "a/packed"}, delta={"ref": "a/delta"}, zero_point={"ref": "a/zero_point"},
                 bias={"ref": "a/bias"}),
            dict(name="b", kind="layernorm", shape=[7], tconv=False, rows=1, inner=7, n_bits=16, rounding="nearest", trained=False,
                 disable_act_quant=True, packed={"ref": "b/packed"}, delta={"ref": "b/delta"}, zero_point={"ref": "b/zero_point"}, bias=None)]
    acts = {"q": dict(act_mode="static", dynamic_bits=8, sites={"0": dict(channels=2, range={"ref": "q/range/0"}),
                                                                 "1": dict(channels=1, range={"ref": "q/range/1"})}),
            "p": dict(act_mode="dynamic", dynamic_bits=10)}
    entries = dict(modules=mods, blocks={"blk": True}, act_quantizers=acts,
                   totals=dict(modules=2, weights=46, size_bits=5 * 39 + 16 * 7, packed_bytes=4 * (3 * 3 + 4), padding_bits=3 * 31 + 16))
    return entries, arrays, levels


def _split(path):
    """the container restated: -> (header dict, payload bytes, byte offset of the payload)"""
    data = open(path, "rb").read()
    assert data[:8] == b"RDOPACK1"
    hlen, = struct.unpack("<Q", data[8:16])
    start = 16 + hlen + (-hlen) % 8
    assert start % 8 == 0 and set(data[16 + hlen:start]) <= {0}
    return json.loads(data[16:16 + hlen].decode("utf-8")), data[start:], start


def _compose(path, header, payload, crc=True):
    header = dict(header)
    if crc:
        header["crc32"], header["payload_bytes"] = zlib.crc32(payload), len(payload)
    text = json.dumps(header).encode("utf-8")
    with open(path, "wb") as f:
        f.write(b"RDOPACK1" + struct.pack("<Q", len(text)) + text + b"\0" * (-len(text) % 8) + payload)


def test_write_then_read_returns_the_arrays_and_the_header(tmp_path):
    from quantization import packed_io
    entries, arrays, levels = _entries()
    keep = json.dumps(entries)
    path = str(tmp_path / "toy.rdopack")
    header, file_bytes = packed_io.write_packed(path, entries, arrays)
    assert json.dumps(entries) == keep                                            # the caller's entries are not written to
    assert sorted(os.listdir(tmp_path)) == ["toy.rdopack"] and os.path.getsize(path) == file_bytes
    got_header, got = packed_io.read_packed(path)
    assert got_header == header and header["version"] == 1
    assert sorted(got) == sorted(arrays)
    for k, a in arrays.items():
        assert got[k].dtype == a.dtype and got[k].shape == a.shape and got[k].tobytes() == a.tobytes(), k
    # the container, restated by hand
    raw_header, payload, start = _split(path)
    assert raw_header == header and len(payload) == header["payload_bytes"] and start + len(payload) == file_bytes
    assert zlib.crc32(payload) == header["crc32"]
    assert [m["name"] for m in header["modules"]] == ["a", "b"] and header["blocks"] == {"blk": True}
    assert header["totals"] == entries["totals"] and header["act_quantizers"]["p"] == entries["act_quantizers"]["p"]
    spans = []
    for m in header["modules"]:
        for f in ("packed", "delta", "zero_point", "bias"):
            if m[f] is not None:
                spans.append((m[f], arrays[m[f]["ref"]]))
    for s in header["act_quantizers"]["q"]["sites"].values():
        spans.append((s["range"], arrays[s["range"]["ref"]]))
    assert len(spans) == len(arrays)
    end = 0
    for ref, a in spans:                                                          # in order, 8-byte aligned, little-endian, zero gaps
        off, length = ref["at"]
        assert off % 8 == 0 and off >= end and set(payload[end:off]) <= {0} and ref["shape"] == list(a.shape)
        assert ref["dtype"] == ("<u4" if a.dtype == np.uint32 else "<f4")
        assert payload[off:off + length] == a.astype(ref["dtype"]).tobytes()
        end = off + length
    assert set(payload[end:]) <= {0} and len(payload) - end < 8
    # the layout: the file's words unpack to the levels, the padding is zero, and bit j of a row is bit j % 8 of the row's byte j / 8
    for name, bits in (("a", 5), ("b", 16)):
        m = next(m for m in header["modules"] if m["name"] == name)
        off, length = m["packed"]["at"]
        rows, inner = m["rows"], m["inner"]
        W = row_words(inner, bits)
        assert length == 4 * rows * W and m["packed"]["shape"] == [rows, W]
        back, padding = unpack_rows(got[f"{name}/packed"], inner, bits)
        assert np.array_equal(back, levels[name]) and all(set(p) <= {"0"} for p in padding)
        for r in range(rows):
            row = payload[off + 4 * W * r:off + 4 * W * (r + 1)]
            for i in range(inner):
                code = sum(((row[(i * bits + t) // 8] >> ((i * bits + t) % 8)) & 1) << t for t in range(bits))
                assert code == levels[name][r, i]


def test_every_corruption_is_refused_with_its_reason(tmp_path):
    from quantization import packed_io
    entries, arrays, _ = _entries()
    good = str(tmp_path / "good.rdopack")
    packed_io.write_packed(good, entries, arrays)
    header, payload, start = _split(good)
    data = open(good, "rb").read()
    bad = str(tmp_path / "bad.rdopack")

    def refused(why):
        with pytest.raises(ValueError, match=f"read_packed: {re.escape(bad)}: .*{why}"):
            packed_io.read_packed(bad)

    def raw(b):
        with open(bad, "wb") as f:
            f.write(b)
    raw(b"RDOPACK2" + data[8:])
    refused("wrong magic")
    raw(b"")
    refused("wrong magic")
    raw(data[:8])
    refused("wrong magic")
    _compose(bad, dict(header, version=2), payload)
    refused("unknown version 2")
    raw(data[:8] + struct.pack("<Q", len(data)) + data[16:])
    refused("header length .* beyond the file")
    raw(data[:8] + struct.pack("<Q", 2 ** 63) + data[16:])
    refused("header length .* beyond the file")
    raw(data[:-1])
    refused("truncated payload")
    raw(data[:start])
    refused("truncated payload")
    raw(data + b"\0")
    refused("behind the payload")
    flipped = bytearray(data)
    flipped[start + header["modules"][0]["packed"]["at"][0]] ^= 1
    raw(bytes(flipped))
    refused("CRC mismatch")
    _compose(bad, dict(header, crc32=header["crc32"] ^ 1), payload, crc=False)
    refused("CRC mismatch")

    def edited(path_to, value):
        h = json.loads(json.dumps(header))
        node = h
        for k in path_to[:-1]:
            node = node[k]
        node[path_to[-1]] = value
        _compose(bad, h, payload)
    n = len(payload)
    b_at = header["modules"][1]["packed"]["at"]
    for at in ([n, 16], [n - 8, 16], [-8, 16], [b_at[0], n], [b_at[0] + 4, 16]):
        edited(("modules", 1, "packed", "at"), at)
        refused("outside the payload")
    edited(("act_quantizers", "q", "sites", "1", "range", "at"), [n + 8, 8])
    refused("outside the payload")
    edited(("modules", 0, "delta", "shape"), [4, 1])
    refused("are not a <f4 array of shape")
    edited(("modules", 0, "rows"), 4)
    refused("module 'a': packed holds 36 bytes, not 4 \\* rows \\* W = 4 \\* 4 \\* 3")
    edited(("modules", 0, "n_bits"), 4)
    refused("module 'a': packed holds 36 bytes, not 4 \\* rows \\* W = 4 \\* 3 \\* 2")
    edited(("modules", 1, "inner"), 9)
    refused("module 'b': packed holds 16 bytes")
    h = json.loads(json.dumps(header))
    del h["modules"][0]["packed"]
    _compose(bad, h, payload)
    refused("malformed header")
    raw(data[:16] + b"{" * (start - 16) + data[start:])
    refused("not a JSON object")
    _compose(bad, header, payload)                                                # and the file composed by hand from the same parts reads
    assert packed_io.read_packed(bad)[0] == header


def test_a_failed_write_leaves_nothing_behind(tmp_path, monkeypatch):
    from quantization import packed_io
    entries, arrays, _ = _entries()
    path = str(tmp_path / "toy.rdopack")
    for broken, why in ((dict(arrays, extra=np.zeros(2, np.float32)), "arrays without a reference"),
                        ({k: v for k, v in arrays.items() if k != "a/bias"}, "names no array"),
                        (dict(arrays, **{"a/bias": np.zeros(3, np.float64)}), "has dtype <f8")):
        with pytest.raises(ValueError, match=f"write_packed: .*{why}"):
            packed_io.write_packed(path, entries, broken)
        assert os.listdir(tmp_path) == []

    def failing(src, dst):
        raise OSError("planted failure")
    monkeypatch.setattr(os, "replace", failing)
    with pytest.raises(OSError, match="planted failure"):
        packed_io.write_packed(path, entries, arrays)
    assert os.listdir(tmp_path) == []
    monkeypatch.undo()
    open(path, "wb").write(b"an older file")                                      # a good write replaces what was there
    packed_io.write_packed(path, entries, arrays)
    assert os.listdir(tmp_path) == ["toy.rdopack"] and packed_io.read_packed(path)[1]["b/delta"].shape == ()


# ----------------------------------------------------------------------------- save_packed / load_packed: refusals without a device
def _weighted(qnn):
    from quantization import QuantModule
    return [(n, m) for n, m in qnn.named_modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def test_save_packed_refuses_an_uninitialised_quantiser_before_anything_is_done(tmp_path, no_library):
    qnn = _toy("cheng")
    path = str(tmp_path / "toy.rdopack")
    mods = _weighted(qnn)
    assert len(mods) > 10 and not any(m.weight_quantizer.inited for _, m in mods)
    with pytest.raises(ValueError, match=f"save_packed: the weight quantiser of module '{re.escape(mods[0][0])}' is not initialised"):
        qnn.save_packed(path)
    for _, m in mods[:-1]:                                                        # all but the LAST one initialised, as if by a forward
        q = m.weight_quantizer
        q.delta, q.zero_point, q.inited = torch.ones(1), torch.zeros(1), True
    from quantization.packed import save_packed
    with pytest.raises(ValueError, match=f"save_packed: the weight quantiser of module '{re.escape(mods[-1][0])}' is not initialised"):
        save_packed(qnn, path)
    assert os.listdir(tmp_path) == []
    # every quantiser initialised: the first pack is the first device work, and on a CPU model it refuses; still nothing is written
    q = mods[-1][1].weight_quantizer
    q.delta, q.zero_point, q.inited = torch.ones(1), torch.zeros(1), True
    with pytest.raises(ValueError, match="weight_pack: .*no CPU path"):
        qnn.save_packed(path)
    assert os.listdir(tmp_path) == []


def test_load_packed_refuses_an_unreadable_file_before_the_model_is_looked_at(tmp_path, no_library):
    qnn = _toy("cheng")
    path = str(tmp_path / "toy.rdopack")
    with open(path, "wb") as f:
        f.write(b"RDOPACK0" + b"\0" * 64)
    with pytest.raises(ValueError, match="read_packed: .*wrong magic"):
        qnn.load_packed(path)
    # a readable file of another model: the differences are listed, the hand-made modules and the toy's own
    from quantization import packed_io
    entries, arrays, _ = _entries()
    packed_io.write_packed(path, entries, arrays)
    first = _weighted(qnn)[0][0]
    with pytest.raises(ValueError, match="load_packed: .*does not fit this model: module 'a' is in the file only; module 'b' is in the file "
                                         f"only; module '{re.escape(first)}' is in the model only"):
        qnn.load_packed(path)
    assert not any(m.weight_quantizer.inited for _, m in _weighted(qnn))
