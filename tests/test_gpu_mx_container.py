"""The packed MX container on the GPU: `ops.mx_pack_rows` / `ops.mx_unpack_dequant` (rdo_mx_pack_rows, rdo_mx_unpack_dequant of
csrc/mx_container.hip) against the numpy reference of tests/mx_container_reference.py and the product's own `mx_pack_codes` /
`mx_dequant`; `save_mx_packed` -> `load_mx_packed` on the toy Cheng2020 (every inner but one ragged) and on the model of
tests/test_mx_tconv_args.py (whole blocks: the file's arrays are the native operands), with formats mixed per unit and one unit left on
its integer grid, after learned rounding, and under MX activations; what save and load refuse on the device.

Every comparison is exact (integers, or the bits of fp32 values): no tolerance appears anywhere."""
import os

import numpy as np
import pytest
import torch

import mx_container_reference as F
import mx_reference as R
from test_gpu_bit_alloc import _same_bits

pytestmark = pytest.mark.gpu

GUARD = 64                                                   # bytes; a multiple of 4, the alignment packed and w need
SENTINEL = 0xA5


def _interior(nbytes, pad=0):
    """a slice of nbytes inside a larger uint8 tensor pre-filled with a sentinel, `pad` bytes off 4-byte alignment -> (whole, slice)"""
    whole = torch.full((nbytes + 2 * GUARD + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD + pad:GUARD + pad + nbytes]


def _guards_untouched(whole, nbytes, pad=0):
    return bool((whole[:GUARD + pad] == SENTINEL).all()) and bool((whole[GUARD + pad + nbytes:] == SENTINEL).all())


def _bits32(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("fmt", R.NAMES)
def test_pack_rows_and_unpack_dequant_against_the_reference(fmt):
    from hipops import ops
    b = R.element_bits(fmt)
    for k, (rows, inner) in enumerate(F.SHAPES):
        codes_np, scales_np = F.random_case(rows, inner, fmt, seed=1000 * b + k)
        codes, scales = torch.from_numpy(codes_np).cuda(), torch.from_numpy(scales_np).cuda()
        low = codes & ((1 << b) - 1)
        nbytes = rows * F.row_bytes(inner, fmt)
        # pack into an interior slice: the reference's bytes, every byte written, the guards untouched
        whole_p, out = _interior(nbytes)
        got = ops.mx_pack_rows(codes, fmt, out=out.view(rows, -1))
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and _guards_untouched(whole_p, nbytes), (rows, inner)
        want = F.pack_rows(codes_np, fmt)
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), (rows, inner)
        fresh = ops.mx_pack_rows(codes, fmt)
        assert torch.equal(fresh, got) and torch.equal(codes, torch.from_numpy(codes_np).cuda())       # the input was not written to
        if inner % 32 == 0:
            op = ops.mx_pack_codes(codes, scales, fmt)
            assert torch.equal(op.packed, got) and torch.equal(ops.mx_unpack_codes(op), low)
        # unpack + dequant from that slice into interior slices: w is mx_dequant of the low bits, NaN where the scale is 255
        w_ref = ops.mx_dequant(low, scales, inner, fmt)
        w_cpu, c_cpu = F.decode_rows(want, scales_np, inner, fmt)
        whole_w, w_out = _interior(4 * rows * inner)
        whole_c, c_out = _interior(rows * inner, pad=3)                               # (codes need no alignment)
        both = ops.mx_unpack_dequant(got, scales, inner, fmt, want=("w", "codes"), w_out=w_out.view(torch.float32).view(rows, inner),
                                     codes_out=c_out.view(rows, inner))
        torch.cuda.synchronize()
        assert _guards_untouched(whole_w, 4 * rows * inner) and _guards_untouched(whole_c, rows * inner, pad=3), (rows, inner)
        assert _guards_untouched(whole_p, nbytes) and torch.equal(got, fresh)        # the packed input was not written to
        assert list(both) == ["w", "codes"]
        assert torch.equal(both["codes"], low) and np.array_equal(c_cpu, low.cpu().numpy()), (rows, inner)
        assert torch.equal(_bits32(both["w"]), _bits32(w_ref)), (rows, inner)
        nan = torch.from_numpy(np.repeat(scales_np == 255, 32, axis=1)[:, :inner]).cuda()
        assert bool(nan.any()) and bool(torch.isnan(both["w"][nan]).all())
        # the CPU decode, off the NaN block and where the random scale leaves the value inside fp32 (a weight's scale always does:
        # E <= 127 - emax; beyond it `mx_dequant`'s bits, compared above, are whatever its pattern arithmetic gives)
        ok = ~nan.cpu().numpy() & np.isfinite(w_cpu)
        assert ok.sum() > ok.size // 2 or rows * inner == 1
        assert np.array_equal(both["w"].cpu().numpy().view(np.uint32)[ok], w_cpu.view(np.uint32)[ok])
        # w only, codes only and both give the same bits
        only_w = ops.mx_unpack_dequant(got, scales, inner, fmt)
        only_c = ops.mx_unpack_dequant(got, scales, inner, fmt, want=("codes",))
        assert list(only_w) == ["w"] and list(only_c) == ["codes"]
        assert torch.equal(_bits32(only_w["w"]), _bits32(both["w"])) and torch.equal(only_c["codes"], both["codes"])


def test_wrappers_refuse_on_the_device_what_they_refuse_on_the_host():
    from hipops import ops
    codes = torch.zeros(3, 75, dtype=torch.uint8, device="cuda")
    pk = ops.mx_pack_rows(codes, "mxfp6_e3m2")
    sc = torch.full((3, 3), 127, dtype=torch.uint8, device="cuda")
    assert pk.shape == (3, 72) and not bool(pk.any())
    assert not bool(ops.mx_unpack_dequant(pk, sc, 75, "mxfp6_e3m2")["w"].any())
    for fn, args, kw, what in [(ops.mx_pack_rows, (codes.float(), "mxfp4"), {}, "codes must be an uint8 tensor"),
                               (ops.mx_pack_rows, (codes, "mxfp4"), {"out": pk}, "out must be a contiguous uint8 \\[3, 48\\]"),
                               (ops.mx_unpack_dequant, (pk, sc, 75, "mxfp4"), {}, "a row of inner 75 in mxfp4 has 48 bytes"),
                               (ops.mx_unpack_dequant, (pk, sc.cpu(), 75, "mxfp6_e3m2"), {}, "scales must be a contiguous uint8 \\[3, 3\\] on cuda"),
                               (ops.mx_unpack_dequant, (pk, sc, 75, "mxfp6_e3m2"), {"codes_out": codes}, "codes_out is given but 'codes' is not wanted"),
                               (ops.mx_unpack_dequant, (pk, sc, 75, "mxfp6_e3m2"), {"w_out": torch.zeros(3, 74, device="cuda")}, "w_out must be a contiguous fp32 \\[3, 75\\]")]:
        with pytest.raises(ValueError, match=what):
            fn(*args, **kw)


# ----------------------------------------------------------------------------- the round trip
def _weighted(qnn):
    from quantization import QuantModule
    return [(n, m) for n, m in qnn.named_modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def _forward(qnn, x, state):
    qnn.set_quant_state(*state)
    with torch.no_grad():
        return qnn(x)


def _leaves(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, dict):
        return [t for k in out for t in _leaves(out[k])]
    return [t for o in out for t in _leaves(o)]


def _same_outputs(a, b):
    la, lb = _leaves(a), _leaves(b)
    return len(la) == len(lb) > 0 and all(_same_bits(s.contiguous(), t.contiguous()) for s, t in zip(la, lb))


def _scramble(qnn):
    """noise over every weight, full-precision copy and bias that a checkpoint covers"""
    g = torch.Generator(device="cuda").manual_seed(7)
    for _, m in _weighted(qnn):
        for t in (m.weight.data, m.org_weight, None if m.bias is None else m.bias.data, m.org_bias):
            if t is not None:
                t.copy_(torch.randn(t.shape, generator=g, device="cuda"))
        m.drop_weight_pack()


def _refs(node):
    if isinstance(node, dict):
        if "ref" in node:
            yield node
        else:
            for v in node.values():
                yield from _refs(v)
    elif isinstance(node, list):
        for v in node:
            yield from _refs(v)


def _check_round_trip(qnn, fresh, x, path, states=((True, False), (True, True))):
    """`qnn` with MX and integer units -> save_mx_packed(path) -> load_mx_packed into `fresh` (same architecture, its weights noise):
    every check of the round trip -> (info, header, MX modules the native paths serve)"""
    from quantization import BaseQuantBlock, mx, packed_io
    from quantization.packed_io import row_words
    from quantization.quantizer import UniformAffineQuantizer
    mods = _weighted(qnn)
    on_mx = [(n, m) for n, m in mods if mx.is_mx_any(m.weight_quantizer)]
    on_int = [(n, m) for n, m in mods if not mx.is_mx_any(m.weight_quantizer)]
    assert on_mx and on_int
    want = {}
    for state in states:
        want[state] = _forward(qnn, x, state)
        assert _same_outputs(want[state], _forward(qnn, x, state)), state           # the saved model is reproducible to the bit
    used = {n: m.weight_quantizer(m.weight).detach().contiguous() for n, m in mods}
    info = qnn.save_mx_packed(path)
    assert _same_outputs(want[states[-1]], _forward(qnn, x, states[-1]))            # saving changes nothing
    header, arrays = packed_io.read_packed(path)
    data = open(path, "rb").read()
    # the sizes obey their formulas
    assert header["container"] == "mx" and header["order"] == [n for n, _ in mods]
    assert [e["name"] for e in header["modules"]] == [n for n, _ in on_int] and [e["name"] for e in header["mx_modules"]] == [n for n, _ in on_mx]
    size_bits = sum(m.weight_quantizer.size_bits(m.weight) for _, m in on_mx) + sum(int(m.weight_quantizer.n_bits) * m.weight.numel() for _, m in on_int)
    geo = {n: (int(m.weight_quantizer._rows(m.weight).shape[0]), m.weight.numel() // int(m.weight_quantizer._rows(m.weight).shape[0]))
           for n, m in mods}
    packed_bytes = sum(geo[n][0] * (F.row_bytes(geo[n][1], m.weight_quantizer.fmt) + R.blocks(geo[n][1])) for n, m in on_mx) + \
        sum(4 * e["rows"] * row_words(e["inner"], e["n_bits"]) for e in header["modules"])
    assert sum(R.size_bits(*geo[n], m.weight_quantizer.fmt) for n, m in on_mx) == sum(m.weight_quantizer.size_bits(m.weight) for _, m in on_mx)
    assert info == dict(modules=len(mods), mx_modules=len(on_mx), weights=sum(m.weight.numel() for _, m in mods), size_bits=size_bits,
                        packed_bytes=packed_bytes, padding_bits=8 * packed_bytes - size_bits, file_bytes=len(data))
    assert info["file_bytes"] == os.path.getsize(path) and info["padding_bits"] >= 0
    assert {k: v for k, v in info.items() if k != "file_bytes"} == header["totals"]
    # no fp32 array of a weight's element count, and no run of a weight's bytes, in the file
    counts = {m.weight.numel() for _, m in mods}
    assert not [r["ref"] for r in _refs(header) if r["dtype"] == "<f4" and int(np.prod(r["shape"], dtype=np.int64)) in counts]
    for name, m in mods:
        if m.kind in ("conv", "tconv", "linear"):
            for t in (m.weight, m.org_weight, used[name]):
                raw = t.detach().cpu().contiguous().numpy().tobytes()
                assert len(raw) >= 32 and raw[:32] not in data, name
    # per MX module: the reference's bytes of the forwarded codes; for a module the native paths serve, the operand's own arrays
    native = 0
    for (name, m), e in zip(on_mx, header["mx_modules"]):
        q = m.weight_quantizer
        rows, inner = geo[name]
        assert (e["grid"], e["fmt"], e["kind"], e["shape"], e["tconv"], e["rows"], e["inner"]) == \
            ("mx", q.fmt, m.kind, list(m.weight.shape), bool(m.if_tconv), rows, inner), name
        assert e["trained"] == bool(m.trained) and e["disable_act_quant"] == bool(m.disable_act_quant)
        assert e["rounding"] == ("learned" if getattr(q, "alpha", None) is not None else "nearest")
        on = getattr(m, "mx_activations", None)
        assert e["mx_activations"] == (None if on is None else list(on))
        packed = arrays[e["packed"]["ref"]].view(np.uint8).reshape(rows, -1)
        scales = arrays[e["scales"]["ref"]].view(np.uint8)
        nb = R.blocks(inner)
        assert not scales[rows * nb:].any() and scales.size == -(-rows * nb // 4) * 4
        scales = scales[:rows * nb].reshape(rows, nb)
        w_file, c_file = F.decode_rows(packed, scales, inner, q.fmt)
        assert np.array_equal(F.pack_rows(c_file, q.fmt), packed), name             # zero padding in every short last block
        assert np.array_equal(w_file.view(np.uint32), q._rows(used[name]).cpu().numpy().view(np.uint32)), name
        if mx.native_kind(m)[0] is not None:
            op = {"linear": mx.native_operand, "conv": mx.native_conv_operand, "tconv": mx.native_tconv_operand}[m.kind](m)
            assert op.packed.cpu().numpy().tobytes() == packed.tobytes() and op.scales.cpu().numpy().tobytes() == scales.tobytes(), name
            native += 1
        assert (e["bias"] is None) == (m.bias is None)
    # load into a model of the same architecture whose weights are noise
    _scramble(fresh)
    old_q = {n: m.weight_quantizer for n, m in _weighted(fresh)}
    totals = fresh.load_mx_packed(path)
    assert totals == header["totals"]
    loaded = dict(fresh.named_modules())
    for name, m in mods:
        t, q = loaded[name], m.weight_quantizer
        if mx.is_mx_any(q):
            assert type(t.weight_quantizer) is mx.MXQuantizer and t.weight_quantizer.fmt == q.fmt and t.weight_quantizer.tconv == t.if_tconv
            assert t.int_weight_quantizer is old_q[name]
            assert getattr(t, "mx_activations", None) == getattr(m, "mx_activations", None)
        else:
            assert t.weight_quantizer is old_q[name] and type(t.weight_quantizer) is UniformAffineQuantizer and t.weight_quantizer.n_bits == q.n_bits
        assert t.trained == m.trained and t.disable_act_quant == m.disable_act_quant and t._pack_memo == {}, name
        for got in (t.weight.detach(), t.org_weight, t.weight_quantizer(t.weight).detach()):
            assert _same_bits(got.contiguous(), used[name]), name
        assert m.bias is None or (_same_bits(t.bias.detach(), m.bias.detach()) and _same_bits(t.org_bias, m.bias.detach())), name
    for name, b in qnn.named_modules():
        if isinstance(b, BaseQuantBlock):
            assert loaded[name].trained == b.trained, name
    for state in states:
        assert _same_outputs(want[state], _forward(fresh, x, state)), state
    return info, header, native


def _mixed_formats(qnn, keep_int):
    """the five formats over the units in turn, `keep_int` left on its integer grid"""
    names = [n for n in qnn.units() if n != keep_int]
    plan = {n: R.NAMES[k % 5] for k, n in enumerate(names)}
    qnn.set_weight_format(plan, rounding="nearest")
    return plan


@pytest.fixture(scope="module")
def cheng_saved(tmp_path_factory):
    """the toy Cheng2020, formats mixed per unit, 'g_a.6' on its integer grid, round to nearest, saved -> (model, images, path, info)"""
    from test_gpu_unit_report import _toy
    qnn, cali, _, _ = _toy()
    _mixed_formats(qnn, "g_a.6")
    path = str(tmp_path_factory.mktemp("mxpacked") / "cheng.rdomx")
    info = qnn.save_mx_packed(path)
    return qnn, cali, path, info


def test_round_trip_on_toy_cheng2020(cheng_saved, tmp_path):
    from test_gpu_unit_report import _toy
    qnn, cali, path, first_info = cheng_saved
    fresh, _, _, _ = _toy()
    again = str(tmp_path / "again.rdomx")
    info, header, native = _check_round_trip(qnn, fresh, cali[:2], again)
    assert info == first_info and open(again, "rb").read() == open(path, "rb").read()          # the same model gives the same file
    assert {e["fmt"] for e in header["mx_modules"]} == set(R.NAMES) and len(header["modules"]) == 1
    # every inner is ragged but one (the 1x1 conv 32 -> 26 of entropy_parameters, which the native path serves)
    whole = [e["name"] for e in header["mx_modules"] if e["inner"] % 32 == 0]
    assert whole == ["model.entropy_parameters.0"] and native == 1 and len(header["mx_modules"]) == 53
    assert {27, 72, 8, 3, 200} <= {e["inner"] for e in header["mx_modules"]}
    assert info["padding_bits"] > 0
    fp32 = sum(v.numel() * v.element_size() for v in qnn.model.state_dict().values())
    print({k: info[k] for k in ("modules", "mx_modules", "weights", "size_bits", "packed_bytes", "padding_bits", "file_bytes")},
          "fp32 state_dict bytes", fp32)
    assert info["file_bytes"] < fp32


def _small():
    """the model of tests/test_gpu_mx_forward.py on the GPU, its integer quantisers initialised by one forward"""
    from test_mx_tconv_args import forward_model
    qnn = forward_model().cuda()
    x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(37)).cuda()
    _forward(qnn, x, (True, False))
    return qnn, x


@pytest.mark.parametrize("act", [None, ("mxfp8_e4m3", "native")])
def test_round_trip_on_the_small_model_with_whole_blocks(act, tmp_path):
    qnn, x = _small()
    assert list(qnn.units()) == ["stem", "conv", "up", "head", "fc"]
    qnn.set_weight_format({"conv": "mxfp4", "up": "mxfp6_e3m2", "head": "mxfp8_e4m3", "fc": "mxfp6_e2m3"})      # the stem stays on 'int'
    if act is not None:
        rep = qnn.set_mx_activations(*act)
        assert sorted(rep["native"]) == ["conv", "fc", "head", "up"]
    fresh, _ = _small()
    info, header, native = _check_round_trip(qnn, fresh, x, str(tmp_path / "small.rdomx"), states=((True, False),))
    assert native == 4 and [e["kind"] for e in header["mx_modules"]] == ["conv", "tconv", "conv", "linear"]
    assert [e["mx_activations"] for e in header["mx_modules"]] == [None if act is None else list(act)] * 4
    # whole blocks have no padding: what there is belongs to the words of the integer stem (27 weights of 8 bits a row)
    assert all(e["inner"] % 32 == 0 for e in header["mx_modules"]) and [(e["name"], e["inner"], e["n_bits"]) for e in header["modules"]] == [("model.stem", 27, 8)]
    assert info["padding_bits"] == 32 * (32 * 7 - 27 * 8)
    if act is not None:                                                             # the MX activations took part in what was compared
        qnn.set_mx_activations(None)
        assert not _same_outputs(_forward(qnn, x, (True, False)), _forward(fresh, x, (True, False)))


def test_round_trip_after_learned_rounding(tmp_path):
    from quantization import BaseQuantBlock, block_reconstruction, layer_reconstruction
    from quantization.mx import MXAdaRoundQuantizer
    from test_gpu_unit_report import _toy
    qnn, cali, _, kwargs = _toy()
    units = qnn.units()
    block, layer = "g_a.1", "g_a.6"
    assert isinstance(units[block], BaseQuantBlock) and not isinstance(units[layer], BaseQuantBlock)
    qnn.set_weight_format({block: "mxfp4", layer: "mxfp6_e2m3", "g_a.2": "mxfp8_e5m2"}, rounding="learned")
    kw = dict(kwargs, iters=8, act_quant=False)
    torch.manual_seed(1005)
    qnn.set_quant_state(True, False)
    block_reconstruction(qnn, units[block], block.split(".")[-1], **kw)
    layer_reconstruction(qnn, units[layer], layer.split(".")[-1], **kw)
    qnn.eval()
    learned = [m for _, m in _weighted(qnn) if isinstance(m.weight_quantizer, MXAdaRoundQuantizer) and m.weight_quantizer.alpha is not None]
    assert len(learned) >= 3 and all(m.trained for m in learned) and units[block].trained
    moved = sum(int((m.weight_quantizer(m.weight) != m.weight_quantizer._nearest(m.weight)).sum()) for m in learned)
    print(f"\n[mx-container] {moved} weights left round to nearest before the save")
    fresh, _, _, _ = _toy()
    info, header, _ = _check_round_trip(qnn, fresh, cali[:2], str(tmp_path / "learned.rdomx"))
    by = {e["name"]: e for e in header["mx_modules"]}
    assert sorted({e["rounding"] for e in by.values()}) == ["learned", "nearest"]   # 'g_a.2' was not calibrated: its alpha is None
    assert sum(e["trained"] for e in by.values()) == len(learned) and sum(header["blocks"].values()) == 1
    assert info["mx_modules"] == len(by) > len(learned)


# ----------------------------------------------------------------------------- refusals
def _state(qnn):
    tensors = [(k, v.clone()) for k, v in qnn.state_dict().items()]
    objects = [(n, id(m.weight_quantizer), "int_weight_quantizer" in m._modules, m.trained, getattr(m, "mx_activations", None)) for n, m in _weighted(qnn)]
    acts = [(n, q.act_mode, q.act_phase, q.dynamic_bits, sorted(q.act_range)) for n, q in qnn.act_quantizers()]
    return tensors, objects, acts


def _same_state(a, b):
    assert a[1] == b[1] and a[2] == b[2] and [k for k, _ in a[0]] == [k for k, _ in b[0]]
    for (k, s), (_, t) in zip(a[0], b[0]):
        assert s.dtype == t.dtype and s.shape == t.shape and torch.equal(s.reshape(-1).view(torch.uint8), t.reshape(-1).view(torch.uint8)), k


def test_save_refuses_a_weight_that_is_not_finite(tmp_path):
    qnn, x = _small()
    qnn.set_weight_format({"conv": "mxfp4", "head": "mxfp8_e4m3"})
    qnn.model.head.weight.data[3, 5, 0, 0] = float("inf")
    with pytest.raises(ValueError, match="save_mx_packed: module 'model.head' \\(mxfp8_e4m3\\) holds a block that is not finite.*nothing was written"):
        qnn.save_mx_packed(str(tmp_path / "inf.rdomx"))
    assert os.listdir(tmp_path) == []


def test_load_refuses_and_leaves_the_target_as_it_was(cheng_saved, tmp_path):
    from test_gpu_unit_report import _toy
    _, cali, path, _ = cheng_saved
    target, _, _, _ = _toy()
    before = _state(target)
    # a file for another architecture
    small, _ = _small()
    small.set_weight_format({"conv": "mxfp4"})
    other = str(tmp_path / "small.rdomx")
    small.save_mx_packed(other)
    with pytest.raises(ValueError, match="load_mx_packed: .* does not fit this model: ") as err:
        target.load_mx_packed(other)
    text = str(err.value)
    assert "module 'model.conv' is in the file only" in text and "module 'model.stem' is in the file only" in text
    assert text.count("is in the model only") == len(_weighted(target)) and "activation quantisers" in text
    _same_state(before, _state(target))
    # a file truncated by one byte
    cut = str(tmp_path / "cut.rdomx")
    with open(cut, "wb") as f:
        f.write(open(path, "rb").read()[:-1])
    with pytest.raises(ValueError, match="read_packed: .*truncated payload"):
        target.load_mx_packed(cut)
    _same_state(before, _state(target))
    # a `save_packed` file
    plain = str(tmp_path / "plain.rdopack")
    target.save_packed(plain)
    with pytest.raises(ValueError, match="load_mx_packed: .*without \"container\": \"mx\": `load_packed` takes what `save_packed` wrote"):
        target.load_mx_packed(plain)
    _same_state(before, _state(target))
    # the same names, other shapes: all listed
    from test_gpu_packed import _cheng_of
    wide = _cheng_of(16)
    _forward(wide, cali[:2], (True, False))
    snap = _state(wide)
    with pytest.raises(ValueError, match="load_mx_packed: .* does not fit this model: ") as err:
        wide.load_mx_packed(path)
    assert str(err.value).count(": shape [") > 10 and "in the file only" not in str(err.value)
    _same_state(snap, _state(wide))
    # and the untouched target still takes both files
    target.load_mx_packed(path)
    assert _same_outputs(_forward(target, cali[:2], (True, False)), _forward(cheng_saved[0], cali[:2], (True, False)))
