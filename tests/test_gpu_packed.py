"""The packed checkpoint on the GPU: `ops.weight_pack` / `ops.weight_unpack` (rdo_weight_pack, rdo_weight_unpack of csrc/weight_pack.hip)
against the product's own fake-quantisation kernels and the bit-string reference of tests/packed_reference.py; `save_packed` ->
`load_packed` on the toy Cheng2020 and one unit of the toy Lu2022; what `load_packed` refuses on the device.

Every comparison is exact (integers, or the bits of fp32 values): no tolerance appears anywhere."""
import functools
import json
import struct
import types

import numpy as np
import pytest
import torch

from packed_reference import pack_rows, row_words, unpack_rows
from test_gpu_bit_alloc import _same_bits, _same_snapshot, _snapshot

pytestmark = pytest.mark.gpu

WIDTHS = [2, 3, 5, 7, 8, 11, 16]
# a single code | a partial single word | an exact word (at 2 bits) | straddling codes | a ragged last word | many workgroups
SHAPES = [(1, 1), (3, 5), (1, 16), (2, 13), (4, 257), (192, 1728), (1, 40001)]
SENTINEL, GUARD = 0x5a5a5a5a, 67                             # (an odd guard: the slices are 4-byte, not 8-byte aligned)


@functools.lru_cache(maxsize=None)
def _case(rows, inner, bits):
    """seeded weights, grids and rounding logits -> (w, delta, zp, alpha) on the GPU, left unchanged by every test.  Even rows have a
    power-of-two delta (so that (k + 0.5) * delta and k * delta are exact and w / delta is exactly k + 0.5 | k), odd rows and the one
    long row a random one.  Of the weights a share is heavy-tailed (Cauchy) so that both clamps engage, a share exact ties, a share
    exact grid points; alpha holds exact zeros of both signs."""
    g = torch.Generator().manual_seed(100000 * bits + 1000 * rows + inner % 997)
    L = 2 ** bits
    delta = torch.pow(10.0, -3.0 * torch.rand(rows, generator=g))
    if inner < 40001:
        delta[::2] = 2.0 ** -5
    zp = torch.randint(0, L, (rows,), generator=g).float()
    zp[0] = float(L // 2)
    u = torch.rand(rows, inner, generator=g)
    heavy = torch.tan(3.14159 * (u - 0.5)) * (L / 6.0)                              # Cauchy, in units of delta
    k = torch.randint(-L, L, (rows, inner), generator=g).float()
    kind = torch.randint(0, 4, (rows, inner), generator=g)
    steps = torch.where(kind == 0, k + 0.5, torch.where(kind == 1, k, heavy))       # ties | grid points | heavy-tailed (half)
    w = (steps * delta[:, None]).contiguous()
    alpha = torch.randn(rows, inner, generator=g)
    alpha[kind == 1] = 0.0
    alpha.view(-1)[::7] = -0.0
    return tuple(t.cuda().contiguous() for t in (w, delta, zp, alpha))


def _interior(n, dtype):
    """a contiguous slice of n elements inside a larger tensor pre-filled with a sentinel -> (the whole tensor, the slice)"""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(dtype)


def _guards_untouched(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("rows,inner", SHAPES)
def test_pack_and_unpack_against_the_fake_quantisation_kernels(rows, inner, bits):
    from hipops import ops
    w, delta, zp, alpha = _case(rows, inner, bits)
    W = row_words(inner, bits)
    assert W == ops.pack_row_words(inner, bits)
    desc = ops.ada_desc(w, 2 ** bits, conv_layout=False)
    refs = {"nearest": (None, ops.uaq_fakequant(desc, w, delta, zp)),
            "adaround": (alpha, ops.adaround_fwd(desc, w, alpha, delta, zp, False))}
    seen = []
    for mode, (a, wq_ref) in refs.items():
        lv_ref = (torch.round(wq_ref / delta[:, None]) + zp[:, None]).to(torch.int64)
        assert 0 <= int(lv_ref.min()) and int(lv_ref.max()) <= 2 ** bits - 1
        if rows * inner >= 1000:                                                    # both clamps engage
            assert int(lv_ref.min()) == 0 and int(lv_ref.max()) == 2 ** bits - 1
        seen.append(lv_ref)
        # pack into an interior slice
        whole_p, out = _interior(rows * W, torch.int32)
        got = ops.weight_pack(w, delta, zp, bits, alpha_rows=a, out=out.view(rows, W))
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and _guards_untouched(whole_p, rows * W)
        words = got.cpu().numpy().view(np.uint32)
        want = pack_rows(lv_ref.cpu().numpy(), bits)
        assert words.shape == want.shape == (rows, W) and np.array_equal(words, want), (mode, "words")
        pad = 32 * W - inner * bits
        assert 0 <= pad < 32 and (pad == 0 or not np.any(words[:, -1] >> np.uint32(32 - pad))), (mode, "padding")
        fresh = ops.weight_pack(w, delta, zp, bits, alpha_rows=a)                   # an allocated output holds the same words
        assert torch.equal(fresh, got)
        # unpack from that slice into interior slices
        whole_l, lv_out = _interior(rows * inner, torch.int32)
        whole_q, wq_out = _interior(rows * inner, torch.float32)
        lv, wq = ops.weight_unpack(got, delta, zp, inner, bits, levels_out=lv_out.view(rows, inner), wq_out=wq_out.view(rows, inner))
        torch.cuda.synchronize()
        assert _guards_untouched(whole_l, rows * inner) and _guards_untouched(whole_q, rows * inner) and _guards_untouched(whole_p, rows * W)
        assert lv.dtype == torch.int32 and torch.equal(lv.to(torch.int64), lv_ref), (mode, "levels")
        assert _same_bits(wq, wq_ref), (mode, "wq")
        assert torch.equal(got, fresh)                                              # the input was not written to
        only_l, none_q = ops.weight_unpack(got, None, None, inner, bits, dequant=False)
        none_l, only_q = ops.weight_unpack(got, delta, zp, inner, bits, levels=False)
        assert none_q is None and none_l is None and torch.equal(only_l, lv) and _same_bits(only_q, wq_ref)
    if rows * inner >= 1000:                                                        # the two roundings differ, so both paths were seen
        assert not torch.equal(seen[0], seen[1])


def test_wrappers_refuse_on_the_device_what_they_refuse_on_the_host():
    from hipops import ops
    w, d, z = torch.zeros(3, 40, device="cuda"), torch.ones(3, device="cuda"), torch.zeros(3, device="cuda")
    pk = ops.weight_pack(w, d, z, 5)
    assert pk.shape == (3, 7) and not bool(pk.any())
    for fn, args, kw, what in [(ops.weight_pack, (w, d, z, 17), {}, "whole number in 2 .. 16"),
                               (ops.weight_pack, (w, d.cpu(), z, 5), {}, "delta must be a contiguous fp32"),
                               (ops.weight_pack, (w[:, ::2], d, z, 5), {}, "contiguous"),
                               (ops.weight_pack, (w, d, z, 5), {"alpha_rows": w[:2]}, "alpha_rows must be a contiguous fp32"),
                               (ops.weight_unpack, (pk, d, z, 45, 5), {}, "W = 8 words a row"),
                               (ops.weight_unpack, (pk, d, None, 40, 5), {}, "zp must be a contiguous fp32"),
                               (ops.weight_unpack, (pk, d, z, 40, 5), {"levels": False, "dequant": False}, "one of them True")]:
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


def _same_outputs(a, b):
    return _same_bits(a["x_hat"], b["x_hat"]) and list(a["likelihoods"]) == list(b["likelihoods"]) and \
        all(_same_bits(a["likelihoods"][k], b["likelihoods"][k]) for k in a["likelihoods"])


def _spread_widths(qnn, x):
    """widths 3, 5, 8 over the units in turn, the scales initialised at them by one forward"""
    names = list(qnn.units())
    qnn.set_weight_bits({n: (3, 5, 8)[k % 3] for k, n in enumerate(names)})
    _forward(qnn, x, (True, False))
    assert {row["size_bits"] // row["weights"] for n, row in qnn.weight_bits().items() if n != "total"} == {3, 5, 8}


def _calibrate(qnn, name, kwargs):
    from quantization import BaseQuantBlock, block_reconstruction, layer_reconstruction
    u = qnn.units()[name]
    torch.manual_seed(1005)
    qnn.set_quant_state(True, True)
    (block_reconstruction if isinstance(u, BaseQuantBlock) else layer_reconstruction)(qnn, u, name.split(".")[-1], **kwargs)
    assert u.trained
    qnn.eval()                                                                      # (the reconstruction leaves the model in train mode)
    return u


def _scramble(qnn):
    """noise over every weight, full-precision copy and bias that a checkpoint covers"""
    g = torch.Generator(device="cuda").manual_seed(7)
    for _, m in _weighted(qnn):
        for t in (m.weight.data, m.org_weight, None if m.bias is None else m.bias.data, m.org_bias):
            if t is not None:
                t.copy_(torch.randn(t.shape, generator=g, device="cuda"))
        m.drop_weight_pack()


def _check_round_trip(qnn, fresh, x, path):
    """`qnn` calibrated in part -> save_packed(path) -> load_packed into `fresh` (same architecture, its weights noise): every check of
    the round trip"""
    from quantization import BaseQuantBlock, packed_io
    from quantization.export import activation_state, integer_state
    from quantization.quantizer import AdaRoundQuantizer, UniformAffineQuantizer
    mods = _weighted(qnn)
    assert any(isinstance(m.weight_quantizer, AdaRoundQuantizer) for _, m in mods)
    assert any(not isinstance(m.weight_quantizer, AdaRoundQuantizer) for _, m in mods)
    # the original's forward is reproducible to the bit; these are what the loaded model has to compute
    want = {}
    for state in ((True, False), (True, True)):
        want[state] = _forward(qnn, x, state)
        assert _same_outputs(want[state], _forward(qnn, x, state)), state
    before = integer_state(qnn)
    assert list(before) == [n for n, _ in mods]
    info = qnn.save_packed(path)
    assert _same_outputs(want[(True, True)], _forward(qnn, x, (True, True)))       # saving changes nothing
    # the sizes
    bits = qnn.weight_bits()
    header, arrays = packed_io.read_packed(path)
    assert info["size_bits"] == bits["total"]["size_bits"] == header["totals"]["size_bits"] and info["weights"] == bits["total"]["weights"]
    assert info["modules"] == len(mods) == len(header["modules"])
    pads = [e["rows"] * (32 * row_words(e["inner"], e["n_bits"]) - e["inner"] * e["n_bits"]) for e in header["modules"]]
    assert all(0 <= 32 * row_words(e["inner"], e["n_bits"]) - e["inner"] * e["n_bits"] < 32 for e in header["modules"])
    assert info["padding_bits"] == sum(pads) and info["packed_bytes"] * 8 == info["size_bits"] + info["padding_bits"]
    assert info["packed_bytes"] == 4 * sum(e["rows"] * row_words(e["inner"], e["n_bits"]) for e in header["modules"])
    data = open(path, "rb").read()
    hlen, = struct.unpack("<Q", data[8:16])
    assert info["file_bytes"] == len(data) == 16 + hlen + (-hlen) % 8 + header["payload_bytes"]
    assert json.loads(data[16:16 + hlen].decode("utf-8")) == header
    # no fp32 weight in the file; the words unpack (bit strings) to integer_state's levels in to_rows order
    for (name, m), e in zip(mods, header["modules"]):
        q = m.weight_quantizer
        assert e["name"] == name and e["rounding"] == ("adaround" if isinstance(q, AdaRoundQuantizer) else "nearest")
        assert e["n_bits"] == q.n_bits == before[name]["n_bits"] and e["trained"] == bool(m.trained)
        if m.kind in ("conv", "tconv", "linear"):                                   # (seeded random weights: 8 of them in a row are a signature)
            raw = m.org_weight.detach().cpu().contiguous().numpy().tobytes()
            assert len(raw) >= 32 and raw[:32] not in data, name
        lv_rows = q._rows(before[name]["levels"]).reshape(e["rows"], e["inner"]).numpy().astype(np.int64)
        got, padding = unpack_rows(arrays[e["packed"]["ref"]], e["inner"], e["n_bits"])
        assert np.array_equal(got, lv_rows) and all(set(p) <= {"0"} for p in padding), name
        assert arrays[e["delta"]["ref"]].shape == tuple(q.delta.shape) and arrays[e["zero_point"]["ref"]].shape == tuple(q.zero_point.shape)
    # load into a model of the same architecture whose weights are noise
    _scramble(fresh)
    totals = fresh.load_packed(path)
    assert totals == header["totals"]
    after = integer_state(fresh)
    assert list(after) == list(before)
    for name in before:
        a, b = before[name], after[name]
        assert a["levels"].dtype == b["levels"].dtype and torch.equal(a["levels"], b["levels"]), name
        assert _same_bits(a["delta"], b["delta"]) and _same_bits(a["zero_point"], b["zero_point"]), name
        assert (a["n_bits"], a["kind"]) == (b["n_bits"], b["kind"]) and (a["bias"] is None) == (b["bias"] is None), name
        assert a["bias"] is None or _same_bits(a["bias"], b["bias"]), name
    sa, sb = activation_state(qnn), activation_state(fresh)
    assert list(sa) == list(sb)
    for k in sa:
        assert _same_bits(sa[k]["lo"], sb[k]["lo"]) and _same_bits(sa[k]["hi"], sb[k]["hi"]) and sa[k]["n_bits"] == sb[k]["n_bits"]
        assert sa[k]["channels"] == sb[k]["channels"]
    assert fresh.weight_bits() == bits
    loaded = dict(fresh.named_modules())
    for name, m in mods:
        t = loaded[name]
        assert type(t.weight_quantizer) is UniformAffineQuantizer and t.weight_quantizer.inited and t.trained == m.trained
        assert t.disable_act_quant == m.disable_act_quant and t.weight_quantizer.delta.device == t.weight.device
        used = m.weight_quantizer(m.weight).detach()
        assert _same_bits(t.weight_quantizer(t.weight).detach().contiguous(), used.contiguous()), name
        assert _same_bits(t.weight.detach().contiguous(), used.contiguous()) and _same_bits(t.org_weight.contiguous(), used.contiguous()), name
        assert m.bias is None or (_same_bits(t.bias.detach(), m.bias.detach()) and _same_bits(t.org_bias, m.bias.detach())), name
    for name, b in qnn.named_modules():
        if isinstance(b, BaseQuantBlock):
            assert loaded[name].trained == b.trained
    # the loaded model computes what the calibrated one computes, with its own weight quantisation on and off
    for state in ((True, False), (True, True)):
        assert _same_outputs(want[state], _forward(fresh, x, state)), state
        assert _same_outputs(want[state], _forward(fresh, x, (False, state[1]))), ("weight quantisation off", state)
    return info, header


def _cheng_of(N):
    """`_toy()` of test_gpu_unit_report.py at another width N (same seeds, same set-up; N = 8 there)"""
    import lic
    from quantization import QuantModel
    torch.manual_seed(1005)
    model = lic.Cheng2020Anchor(N=N).cuda().eval()
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq, is_cheng=True).cuda().eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    return qnn


@pytest.fixture(scope="module")
def cheng_saved(tmp_path_factory):
    """the toy Cheng2020 at widths 3 | 5 | 8, one block unit and one layer unit calibrated (20 iterations), the layer's activation
    quantiser frozen to hand-made static ranges, saved -> (model, images, path, info)"""
    from test_gpu_unit_report import _toy
    from quantization import BaseQuantBlock
    qnn, cali, _, kwargs = _toy()
    x = cali[:2]
    _spread_widths(qnn, x)
    units = qnn.units()
    block = next(n for n, u in units.items() if isinstance(u, BaseQuantBlock))
    layer = next(n for n, u in units.items() if not isinstance(u, BaseQuantBlock) and n.startswith("g_a"))
    assert (block, layer) == ("g_a.0", "g_a.6")
    assert kwargs["iters"] == 20
    for name in (block, layer):
        _calibrate(qnn, name, kwargs)
    # static ranges by hand, as tests/test_actquant_static_args.py makes them: the channel count from one observed forward, the values ours
    q = units[layer].act_quantizer
    q.set_act_mode("static")
    q.act_observe()
    _forward(qnn, x, (True, True))
    assert sorted(q.act_range) == [0]
    C = q.act_range[0].numel() // 2
    lo = -0.125 * torch.arange(1, C + 1, dtype=torch.float32, device="cuda")
    q.act_range = {0: torch.cat([lo, -lo * 2])}
    q.act_phase = "frozen"
    assert q.act_frozen() and len(qnn.act_ranges()) == 1
    path = str(tmp_path_factory.mktemp("packed") / "cheng.rdopack")
    info = qnn.save_packed(path)
    return qnn, cali, path, info


def test_round_trip_on_toy_cheng2020(cheng_saved, tmp_path):
    from test_gpu_unit_report import _toy
    qnn, cali, path, first_info = cheng_saved
    fresh, _, _, _ = _toy()
    again = str(tmp_path / "again.rdopack")
    info, header = _check_round_trip(qnn, fresh, cali[:2], again)
    assert info == first_info and open(again, "rb").read() == open(path, "rb").read()          # the same model gives the same file
    print({k: info[k] for k in ("modules", "weights", "size_bits", "packed_bytes", "padding_bits", "file_bytes")})
    assert {e["n_bits"] for e in header["modules"]} == {3, 5, 8}
    assert "conv" in {e["kind"] for e in header["modules"]}
    frozen = [r for r in header["act_quantizers"].values() if "sites" in r]
    assert len(frozen) == 1 and frozen[0]["act_mode"] == "static" and list(frozen[0]["sites"]) == ["0"]
    assert sum(header["blocks"].values()) == 1 and sum(e["trained"] for e in header["modules"]) >= 2


def test_round_trip_on_one_unit_of_toy_lu2022(tmp_path):
    from test_gpu_rd_report import _lu2022
    from quantization.quant_block import QuantRSTB
    qnn, cali = _lu2022()
    cali = torch.cat([cali, torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(12)).cuda()])
    _spread_widths(qnn, cali)
    name = "g_a1"
    assert isinstance(qnn.units()[name], QuantRSTB)
    args = types.SimpleNamespace(lmbda=0.0483, task_loss=2.0, arch="Lu2022")
    kwargs = dict(cali_data=cali, batch_size=2, iters=6, weight=0.01, input_prob=0.5, lr=4e-5, asym=True, b_range=(20, 2), warmup=0.2,
                  act_quant=True, opt_mode="mse", config=None, args=args)
    u = _calibrate(qnn, name, kwargs)
    kinds = {m.kind for _, m in _weighted(u)}
    assert {"linear", "layernorm"} <= kinds
    fresh, _ = _lu2022()
    info, header = _check_round_trip(qnn, fresh, cali, str(tmp_path / "lu2022.rdopack"))
    rows = {e["kind"]: e["rows"] for e in header["modules"]}
    assert rows["layernorm"] == 1 and rows["linear"] > 1                            # per-tensor rows and per-channel rows
    assert {e["n_bits"] for e in header["modules"]} == {3, 5, 8}


# ----------------------------------------------------------------------------- refusals
def _tensors(qnn):
    out = []
    for _, m in _weighted(qnn):
        out += [m.weight.detach().clone(), m.org_weight.clone()] + ([] if m.bias is None else [m.bias.detach().clone(), m.org_bias.clone()])
    for _, q in qnn.act_quantizers():
        out += [(q.act_mode, q.act_phase, q.dynamic_bits, sorted(q.act_range))]
    return out


def _same_tensors(a, b):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert _same_bits(s, t) if torch.is_tensor(s) else s == t


def test_load_packed_refuses_and_leaves_the_target_as_it_was(cheng_saved, tmp_path):
    from test_gpu_unit_report import _toy
    from quantization import packed_io
    _, cali, path, _ = cheng_saved
    # a target that holds a trained module
    target, _, _, _ = _toy()
    name, m = _weighted(target)[3]
    m.trained = True
    snap, tens = _snapshot(target), _tensors(target)
    with pytest.raises(ValueError, match=f"load_packed: the target holds trained module\\(s\\) \\['{name}'\\]"):
        target.load_packed(path)
    _same_snapshot(snap, _snapshot(target))
    _same_tensors(tens, _tensors(target))
    m.trained = False
    # a file truncated by one byte
    cut = str(tmp_path / "cut.rdopack")
    with open(cut, "wb") as f:
        f.write(open(path, "rb").read()[:-1])
    snap, tens = _snapshot(target), _tensors(target)
    with pytest.raises(ValueError, match="read_packed: .*truncated payload"):
        target.load_packed(cut)
    _same_snapshot(snap, _snapshot(target))
    _same_tensors(tens, _tensors(target))
    # a model of another width N: the same names, other shapes, all listed
    other = _cheng_of(16)
    _forward(other, cali[:2], (True, False))
    snap, tens = _snapshot(other), _tensors(other)
    (first, m0), e0 = _weighted(other)[0], packed_io.read_packed(path)[0]["modules"][0]
    with pytest.raises(ValueError, match="load_packed: .*does not fit this model: ") as err:
        other.load_packed(path)
    text = str(err.value)
    assert e0["name"] == first and e0["shape"][0] == 8 and m0.weight.shape[0] == 16
    assert f"module '{first}': shape {e0['shape']} in the file, {list(m0.weight.shape)} in the model" in text
    assert text.count(": shape [") > 10 and "in the file only" not in text
    _same_snapshot(snap, _snapshot(other))
    _same_tensors(tens, _tensors(other))
    # and the untouched target still takes the file
    target.load_packed(path)
    assert target.weight_bits() == cheng_saved[0].weight_bits()
