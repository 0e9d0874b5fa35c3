"""Packed checkpoint of a calibrated QuantModel: the integer levels of every weight packed at their own width (`ops.weight_pack`), the
grids, the biases and the frozen activation ranges in one file (`packed_io`), and back into a fresh QuantModel of the same architecture
(`ops.weight_unpack`).  The file holds no fp32 weight; the loaded model computes bit for bit what the calibrated one computes.

Why a plain quantiser suffices on the loading side: with w_q = (l - z) * d the stored weight of a level l on the grid (d, z),
round-to-nearest of w_q on that grid gives l back and re-dequantises to the same bits, so a `UniformAffineQuantizer` holding (d, z)
reproduces the hard-rounded weights of an `AdaRoundQuantizer` with weight quantisation on, and `org_weight = w_q` does with it off."""
from collections import OrderedDict

import numpy as np
import torch

from . import packed_io
from .mx import refuse_mx
from .quant_block import BaseQuantBlock
from .quant_layer import QuantModule
from .quantizer import MAX_BITS, AdaRoundQuantizer, UniformAffineQuantizer, from_rows


def _weighted(qnn):
    return [(name, m) for name, m in qnn.named_modules() if isinstance(m, QuantModule) and m.org_weight is not None]


def _blocks(qnn):
    return [(name, m) for name, m in qnn.named_modules() if isinstance(m, BaseQuantBlock)]


def _row_shape(q, w):
    """the shape of `q._rows(w)` without making it"""
    if q.channel_wise and w.dim() != 1:
        if w.dim() == 4:
            return tuple(w.permute(1, 2, 3, 0).shape) if q.tconv else tuple(w.permute(0, 2, 3, 1).shape)
        return tuple(w.shape)
    return (1, w.numel())


def check_int_module(what, name, m):
    """ValueError naming a module whose integer-grid weight quantiser cannot be packed: not initialised, or at a width outside the grid"""
    q = m.weight_quantizer
    if not getattr(q, "inited", True) or q.delta is None or q.zero_point is None:
        raise ValueError(f"{what}: the weight quantiser of module {name!r} is not initialised: run a quantised forward (or calibrate) "
                         "first; nothing was written")
    if not 2 <= int(q.n_bits) <= MAX_BITS or q.n_levels != 2 ** int(q.n_bits):
        raise ValueError(f"{what}: module {name!r} stands at {q.n_bits} bits with {q.n_levels} levels")


def pack_int_module(name, m, arrays):
    """Pack one integer-grid module (`check_int_module` passed): its arrays go into `arrays` under '<name>/<field>' -> (the header entry,
    weight elements, n_bits x elements, 32-bit words).  What `save_packed` writes per module, shared with `mx_packed.save_mx_packed`."""
    from hipops import ops
    q = m.weight_quantizer
    w = m.org_weight.detach()
    wr = q._rows(w)
    wr = wr.reshape(wr.shape[0], -1)
    rows, inner, bits = int(wr.shape[0]), int(wr.shape[1]), int(q.n_bits)
    d = q.delta.detach().to(w.device, torch.float32)
    z = q.zero_point.detach().to(w.device, torch.float32)
    dr, zr = d.reshape(-1).expand(rows).contiguous(), z.reshape(-1).expand(rows).contiguous()
    ada = isinstance(q, AdaRoundQuantizer)
    ar = q._rows(q.alpha.detach()).reshape(rows, inner).contiguous() if ada else None
    packed = ops.weight_pack(wr, dr, zr, bits, alpha_rows=ar)
    entry = OrderedDict(name=name, kind=m.kind, shape=[int(s) for s in w.shape], tconv=bool(q.tconv), rows=rows, inner=inner,
                        n_bits=bits, rounding="adaround" if ada else "nearest", trained=bool(m.trained),
                        disable_act_quant=bool(m.disable_act_quant))
    for field, t in (("packed", packed.cpu().numpy().view(np.uint32)), ("delta", d.cpu().numpy()), ("zero_point", z.cpu().numpy())):
        arrays[f"{name}/{field}"] = t
        entry[field] = {"ref": f"{name}/{field}"}
    pack_bias(name, m, entry, arrays)
    return entry, rows * inner, bits * rows * inner, rows * packed.shape[1]


def pack_bias(name, m, entry, arrays):
    """the bias the quantised forward uses (`m.bias`, a bias correction included) as the entry's 'bias': an array reference or None"""
    if m.bias is None:
        entry["bias"] = None
    else:
        arrays[f"{name}/bias"] = m.bias.detach().to(torch.float32).cpu().numpy()
        entry["bias"] = {"ref": f"{name}/bias"}


def pack_act_quantizers(qnn, arrays):
    """name -> {act_mode, dynamic_bits, and the frozen ranges of a static quantiser} of every activation quantiser, the ranges in `arrays`"""
    acts = OrderedDict()
    for name, q in qnn.act_quantizers():
        row = OrderedDict(act_mode=getattr(q, "act_mode", "dynamic"), dynamic_bits=int(getattr(q, "dynamic_bits", 8)))
        if q.act_frozen():
            row["sites"] = OrderedDict()
            for site in sorted(q.act_range):
                r = q.act_range[site].detach().to(torch.float32).cpu().numpy()
                arrays[f"{name}/range/{site}"] = r
                row["sites"][str(site)] = {"channels": int(r.size // 2), "range": {"ref": f"{name}/range/{site}"}}
        acts[name] = row
    return acts


def save_packed(qnn, path) -> dict:
    """Write the packed checkpoint of `qnn` to `path`.  Covered is every QuantModule that holds a weight; one whose weight quantiser is
    not initialised is refused (ValueError naming it) before anything is packed or written -- `integer_state` skips such modules, a
    checkpoint must not.  A module with an `AdaRoundQuantizer` is packed with its rounding logits (down, plus one where alpha >= 0), any
    other to nearest; the levels are those of `m.org_weight`, as in `integer_state`; the bias is `m.bias`, the one the quantised forward
    uses (a bias correction included).  Frozen static activation ranges, `trained` and `disable_act_quant` go along.  The file is
    written under a temporary name in the same directory and renamed.
    -> {'modules', 'weights', 'size_bits' (sum of n_bits x elements: `weight_bits()['total']['size_bits']`), 'packed_bytes' (4 x sum of
    rows x W), 'padding_bits' (8 packed_bytes - size_bits), 'file_bytes'}."""
    what = "save_packed"
    mods = _weighted(qnn)
    refuse_mx(what, mods, ValueError, "a packed MX container is not built; nothing was written")
    for name, m in mods:
        check_int_module(what, name, m)
    entries, arrays = [], OrderedDict()
    weights = size_bits = words = 0
    for name, m in mods:
        entry, n, sb, nw = pack_int_module(name, m, arrays)
        entries.append(entry)
        weights, size_bits, words = weights + n, size_bits + sb, words + nw
    acts = pack_act_quantizers(qnn, arrays)
    totals = OrderedDict(modules=len(entries), weights=weights, size_bits=size_bits, packed_bytes=4 * words,
                         padding_bits=32 * words - size_bits)
    header = OrderedDict(modules=entries, blocks=OrderedDict((n, bool(b.trained)) for n, b in _blocks(qnn)), act_quantizers=acts,
                         totals=totals)
    _, file_bytes = packed_io.write_packed(path, header, arrays)
    return dict(totals, file_bytes=file_bytes)


def module_differences(n, e, m, geometry=None):
    """what keeps a stored entry `e` from fitting the module `m` of the same name `n`, whatever grid it is on: kind, shape, rows x inner,
    tconv, bias -> (sentences, whether the shapes agree).  `geometry`: the model's (rows, inner, tconv) where they are not those of the
    module's present weight quantiser (an MX entry lies along `to_rows` whatever `channel_wise` says)."""
    diffs = []
    if e["kind"] != m.kind:
        diffs.append(f"module {n!r}: kind {e['kind']!r} in the file, {m.kind!r} in the model")
    if list(e["shape"]) != [int(s) for s in m.weight.shape]:
        diffs.append(f"module {n!r}: shape {list(e['shape'])} in the file, {[int(s) for s in m.weight.shape]} in the model")
        return diffs, False
    if geometry is None:
        q = m.weight_quantizer
        rows = _row_shape(q, m.weight)[0]
        geometry = (rows, m.weight.numel() // rows, bool(q.tconv))
    rows, inner, tconv = geometry
    if (int(e["rows"]), int(e["inner"])) != (rows, inner) or bool(e["tconv"]) != tconv:
        diffs.append(f"module {n!r}: rows x inner {e['rows']} x {e['inner']} (tconv {e['tconv']}) in the file, "
                     f"{rows} x {inner} (tconv {tconv}) in the model")
    if (e["bias"] is None) != (m.bias is None) or (e["bias"] is not None and list(e["bias"]["shape"]) != [int(s) for s in m.bias.shape]):
        diffs.append(f"module {n!r}: the bias of the file does not fit the bias of the model")
    return diffs, True


def int_module_differences(n, e, m):
    """`module_differences` and what an integer-grid entry must hold besides: a width, a delta and a zero point that fit its rows"""
    diffs, same_shape = module_differences(n, e, m)
    if not same_shape:
        return diffs
    if isinstance(e["n_bits"], bool) or not isinstance(e["n_bits"], int) or not 2 <= e["n_bits"] <= MAX_BITS:
        diffs.append(f"module {n!r}: n_bits {e['n_bits']!r} is not a whole number in 2 .. {MAX_BITS}")
    for f in ("delta", "zero_point"):
        if int(np.prod(e[f]["shape"], dtype=np.int64)) not in (1, int(e["rows"])) or e[f]["dtype"] != "<f4":
            diffs.append(f"module {n!r}: {f} of shape {e[f]['shape']} does not fit {e['rows']} rows")
    return diffs


def other_differences(header, blocks, acts):
    """blocks and activation quantisers that are in the file or in the model only"""
    diffs = []
    if sorted(header["blocks"]) != sorted(n for n, _ in blocks):
        diffs.append(f"blocks {sorted(set(header['blocks']) ^ set(n for n, _ in blocks))} are on one side only")
    if sorted(header["act_quantizers"]) != sorted(n for n, _ in acts):
        diffs.append(f"activation quantisers {sorted(set(header['act_quantizers']) ^ set(n for n, _ in acts))} are on one side only")
    return diffs


def _differences(header, mods, blocks, acts):
    """what keeps the file from fitting the model, as a list of sentences (empty: it fits)"""
    diffs = []
    stored = OrderedDict((e["name"], e) for e in header["modules"])
    mine = OrderedDict(mods)
    diffs += [f"module {n!r} is in the file only" for n in stored if n not in mine]
    diffs += [f"module {n!r} is in the model only" for n in mine if n not in stored]
    for n, e in stored.items():
        if n in mine:
            diffs += int_module_differences(n, e, mine[n])
    return diffs + other_differences(header, blocks, acts)


def stage_int_module(m, e, arrays):
    """unpack one integer-grid entry on the GPU -> what `install_int_module` writes; nothing of the model is written here"""
    from hipops import ops
    dev = m.weight.device
    rows, inner, bits = int(e["rows"]), int(e["inner"]), int(e["n_bits"])
    d, z = torch.from_numpy(arrays[e["delta"]["ref"]]).to(dev), torch.from_numpy(arrays[e["zero_point"]["ref"]]).to(dev)
    packed = torch.from_numpy(arrays[e["packed"]["ref"]].view(np.int32).reshape(rows, -1)).to(dev).contiguous()
    _, wq = ops.weight_unpack(packed, d.reshape(-1).expand(rows).contiguous(), z.reshape(-1).expand(rows).contiguous(), inner, bits,
                              levels=False, dequant=True)
    q = m.weight_quantizer
    wr = wq.reshape(_row_shape(q, m.weight))
    w = from_rows(wr, m.weight, q.tconv) if (q.channel_wise and m.weight.dim() != 1) else wr.reshape(m.weight.shape)
    bias = None if e["bias"] is None else torch.from_numpy(arrays[e["bias"]["ref"]]).to(dev)
    return m, e, w, bias, d, z


def install_weight(m, e, w, bias):
    """the staged weight and bias into `weight` / `org_weight` and `bias` / `org_bias`, `trained` and `disable_act_quant` as stored"""
    m.weight.data.copy_(w)
    m.org_weight.copy_(w)
    if bias is not None:
        m.bias.data.copy_(bias)
        m.org_bias.copy_(bias)
    m.trained, m.disable_act_quant = bool(e["trained"]), bool(e["disable_act_quant"])


def install_int_module(m, e, w, bias, d, z):
    install_weight(m, e, w, bias)
    q = m.weight_quantizer
    q.bitwidth_refactor(int(e["n_bits"]))
    q.delta, q.zero_point, q.inited = d, z, True
    m.drop_weight_pack()


def stage_act_ranges(what, path, header, arrays, acts, device):
    """check the stored activation quantisers and put their frozen ranges on `device` -> name -> site -> range"""
    ranges = {}
    for name, q in acts:
        row = header["act_quantizers"][name]
        if row["act_mode"] not in ("dynamic", "static") or not 2 <= int(row["dynamic_bits"]) <= MAX_BITS:
            raise ValueError(f"{what}: {path}: activation quantiser {name!r} has act_mode {row['act_mode']!r}, dynamic_bits {row['dynamic_bits']!r}")
        ranges[name] = {int(s): torch.from_numpy(arrays[r["range"]["ref"]]).to(device) for s, r in row.get("sites", {}).items()}
    return ranges


def install_blocks_and_acts(header, blocks, acts, ranges):
    for name, b in blocks:
        b.trained = bool(header["blocks"][name])
    for name, q in acts:
        row = header["act_quantizers"][name]
        q.set_act_mode(row["act_mode"])
        q.dynamic_bits = int(row["dynamic_bits"])
        if "sites" in row:
            q.act_range, q.act_phase = ranges[name], "frozen"


def load_packed(qnn, path) -> dict:
    """Install the packed checkpoint `path` into `qnn`, a QuantModel of the same architecture that has not been calibrated.  Every check
    runs, and every weight is unpacked, before anything is written: a refusal (ValueError: an unreadable file, `packed_io.read_packed`;
    module names, kinds or shapes that differ, all listed; a target that holds a trained module; a target that is not on the GPU)
    leaves the model bit for bit as it was found.
    Per module the weight is unpacked on the GPU to w_q = (level - zero_point) * delta and copied into `weight` and `org_weight`, the
    bias into `bias` and `org_bias`; the weight quantiser stays a `UniformAffineQuantizer`, at the stored width, with the stored delta and
    zero point in their stored shapes on the weight's device and `inited = True`; `trained` and `disable_act_quant` are set as stored
    and the weight pack is dropped.  Blocks get their `trained`, activation quantisers their `act_mode` and `dynamic_bits`, and frozen
    static ones their ranges (phase "frozen").  -> the header's totals."""
    from .widths import is_trained
    what = "load_packed"
    try:
        header, arrays = packed_io.read_packed(path)
        mods, blocks, acts = _weighted(qnn), _blocks(qnn), qnn.act_quantizers()
        diffs = _differences(header, mods, blocks, acts)
    except (KeyError, TypeError, IndexError, AttributeError) as e:
        raise ValueError(f"{what}: {path}: malformed header: {e!r}")
    if diffs:
        raise ValueError(f"{what}: {path} does not fit this model: " + "; ".join(diffs))
    trained = [n for n, m in mods if is_trained(m) or not isinstance(m.weight_quantizer, UniformAffineQuantizer)]
    trained += [n for n, b in blocks if b.trained]
    if trained:
        raise ValueError(f"{what}: the target holds trained module(s) {trained}: a checkpoint goes into a model that has not been calibrated")
    off_gpu = [n for n, m in mods if not m.weight.is_cuda]
    if off_gpu:
        raise ValueError(f"{what}: module(s) {off_gpu[:3]} are not on the GPU; there is no CPU path")
    stored = {e["name"]: e for e in header["modules"]}
    staged = [stage_int_module(m, stored[name], arrays) for name, m in mods]
    ranges = stage_act_ranges(what, path, header, arrays, acts, next(qnn.parameters()).device)
    # nothing was written so far
    with torch.no_grad():
        for item in staged:
            install_int_module(*item)
    install_blocks_and_acts(header, blocks, acts, ranges)
    return dict(header["totals"])
