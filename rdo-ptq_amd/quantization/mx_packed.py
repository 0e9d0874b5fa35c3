"""Packed checkpoint of a QuantModel whose weights stand on MX block formats (`QuantModel.set_weight_format`), on integer grids, or on
both: `save_mx_packed` / `load_mx_packed`.  The container is `packed_io`'s, magic and version unchanged; the header carries
"container": "mx".  `save_packed` / `load_packed` keep serving models that are on integer grids throughout, and keep refusing MX modules.

File, as far as it differs from `packed_io`'s description:
  container       "mx"
  modules         the integer-grid modules in `named_modules` order: entry and arrays exactly what `save_packed` writes for them
                  (`packed.pack_int_module`; `packed_io.read_packed` checks their packed lengths)
  mx_modules      the MX modules in `named_modules` order; each entry: name, grid ("mx"), fmt, rounding ("nearest" | "learned"), kind,
                  shape (logical weight shape), tconv, rows, inner (of `to_rows(weight, tconv)`), trained, disable_act_quant,
                  mx_activations ([act_fmt, mode] or null), and the arrays
                    packed  "<u4" [rows, nb * b], nb = ceil(inner / 32): the bytes of `ops.mx_pack_rows` (include/rdo_ptq_mxfile.h; for
                            inner % 32 == 0 the packed operand the block-scaled matrix instruction reads)
                    scales  "<u4" [ceil(rows * nb / 4)]: the rows * nb E8M0 bytes of the blocks, row by row, zero-padded to whole words
                    bias    "<f4" or null: the bias the quantised forward uses
  order           every weighted module's name in `named_modules` order (the two lists interleave)
  totals          modules, mx_modules, weights, size_bits, packed_bytes, padding_bits
The codes and scales are those of the weight as its quantiser forwards it -- `ops.mx_fakequant` for an `MXQuantizer`,
`codes_and_scales(weight)` for an `MXAdaRoundQuantizer`, learned rounding included.  The file holds no fp32 weight.

Why a plain `MXQuantizer` suffices on the loading side.  The loaded weight is on the grid of its blocks: w = q * X with q a grid value
of the format and X = 2^E the stored scale.  Round-to-nearest of an on-grid block on its own grid gives the block back, so it is enough
that the scale byte is re-derived equal, E' = clamp(floor(log2(amax)) - emax, -127, .) = E.  The largest element of the block the
quantiser saw lay in [2^(emax + E), 2^(emax + E + 1)) (or E = -127 and it lay below 2^(emax - 127 + 1)).  Rounding to nearest maps
that binade, in units of X, into [2^emax, max] -- the grid holds 2^emax, and what would round above max saturates at max < 2^(emax +
1) -- and learned rounding takes the lower or the upper neighbour of the same interval, never a value below 2^emax (2^emax is itself a
grid value, so it is the lowest lower neighbour of the binade) and never one above max (a pinned element).  So the largest stored
magnitude is again in [2^(emax + E), 2^(emax + E + 1)) and E' = E; under E = -127 a block whose largest element lies below 2^(emax -
127) re-derives an exponent below -127 that the clamp puts back to -127.  An all-zero block has E = -127 on both sides.
tests/test_mx_container_args.py proves it on the CPU reference for every grid value of every format as the block maximum at several E,
-127 included; no counter-example exists, so the loaded module re-quantises and no stored-weight bypass is built."""
from collections import OrderedDict

import numpy as np
import torch

from hipops import _lib as L

from . import packed_io
from .mx import MX_ACT_MODES, MX_FORMATS, MXQuantizer, is_mx_any, is_mx_learned
from .packed import (_blocks, _weighted, check_int_module, install_blocks_and_acts, install_int_module, install_weight,
                     int_module_differences, module_differences, other_differences, pack_act_quantizers, pack_bias, pack_int_module,
                     stage_act_ranges, stage_int_module)
from .quantizer import UniformAffineQuantizer, from_rows

CONTAINER = "mx"
MX_BLOCK = L.MX_BLOCK


def mx_row_geometry(weight, tconv):
    """(rows, inner) of `to_rows(weight, tconv)` flattened to rank 2, without making it"""
    rows = 1 if weight.dim() == 1 else int(weight.shape[1] if (tconv and weight.dim() == 4) else weight.shape[0])
    return rows, int(weight.numel()) // rows


def _mx_codes(m):
    """(codes uint8 [rows, inner], scales uint8 [rows, nb]) of a module's weight as its MX quantiser forwards it"""
    from hipops import ops
    q = m.weight_quantizer
    if is_mx_learned(q):
        return q.codes_and_scales(m.weight)
    out = ops.mx_fakequant(q._rows(m.weight.detach()), q.fmt, want=("codes", "scales"))
    return out["codes"], out["scales"]


def save_mx_packed(qnn, path) -> dict:
    """Write the packed checkpoint of `qnn` to `path`: every QuantModule that holds a weight, whatever grid it stands on.  An
    integer-grid module is checked and packed as `save_packed` does it.  An MX module (`MXQuantizer` or `MXAdaRoundQuantizer`) stores
    the element codes of `m.weight` as its quantiser forwards them, packed at their own width along `to_rows` (`ops.mx_pack_rows`),
    the blocks' scale bytes, the bias the quantised forward uses (`m.bias`) and its `mx_activations`.  Blocks' `trained` and the
    activation quantisers go along as in `save_packed`.  Everything is checked before anything is written: a module whose weight
    quantiser is not initialised, a module off the GPU, and a module one of whose blocks is not finite (scale code 255) are refused by
    name (ValueError), and no file appears.
    -> {'modules' (all of them), 'mx_modules', 'weights', 'size_bits', 'packed_bytes', 'padding_bits', 'file_bytes'}.  size_bits: per
    integer-grid module n_bits x elements, per MX module `q.size_bits(weight)` = element bits x elements + 8 x blocks; packed_bytes:
    the packed elements and, for MX modules, the scale bytes; padding_bits = 8 packed_bytes - size_bits (the unused bits of a row's
    last word, or of its short last block)."""
    from hipops import ops
    what = "save_mx_packed"
    mods = _weighted(qnn)
    off_gpu = [n for n, m in mods if not m.weight.is_cuda]
    if off_gpu:
        raise ValueError(f"{what}: module(s) {off_gpu[:3]} are not on the GPU; there is no CPU path; nothing was written")
    coded = {}
    for name, m in mods:
        if not is_mx_any(m.weight_quantizer):
            check_int_module(what, name, m)
            continue
        codes, scales = _mx_codes(m)
        if bool((scales == 255).any()):
            raise ValueError(f"{what}: module {name!r} ({m.weight_quantizer.fmt}) holds a block that is not finite (a NaN or an infinity in "
                             "its weight): it has no codes to store; nothing was written")
        coded[name] = (codes, scales)
    entries, mx_entries, arrays = [], [], OrderedDict()
    weights = size_bits = nbytes = 0
    for name, m in mods:
        q = m.weight_quantizer
        if name not in coded:
            entry, n, sb, words = pack_int_module(name, m, arrays)
            entries.append(entry)
            weights, size_bits, nbytes = weights + n, size_bits + sb, nbytes + 4 * words
            continue
        codes, scales = coded[name]
        rows, inner = int(codes.shape[0]), int(codes.shape[1])
        assert (rows, inner) == mx_row_geometry(m.weight, q.tconv)
        packed = ops.mx_pack_rows(codes, q.fmt)
        on = getattr(m, "mx_activations", None)
        entry = OrderedDict(name=name, grid="mx", fmt=q.fmt, rounding="learned" if is_mx_learned(q) and q.alpha is not None else "nearest",
                            kind=m.kind, shape=[int(s) for s in m.weight.shape], tconv=bool(q.tconv), rows=rows, inner=inner,
                            trained=bool(m.trained), disable_act_quant=bool(m.disable_act_quant),
                            mx_activations=None if on is None else [on[0], on[1]])
        sc = scales.reshape(-1).cpu().numpy()
        arrays[f"{name}/packed"] = packed.cpu().numpy().view(np.uint32)
        arrays[f"{name}/scales"] = np.concatenate([sc, np.zeros(-sc.size % 4, np.uint8)]).view(np.uint32)
        entry["packed"], entry["scales"] = {"ref": f"{name}/packed"}, {"ref": f"{name}/scales"}
        pack_bias(name, m, entry, arrays)
        mx_entries.append(entry)
        weights, size_bits, nbytes = weights + rows * inner, size_bits + q.size_bits(m.weight), nbytes + packed.numel() + sc.size
    acts = pack_act_quantizers(qnn, arrays)
    totals = OrderedDict(modules=len(mods), mx_modules=len(mx_entries), weights=weights, size_bits=size_bits, packed_bytes=nbytes,
                         padding_bits=8 * nbytes - size_bits)
    header = OrderedDict(container=CONTAINER, modules=entries, mx_modules=mx_entries, order=[n for n, _ in mods],
                         blocks=OrderedDict((n, bool(b.trained)) for n, b in _blocks(qnn)), act_quantizers=acts, totals=totals)
    _, file_bytes = packed_io.write_packed(path, header, arrays)
    return dict(totals, file_bytes=file_bytes)


def _mx_differences(n, e, m):
    """what keeps a stored MX entry from fitting the module of its name: `module_differences` along `to_rows`, the format, the array
    sizes, the `mx_activations` pair"""
    rows, inner = mx_row_geometry(m.weight, m.if_tconv)
    diffs, same_shape = module_differences(n, e, m, geometry=(rows, inner, bool(m.if_tconv)))
    if not isinstance(e["fmt"], str) or e["fmt"] not in MX_FORMATS:
        return diffs + [f"module {n!r}: unknown MX format {e['fmt']!r}; the formats are {list(MX_FORMATS)}"]
    if not same_shape:
        return diffs
    nb, bits = -(-inner // MX_BLOCK), L.MX_FORMATS[e["fmt"]][1]
    if list(e["packed"]["shape"]) != [rows, nb * bits] or e["packed"]["dtype"] != "<u4":
        diffs.append(f"module {n!r}: packed of shape {e['packed']['shape']} is not the [{rows}, {nb * bits}] words of {e['fmt']} rows")
    if list(e["scales"]["shape"]) != [-(-rows * nb // 4)] or e["scales"]["dtype"] != "<u4":
        diffs.append(f"module {n!r}: scales of shape {e['scales']['shape']} are not the {rows * nb} scale bytes of its blocks")
    on = e["mx_activations"]
    if on is not None and not (isinstance(on, list) and len(on) == 2 and on[0] in MX_FORMATS and on[1] in MX_ACT_MODES):
        diffs.append(f"module {n!r}: mx_activations {on!r} is no pair of a format out of {list(MX_FORMATS)} and a mode out of {list(MX_ACT_MODES)}")
    return diffs


def _differences(header, mods, blocks, acts):
    diffs = []
    stored = OrderedDict((e["name"], ("int", e)) for e in header["modules"])
    stored.update((e["name"], ("mx", e)) for e in header["mx_modules"])
    mine = OrderedDict(mods)
    diffs += [f"module {n!r} is in the file only" for n in header["order"] if n not in mine]
    diffs += [f"module {n!r} is in the model only" for n in mine if n not in stored]
    if sorted(header["order"]) != sorted(stored) or len(stored) != len(header["modules"]) + len(header["mx_modules"]):
        diffs.append("the file's module lists do not agree with its order")
    for n, (grid, e) in stored.items():
        if n in mine:
            diffs += int_module_differences(n, e, mine[n]) if grid == "int" else _mx_differences(n, e, mine[n])
    return diffs + other_differences(header, blocks, acts), stored


def load_mx_packed(qnn, path) -> dict:
    """Install the checkpoint `path` that `save_mx_packed` wrote into `qnn`, a QuantModel of the same architecture, on the GPU, that has
    not been calibrated and whose weights are on their integer quantisers.  Every check runs, and every weight is decoded, before
    anything is written: a refusal (ValueError: an unreadable file, `packed_io.read_packed`; a file without "container": "mx" -- a
    `save_packed` file, which `load_packed` takes --; module names, kinds, shapes, rows, inner or tconv that differ, an unknown format,
    all listed; a target that holds a trained module or an MX quantiser; a target that is not on the GPU) leaves the model bit for bit
    as it was found.
    An integer-grid module is installed as `load_packed` installs it.  Per MX module the weight is decoded on the GPU in one launch
    (`ops.mx_unpack_dequant`), brought back from rows (`from_rows`) and copied into `weight` and `org_weight`, the bias into `bias` and
    `org_bias`; the weight quantiser becomes `MXQuantizer(fmt, tconv=m.if_tconv)` -- round to nearest gives an on-grid weight back
    bit for bit (the module docstring), so learned rounding needs no state on this side -- and the replaced quantiser is kept as
    `int_weight_quantizer`, as `set_weight_format` keeps it; `trained`, `disable_act_quant` and `mx_activations` are set as stored and
    the weight pack is dropped.  Blocks and activation quantisers as in `load_packed`.  -> the header's totals."""
    from hipops import ops
    from .widths import is_trained
    what = "load_mx_packed"
    header, arrays = packed_io.read_packed(path)
    if not isinstance(header, dict) or header.get("container") != CONTAINER:
        raise ValueError(f"{what}: {path} is a packed checkpoint without \"container\": \"{CONTAINER}\": `load_packed` takes what "
                         "`save_packed` wrote")
    try:
        mods, blocks, acts = _weighted(qnn), _blocks(qnn), qnn.act_quantizers()
        diffs, stored = _differences(header, mods, blocks, acts)
    except (KeyError, TypeError, IndexError, AttributeError) as e:
        raise ValueError(f"{what}: {path}: malformed header: {e!r}")
    if diffs:
        raise ValueError(f"{what}: {path} does not fit this model: " + "; ".join(diffs))
    on_mx = [n for n, m in mods if is_mx_any(m.weight_quantizer)]
    if on_mx:
        raise ValueError(f"{what}: the target holds MX quantiser(s) on module(s) {on_mx[:3]}: a checkpoint goes into a fresh model "
                         "(set_weight_format('int') puts the integer quantisers back)")
    trained = [n for n, m in mods if is_trained(m) or not isinstance(m.weight_quantizer, UniformAffineQuantizer)]
    trained += [n for n, b in blocks if b.trained]
    if trained:
        raise ValueError(f"{what}: the target holds trained module(s) {trained}: a checkpoint goes into a model that has not been calibrated")
    off_gpu = [n for n, m in mods if not m.weight.is_cuda]
    if off_gpu:
        raise ValueError(f"{what}: module(s) {off_gpu[:3]} are not on the GPU; there is no CPU path")
    staged = []
    for name, m in mods:
        grid, e = stored[name]
        if grid == "int":
            staged.append(("int", stage_int_module(m, e, arrays)))
            continue
        dev = m.weight.device
        rows, inner = int(e["rows"]), int(e["inner"])
        nb = -(-inner // MX_BLOCK)
        packed = torch.from_numpy(arrays[e["packed"]["ref"]].view(np.uint8).reshape(rows, -1)).to(dev).contiguous()
        scales = torch.from_numpy(arrays[e["scales"]["ref"]].view(np.uint8)[:rows * nb].reshape(rows, nb).copy()).to(dev)
        if bool((scales == 255).any()):
            raise ValueError(f"{what}: {path}: module {name!r} stores the scale code 255 (a block that is not finite)")
        wr = ops.mx_unpack_dequant(packed, scales, inner, e["fmt"])["w"]
        tconv = bool(m.if_tconv)
        like = m.weight
        shape = tuple(like.permute(1, 2, 3, 0).shape if tconv else like.permute(0, 2, 3, 1).shape) if like.dim() == 4 else (rows, inner)
        w = from_rows(wr.reshape(shape), like, tconv)
        bias = None if e["bias"] is None else torch.from_numpy(arrays[e["bias"]["ref"]]).to(dev)
        staged.append(("mx", (m, e, w, bias)))
    ranges = stage_act_ranges(what, path, header, arrays, acts, next(qnn.parameters()).device)
    # nothing was written so far
    with torch.no_grad():
        for grid, item in staged:
            if grid == "int":
                install_int_module(*item)
                continue
            m, e, w, bias = item
            install_weight(m, e, w, bias)
            m.int_weight_quantizer = m.weight_quantizer
            m.weight_quantizer = MXQuantizer(e["fmt"], tconv=m.if_tconv)
            on = e["mx_activations"]
            m.mx_activations = None if on is None else (on[0], on[1])
            m.drop_weight_pack()
    install_blocks_and_acts(header, blocks, acts, ranges)
    return dict(header["totals"])
