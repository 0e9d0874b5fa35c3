"""The container of a packed checkpoint (`packed.save_packed` / `packed.load_packed`): plain numpy and the standard library -- no torch
device, no library call.

File:  8-byte magic b"RDOPACK1" | uint64 little-endian header length | UTF-8 JSON header | zero padding to an 8-byte boundary | payload.
Every payload array is little-endian and starts at an 8-byte boundary of the payload; the gaps are zero.  The header names an array by
  {"ref": key, "at": [offset, length] (bytes, inside the payload), "shape": the logical shape, "dtype": "<f4" | "<u4" | "<i4"}
and holds
  version         1
  crc32           zlib.crc32 of the payload
  payload_bytes
  modules         a list in `named_modules` order; each entry: name, kind, shape (logical weight shape), tconv, rows, inner, n_bits,
                  rounding ("adaround" | "nearest"), trained, disable_act_quant, and the arrays packed ("<u4" [rows, W], W =
                  ceil(inner * n_bits / 32), the bit layout of include/rdo_ptq_pack.h), delta and zero_point ("<f4", the quantiser's own
                  shapes), bias ("<f4") or null
  blocks          name -> trained, for every quant block
  act_quantizers  name -> {act_mode, dynamic_bits, and for a frozen static quantiser sites: site -> {channels, range: "<f4" [2 channels]
                  = lo | hi}}
  totals          modules, weights, size_bits, packed_bytes, padding_bits"""
import json
import os
import struct
import tempfile
import zlib

import numpy as np

MAGIC = b"RDOPACK1"
VERSION = 1
DTYPES = ("<f4", "<u4", "<i4")


def row_words(inner, bits):
    """W = ceil(inner * bits / 32): the 32-bit words of one row (rdo_pack_row_words)"""
    return -(-int(inner) * int(bits) // 32)


def _refs(node):
    """every array reference (a dict with a 'ref' key) under `node`, in document order"""
    if isinstance(node, dict):
        if "ref" in node:
            yield node
        else:
            for v in node.values():
                yield from _refs(v)
    elif isinstance(node, (list, tuple)):
        for v in node:
            yield from _refs(v)


def write_packed(path, header_entries, arrays):
    """Write a checkpoint.  `header_entries`: the header without version, crc32 and payload_bytes, with {"ref": key} (a "dtype" may be given
    with it; otherwise the array's own) wherever an array of `arrays` (key -> numpy array of 4-byte items) belongs; every key must be
    referred to exactly once.  The arrays are laid out in the order of their references.  The file is written under a temporary name in
    the directory of `path` and renamed over it; a failure leaves neither behind.  -> (the header as written, file bytes)."""
    header = json.loads(json.dumps(header_entries))                    # a deep copy that is JSON by construction
    chunks, off, seen = [], 0, set()
    for ref in _refs(header):
        key = ref["ref"]
        if key not in arrays or key in seen:
            raise ValueError(f"write_packed: {path}: the reference {key!r} names no array, or is used twice")
        seen.add(key)
        dtype = ref.get("dtype") or np.asarray(arrays[key]).dtype.newbyteorder("<").str
        if dtype not in DTYPES:
            raise ValueError(f"write_packed: {path}: array {key!r} has dtype {dtype}; the container holds {DTYPES}")
        a = np.asarray(arrays[key]).astype(dtype, copy=False)          # (0-d arrays stay 0-d: a per-tensor delta has the shape [])
        raw = a.tobytes(order="C")
        ref["at"], ref["shape"], ref["dtype"] = [off, len(raw)], [int(s) for s in a.shape], dtype
        pad = -len(raw) % 8
        chunks.append(raw + b"\0" * pad)
        off += len(raw) + pad
    if seen != set(arrays):
        raise ValueError(f"write_packed: {path}: arrays without a reference: {sorted(set(arrays) - seen)}")
    payload = b"".join(chunks)
    header["version"], header["crc32"], header["payload_bytes"] = VERSION, zlib.crc32(payload) & 0xffffffff, len(payload)
    text = json.dumps(header).encode("utf-8")
    head = MAGIC + struct.pack("<Q", len(text)) + text + b"\0" * (-len(text) % 8)
    directory = os.path.dirname(os.path.abspath(path))
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=directory)
    try:
        with os.fdopen(fd, "wb") as f:
            f.write(head)
            f.write(payload)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return header, len(head) + len(payload)


def read_packed(path):
    """-> (header, arrays: key -> numpy array in its logical shape).  ValueError naming the file and the reason for: wrong magic, unknown
    version, header length beyond the file, truncated payload (or bytes behind it), CRC mismatch, an offset or length outside the payload
    (or not 8-byte aligned, or not the size of its shape), a packed length that is not 4 * rows * W."""
    def bad(why):
        return ValueError(f"read_packed: {path}: {why}")
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 16 or data[:8] != MAGIC:
        raise bad(f"wrong magic {data[:8]!r}: not a packed checkpoint")
    hlen, = struct.unpack("<Q", data[8:16])
    if 16 + hlen > len(data):
        raise bad(f"header length {hlen} is beyond the file ({len(data)} bytes)")
    try:
        header = json.loads(data[16:16 + hlen].decode("utf-8"))
        version = header["version"]
        crc, n = int(header["crc32"]), int(header["payload_bytes"])
    except (ValueError, KeyError, TypeError) as e:
        raise bad(f"the header is not a JSON object with version, crc32 and payload_bytes: {e!r}")
    if version != VERSION:
        raise bad(f"unknown version {version!r}; this reader knows {VERSION}")
    start = 16 + hlen + (-hlen % 8)
    if len(data) - start < n:
        raise bad(f"truncated payload: {max(len(data) - start, 0)} of {n} bytes")
    if len(data) - start > n:
        raise bad(f"{len(data) - start - n} bytes behind the payload")
    payload = data[start:]
    if zlib.crc32(payload) & 0xffffffff != crc:
        raise bad(f"CRC mismatch: the payload has {zlib.crc32(payload) & 0xffffffff:#010x}, the header {crc:#010x}")
    arrays = {}
    try:
        for ref in _refs(header):
            key, (off, length), shape, dtype = ref["ref"], ref["at"], [int(s) for s in ref["shape"]], ref["dtype"]
            if not (isinstance(off, int) and isinstance(length, int) and 0 <= off and 0 <= length and off + length <= n) or off % 8:
                raise bad(f"array {key!r} at offset {off}, length {length} lies outside the payload of {n} bytes (or is not 8-byte aligned)")
            if dtype not in DTYPES or any(s < 0 for s in shape) or 4 * int(np.prod(shape, dtype=np.int64)) != length:
                raise bad(f"array {key!r}: {length} bytes are not a {dtype} array of shape {shape}")
            if key in arrays:
                raise bad(f"array {key!r} is referred to twice")
            arrays[key] = np.frombuffer(payload, dtype=dtype, count=length // 4, offset=off).reshape(shape).astype(dtype[1:])
        for m in header.get("modules", []):
            W = row_words(m["inner"], m["n_bits"])
            length = m["packed"]["at"][1]
            if m["rows"] < 1 or m["inner"] < 1 or length != 4 * m["rows"] * W:
                raise bad(f"module {m['name']!r}: packed holds {length} bytes, not 4 * rows * W = 4 * {m['rows']} * {W}")
    except (KeyError, TypeError, IndexError) as e:
        raise bad(f"malformed header: {e!r}")
    except ValueError as e:
        if str(e).startswith("read_packed: "):
            raise
        raise bad(f"malformed header: {e!r}")
    return header, arrays
