"""Reference of the stored MX rows (include/rdo_ptq_mxfile.h), shared by tests/test_mx_container_args.py and
tests/test_gpu_mx_container.py: numpy on the CPU, building on tests/mx_reference.py.  A row of any length is ceil(inner / 32) blocks of
4 b bytes; element j of a block occupies bits [j b, (j + 1) b) of the block's little-endian bit string; the missing elements of a short
last block are zero codes.  Written on its own, not through tests/mx_gemm_reference.py, whose packing it is compared with.

Run as a script it writes the cases tools/mx_block_bits_check.cpp reads (the host program that runs the kernels' own bit-placement
functions): `python tests/mx_container_reference.py cases.bin`."""
import sys

import numpy as np

import mx_reference as R

NAMES = R.NAMES
BLOCK = R.BLOCK
SHAPES = ((1, 1), (3, 27), (5, 33), (2, 75), (4, 64), (7, 101), (16, 288))      # rows x inner of the kernel tests


def row_bytes(inner, fmt):
    return R.blocks(inner) * 4 * R.element_bits(fmt)


def pack_rows(codes, fmt):
    """codes uint8 [rows, inner] (upper bits ignored) -> uint8 numpy [rows, row_bytes]"""
    c = np.asarray(codes, dtype=np.uint8)
    b = R.element_bits(fmt)
    rows, inner = c.shape
    nb = R.blocks(inner)
    out = np.zeros((rows, nb * 4 * b), dtype=np.uint8)
    for r in range(rows):
        for kb in range(nb):
            word = 0                                                             # the block's bit string as one Python integer
            for j, code in enumerate(c[r, kb * BLOCK:(kb + 1) * BLOCK]):
                word |= (int(code) & ((1 << b) - 1)) << (j * b)
            out[r, kb * 4 * b:(kb + 1) * 4 * b] = np.frombuffer(word.to_bytes(4 * b, "little"), dtype=np.uint8)
    return out


def unpack_rows(packed, inner, fmt):
    """the inverse of `pack_rows` -> uint8 numpy [rows, inner]; the padding of a short last block is not looked at"""
    p = np.asarray(packed, dtype=np.uint8)
    b = R.element_bits(fmt)
    rows = p.shape[0]
    assert p.shape[1] == row_bytes(inner, fmt)
    out = np.zeros((rows, inner), dtype=np.uint8)
    for r in range(rows):
        for kb in range(R.blocks(inner)):
            word = int.from_bytes(p[r, kb * 4 * b:(kb + 1) * 4 * b].tobytes(), "little")
            for j in range(min(BLOCK, inner - kb * BLOCK)):
                out[r, kb * BLOCK + j] = (word >> (j * b)) & ((1 << b) - 1)
    return out


def decode_rows(packed, scales, inner, fmt):
    """packed uint8 [rows, row_bytes], scales uint8 [rows, blocks] -> (w float32 numpy [rows, inner], codes uint8 [rows, inner]): the
    decode is tests/mx_reference.py's (a scale code of 255 gives NaN)"""
    import torch
    codes = unpack_rows(packed, inner, fmt)
    w = R.dequantize(torch.from_numpy(codes), torch.from_numpy(np.ascontiguousarray(scales)), fmt)
    return w.numpy(), codes


def random_case(rows, inner, fmt, seed):
    """codes uint8 [rows, inner] with garbage in the upper bits, scales uint8 [rows, blocks] in 0 .. 254 with one 255"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (rows, inner)).astype(np.uint8)
    scales = rng.integers(0, 255, (rows, R.blocks(inner))).astype(np.uint8)
    scales[rng.integers(0, rows), rng.integers(0, scales.shape[1])] = 255
    return codes, scales


def write_cases(path):
    """every format x SHAPES (+ every n = 1 .. 32 as one row) as records: int32 bits, rows, inner, row_bytes | codes | packed"""
    with open(path, "wb") as f:
        for fi, fmt in enumerate(NAMES):
            for si, (rows, inner) in enumerate(SHAPES + tuple((1, n) for n in range(1, 33))):
                codes, _ = random_case(rows, inner, fmt, 100 * fi + si)
                packed = pack_rows(codes, fmt)
                f.write(np.array([R.element_bits(fmt), rows, inner, packed.shape[1]], dtype="<i4").tobytes())
                f.write(codes.tobytes())
                f.write(packed.tobytes())


if __name__ == "__main__":
    write_cases(sys.argv[1])
