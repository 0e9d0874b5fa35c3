"""Reference packer and unpacker of the packed-checkpoint bit layout (include/rdo_ptq_pack.h), shared by tests/test_packed_args.py and
tests/test_gpu_packed.py: plain Python bit strings, no arithmetic on words.  string[j] is bit j of a row's bit string: code i occupies
string[i * b : (i + 1) * b] with its least significant bit first, word k is string[32 k : 32 k + 32] with ITS least significant bit
first, and the string is filled with zeros up to 32 W bits."""
import numpy as np


def row_words(inner, bits):
    return (inner * bits + 31) // 32


def pack_rows(levels, bits):
    """levels: integer array [rows, inner] with values in [0, 2^bits) -> uint32 [rows, W]"""
    levels = np.asarray(levels)
    rows, inner = levels.shape
    W = row_words(inner, bits)
    out = np.zeros((rows, W), dtype=np.uint32)
    for r in range(rows):
        codes = [int(v) for v in levels[r]]
        assert all(0 <= v < 2 ** bits for v in codes)
        string = "".join(format(v, f"0{bits}b")[::-1] for v in codes)
        string += "0" * (32 * W - len(string))
        for k in range(W):
            out[r, k] = int(string[32 * k:32 * k + 32][::-1], 2)
    return out


def unpack_rows(words, inner, bits):
    """uint32 [rows, W] -> (int64 levels [rows, inner], the padding bits of every row as a string)"""
    words = np.asarray(words)
    rows, W = words.shape
    assert W == row_words(inner, bits)
    levels = np.zeros((rows, inner), dtype=np.int64)
    padding = []
    for r in range(rows):
        string = "".join(format(int(v) & 0xffffffff, "032b")[::-1] for v in words[r])
        for i in range(inner):
            levels[r, i] = int(string[i * bits:(i + 1) * bits][::-1], 2)
        padding.append(string[inner * bits:])
    return levels, padding
