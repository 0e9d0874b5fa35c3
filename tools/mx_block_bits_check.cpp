// Host check of the bit placement of one MX block (rdo-ptq_amd/csrc/mx_block_bits.h: the functions the kernels of mx_container.hip call)
// against the numpy reference, under the host sanitizers.  A program of its own: nothing of it is loaded into Python or runs on a GPU.
//   python tests/mx_container_reference.py cases.bin
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mx_block_bits_check.cpp -o mx_block_bits_check
//   ./mx_block_bits_check cases.bin
// Each record: int32 bits, rows, inner, row_bytes | codes uint8 [rows][inner] | packed uint8 [rows][row_bytes].  The rows are walked as
// the kernels walk them; codes and packed live in heap buffers of their exact sizes, so a read or write outside a row's last block is
// an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../rdo-ptq_amd/csrc/mx_block_bits.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    long records = 0, blocks = 0;
    int32_t head[4];
    while (std::fread(head, sizeof(int32_t), 4, f) == 4) {
        const int bits = head[0];
        const long rows = head[1], inner = head[2], row_bytes = head[3];
        const long nb = (inner + 31) / 32;
        if ((bits != 4 && bits != 6 && bits != 8) || rows < 1 || inner < 1 || row_bytes != nb * 4 * bits) {
            std::fprintf(stderr, "record %ld: bad head %d %ld %ld %ld\n", records, bits, rows, inner, row_bytes);
            return 1;
        }
        std::vector<uint8_t> codes((size_t)(rows * inner)), want((size_t)(rows * row_bytes));
        if (std::fread(codes.data(), 1, codes.size(), f) != codes.size() || std::fread(want.data(), 1, want.size(), f) != want.size()) {
            std::fprintf(stderr, "record %ld: truncated\n", records);
            return 1;
        }
        std::vector<uint32_t> packed((size_t)(rows * nb * bits));
        for (long at = 0; at < rows * nb * bits; ++at) {                         // mx_pack_rows_kernel's index arithmetic
            const long g = at / bits;
            const int d = (int)(at - g * bits);
            const long row = g / nb, kb = g - row * nb;
            const long left = inner - kb * 32;
            packed[(size_t)at] = mx_block_word(codes.data() + row * inner + kb * 32, left < 32 ? (int)left : 32, bits, d);
        }
        if (std::memcmp(packed.data(), want.data(), want.size()) != 0) {         // (a little-endian host, as the file format is)
            std::fprintf(stderr, "record %ld (bits %d, %ld x %ld): packed bytes differ from the reference\n", records, bits, rows, inner);
            return 1;
        }
        std::vector<uint32_t> image(want.size() / 4);                            // unpack from the reference's bytes
        std::memcpy(image.data(), want.data(), want.size());
        for (long g = 0; g < rows * nb; ++g) {                                   // mx_unpack_dequant_kernel's index arithmetic
            const long row = g / nb, kb = g - row * nb;
            for (int lane = 0; lane < 32; ++lane) {
                const long i = kb * 32 + lane;
                if (i >= inner) continue;
                const uint32_t c = mx_block_element(image.data() + g * bits, bits, lane);
                if (c != (uint32_t)(codes[(size_t)(row * inner + i)] & ((1u << bits) - 1u))) {
                    std::fprintf(stderr, "record %ld (bits %d, %ld x %ld): element (%ld, %ld) is %u\n", records, bits, rows, inner, row, i, c);
                    return 1;
                }
            }
            ++blocks;
        }
        ++records;
    }
    std::fclose(f);
    if (records == 0) {
        std::fprintf(stderr, "no record read\n");
        return 1;
    }
    std::printf("mx_block_bits_check ok: %ld records, %ld blocks\n", records, blocks);
    return 0;
}
