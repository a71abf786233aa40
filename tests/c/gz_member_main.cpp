// gz_member_main.cpp -- the member rule of csrc/fc2_gzmember_impl.h alone, for a host build with sanitizers.
//   gz_member_main assemble IN OUT   IN: n_tiles, tile, stride (32 bits each), n_bytes (64), out_len[n_tiles],
//                                    crc[n_tiles], then the slots (n_tiles * stride bytes), little-endian.  The
//                                    member goes to OUT through a heap buffer of exactly member_size bytes, so
//                                    a byte written past it is an error of the sanitizer's; "unwritten" and an
//                                    empty OUT if member_size is 0.
//   gz_member_main arith N_TILES N_BYTES TILE CRC_FULL CRC_LAST
//                                    the length arithmetic alone, for pieces no buffer is made for: piece_ok,
//                                    ISIZE, the last tile's bytes, and the CRC-32 combined from N_TILES - 1 tiles
//                                    with CRC_FULL and a last one with CRC_LAST.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../find_circ2_amd/csrc/fc2_gzmember_impl.h"

using namespace fc2::gzm;

static bool read_all(const char *path, std::vector<uint8_t> &buf) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t tmp[65536];
    size_t k;
    while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + k);
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc == 7 && !strcmp(argv[1], "arith")) {
        const uint64_t n_tiles = strtoull(argv[2], nullptr, 10), n_bytes = strtoull(argv[3], nullptr, 10);
        const uint32_t tile = (uint32_t)strtoul(argv[4], nullptr, 10);
        const bool ok = piece_ok(n_tiles, n_bytes, tile);
        uint32_t c = 0, last = 0;
        if (ok) {
            std::vector<uint32_t> crc(n_tiles, (uint32_t)strtoul(argv[5], nullptr, 10));
            crc[n_tiles - 1] = (uint32_t)strtoul(argv[6], nullptr, 10);
            c = piece_crc(crc.data(), n_tiles, n_bytes, tile);
            last = tile_bytes(n_tiles - 1, n_tiles, n_bytes, tile);
        }
        printf("%d %u %u %u\n", ok ? 1 : 0, isize_of(n_bytes), last, c);
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "assemble")) {
        fprintf(stderr, "usage: gz_member_main assemble IN OUT | arith N_TILES N_BYTES TILE CRC_FULL CRC_LAST\n");
        return 2;
    }
    std::vector<uint8_t> in;
    if (!read_all(argv[2], in) || in.size() < 20) return 2;
    uint32_t n_tiles, tile, stride;
    uint64_t n_bytes;
    memcpy(&n_tiles, &in[0], 4);
    memcpy(&tile, &in[4], 4);
    memcpy(&stride, &in[8], 4);
    memcpy(&n_bytes, &in[12], 8);
    if (in.size() != 20 + (size_t)n_tiles * 8 + (size_t)n_tiles * stride) return 2;
    std::vector<uint32_t> len(n_tiles), crc(n_tiles);     // (copies: the file's fields are not aligned)
    memcpy(len.data(), &in[20], (size_t)n_tiles * 4);
    memcpy(crc.data(), &in[20 + (size_t)n_tiles * 4], (size_t)n_tiles * 4);
    std::vector<uint8_t> slots(in.begin() + 20 + (size_t)n_tiles * 8, in.end());
    const uint64_t size = member_size(len.data(), n_tiles, n_bytes, tile);
    FILE *f = fopen(argv[3], "wb");
    if (!f) return 2;
    if (!size) {
        fclose(f);
        printf("unwritten\n");
        return 0;
    }
    std::vector<uint8_t> out(size);                 // exactly the member: one byte more is a heap overflow
    member_write(slots.data(), stride, len.data(), crc.data(), n_tiles, n_bytes, tile, out.data());
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    printf("ok %llu\n", (unsigned long long)size);
    return ok ? 0 : 2;
}
