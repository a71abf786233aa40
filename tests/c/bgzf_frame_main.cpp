// bgzf_frame_main.cpp -- the framing rule of csrc/fc2_bgzf_frame_impl.h alone, for a host build with
// sanitizers: the alignment sweep of tests/test_bgzf_frame_host.py (out_len cycling 1..40, one tile of the
// stored form's length, a short last tile) into a heap buffer of exactly `total` bytes, so a byte written
// past it is an error of the sanitizer's; the block stream is checked field by field, and each invalid
// out_len must leave the output untouched.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../find_circ2_amd/csrc/fc2_bgzf_frame_impl.h"

using namespace fc2::bgzf;

static int fail(const char *what, uint32_t n_tiles) {
    printf("FAILED: %s at n_tiles = %u\n", what, n_tiles);
    return 1;
}

int main() {
    const uint32_t tile = 64, stride = (FC2_DEFLATE_TILE_BOUND(tile) + 15u) & ~15u;
    const uint32_t counts[] = {1, 2, 63, 64, 65, 130};
    for (uint32_t n_tiles : counts) {
        std::vector<uint8_t> slots((size_t)n_tiles * stride);
        uint32_t x = 12345u + n_tiles;
        for (uint8_t &b : slots) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
        std::vector<uint32_t> len(n_tiles), crc(n_tiles), off(n_tiles + 1);
        uint32_t want = 0;
        for (uint32_t i = 0; i < n_tiles; ++i) {
            len[i] = i == n_tiles / 2 ? tile + 5 : 1 + i % 40;
            crc[i] = (x = x * 1664525u + 1013904223u);
            want += 26 + len[i];
        }
        const uint64_t n_bytes = (uint64_t)(n_tiles - 1) * tile + 7;
        if (!piece_ok(n_tiles, n_bytes, tile)) return fail("piece_ok", n_tiles);
        std::vector<uint8_t> out(want);         // exactly the piece: one byte more is a heap overflow
        uint32_t total = 1;
        frame_piece(slots.data(), stride, len.data(), crc.data(), n_tiles, n_bytes, tile, out.data(), off.data(), &total);
        if (total != want || off[n_tiles] != want) return fail("total", n_tiles);
        uint32_t at = 0;
        for (uint32_t i = 0; i < n_tiles; ++i) {
            static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
            const uint8_t *b = out.data() + at;
            const uint32_t isize = i + 1 < n_tiles ? tile : 7, bsize = 26 + len[i];
            if (off[i] != at) return fail("offset", n_tiles);
            if (memcmp(b, head, 16) || b[16] != ((bsize - 1) & 0xff) || b[17] != (bsize - 1) >> 8) return fail("header", n_tiles);
            if (memcmp(b + 18, slots.data() + (size_t)i * stride, len[i])) return fail("stream", n_tiles);
            uint32_t c, n;
            memcpy(&c, b + 18 + len[i], 4);
            memcpy(&n, b + 22 + len[i], 4);
            if (c != crc[i] || n != isize) return fail("trailer", n_tiles);
            at += bsize;
        }
        const uint32_t bad[] = {0xFFFFFFFFu, 0u, FC2_DEFLATE_TILE_BOUND(tile) + 1u};
        for (uint32_t v : bad) {
            std::vector<uint32_t> l2(len);
            l2[n_tiles - 1] = v;
            std::vector<uint8_t> none(1, 0xC3);
            frame_piece(slots.data(), stride, l2.data(), crc.data(), n_tiles, n_bytes, tile, none.data(), off.data(), &total);
            if (total != 0 || none[0] != 0xC3 || off[0] != 0 || off[n_tiles] != 0) return fail("invalid tile", n_tiles);
        }
    }
    if (piece_ok(1, 0xff01, 0xff01) || !piece_ok(1, 0xff00, 0xff00) || piece_ok(2, 64, 64) || piece_ok(2, 129, 64))
        return fail("piece_ok's limits", 0);
    if (tile_ok(0xff00 + 17, 0xff00) || !tile_ok(0xff00 + 5, 0xff00)) return fail("tile_ok's limits", 0);
    printf("ok\n");
    return 0;
}
