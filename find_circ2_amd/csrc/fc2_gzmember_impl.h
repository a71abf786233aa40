// fc2_gzmember_impl.h -- the gzip member of a piece that fc2_deflate_launch_hist (include/fc2_caller.h)
// compressed with a history: the rule itself, host code over the launch's tables -- the tiles' stream lengths
// and CRC-32s, the piece's input size and the tile size -- used by fc2_deflate_gpu.hip and, alone, by
// tests/c/gz_member_main.cpp.
//
// With a history the tiles' streams are the parts of one raw DEFLATE stream (every one but the last ends on a
// byte boundary with BFINAL = 0; fc2_deflate.hip), so a piece of n_tiles tiles is one member (RFC 1952):
//   10 bytes  1f 8b 08 00 00 00 00 00 00 ff
//   the tiles' streams back to back: out_len[i] bytes from slots + i * stride, i = 0 .. n_tiles - 1
//    8 bytes  the CRC-32 of the piece's input, then ISIZE: its input bytes modulo 2^32 (little-endian)
// The piece's CRC-32 is combined from the tiles' (zlib's crc32_combine): tile i holds `tile` bytes, the last
// one the rest of n_bytes.
//
// A tile is invalid if its out_len is 0xFFFFFFFF (the compressor gave it up), 0, or more than
// FC2_DEFLATE_TILE_BOUND(tile).  One invalid tile makes the whole piece unwritten: member_size is 0, and the
// caller compresses the piece itself.
#pragma once
#include <stdint.h>
#include <string.h>
#include <zlib.h>

#include "../../include/fc2_caller.h"

namespace fc2 {
namespace gzm {

constexpr uint32_t kHead = 10, kTail = 8;

// the arguments a piece can have: tile 1..65536, at least one tile, the last one holding 1..tile bytes
inline bool piece_ok(uint64_t n_tiles, uint64_t n_bytes, uint32_t tile) {
    if (!tile || tile > 65536u || !n_tiles) return false;
    return n_bytes > (n_tiles - 1) * tile && n_bytes <= n_tiles * tile;
}

inline bool tile_ok(uint32_t out_len, uint32_t tile) {
    return out_len != 0xFFFFFFFFu && out_len != 0 && out_len <= FC2_DEFLATE_TILE_BOUND(tile);
}

// the input bytes of tile i, and the member's ISIZE
inline uint32_t tile_bytes(uint64_t i, uint64_t n_tiles, uint64_t n_bytes, uint32_t tile) {
    return i + 1 < n_tiles ? tile : (uint32_t)(n_bytes - (n_tiles - 1) * tile);
}
inline uint32_t isize_of(uint64_t n_bytes) { return (uint32_t)(n_bytes & 0xFFFFFFFFull); }

// the piece's CRC-32 from its tiles'
inline uint32_t piece_crc(const uint32_t *crc, uint64_t n_tiles, uint64_t n_bytes, uint32_t tile) {
    uLong c = crc[0];
    for (uint64_t i = 1; i < n_tiles; ++i) c = crc32_combine(c, crc[i], (z_off_t)tile_bytes(i, n_tiles, n_bytes, tile));
    return (uint32_t)c;
}

// the member's bytes; 0: the arguments are refused or a tile is invalid
inline uint64_t member_size(const uint32_t *out_len, uint64_t n_tiles, uint64_t n_bytes, uint32_t tile) {
    if (!piece_ok(n_tiles, n_bytes, tile)) return 0;
    uint64_t total = kHead + kTail;
    for (uint64_t i = 0; i < n_tiles; ++i) {
        if (!tile_ok(out_len[i], tile)) return 0;
        total += out_len[i];
    }
    return total;
}

// the member into out (member_size bytes, not 0); nothing outside them is written
inline void member_write(const uint8_t *slots, uint64_t stride, const uint32_t *out_len, const uint32_t *crc,
                         uint64_t n_tiles, uint64_t n_bytes, uint32_t tile, uint8_t *out) {
    static const uint8_t head[kHead] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    memcpy(out, head, kHead);
    uint8_t *d = out + kHead;
    for (uint64_t i = 0; i < n_tiles; ++i) {
        memcpy(d, slots + i * stride, out_len[i]);
        d += out_len[i];
    }
    const uint32_t c = piece_crc(crc, n_tiles, n_bytes, tile), isize = isize_of(n_bytes);
    for (int b = 0; b < 4; ++b) d[b] = (uint8_t)(c >> (8 * b));
    for (int b = 0; b < 4; ++b) d[4 + b] = (uint8_t)(isize >> (8 * b));
}

}  // namespace gzm
}  // namespace fc2
