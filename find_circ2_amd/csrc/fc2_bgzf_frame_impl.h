// fc2_bgzf_frame_impl.h -- the BGZF form of a piece the GPU DEFLATE compressor left in its slots (include/
// fc2_caller.h fc2_bgzf_frame_launch): the rule itself, compiled twice -- into bgzf_frame_kernel
// (fc2_bgzf_out.hip) and into fc2_bgzf_frame_host (the same file's host side) -- over the same tables: the
// tiles' stream lengths and CRC-32s, the piece's input size and the tile size.
//
// Tile i of n_tiles (its raw DEFLATE stream: out_len[i] bytes at slots + i * stride) becomes one BGZF block
// (SAM/BAM spec 4.1) of 26 + out_len[i] bytes at off[i] = sum over j < i of (26 + out_len[j]):
//   18 bytes  1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00, then BSIZE - 1 (16 bits, little-endian)
//   out_len[i] bytes of the stream
//    8 bytes  the CRC-32 of the tile's input, then ISIZE: its input bytes (both 32 bits, little-endian)
// and total = off[n_tiles].  ISIZE is `tile` for every tile but the last, which holds the rest of n_bytes.
//
// A tile is invalid if its out_len is 0xFFFFFFFF (the compressor gave it up), 0, or more than
// FC2_DEFLATE_TILE_BOUND(tile); so is one whose block would exceed 65536 bytes.  One invalid tile makes the
// whole piece unwritten: total = 0, every offset 0, no byte of the output touched.
//
// The 64 KiB a block may take is a condition here, not a measurement: deflate_kernel (fc2_deflate.hip)
// writes a tile of n <= 65535 bytes that does not shrink as one stored block of n + 5 bytes, so at the
// largest tile, 0xff00, a block is at most 65280 + 5 + 26 = 65311 <= 65536 bytes; and whatever out_len
// says, a length over the tile's bound (0xff00 + 16: a block of 65322) is refused before it is framed.
#pragma once
#include <stdint.h>

#include "../../include/fc2_caller.h"

#if defined(__HIPCC__)
#define FC2_BGZF_HD __host__ __device__ inline
#else
#define FC2_BGZF_HD inline
#endif

namespace fc2 {
namespace bgzf {

constexpr uint32_t kTileMax = 0xff00;           // input bytes a block holds at most (htslib's BGZF_BLOCK_SIZE)
constexpr uint32_t kBlockMax = 65536;           // bytes a block takes at most: BSIZE - 1 is 16 bits wide
constexpr uint32_t kHead = 18, kTail = 8, kOverhead = kHead + kTail;
constexpr uint32_t kTilesMax = 0xffff;          // tiles of one piece: total and every offset fit 32 bits

// the arguments a piece can have: tile 1..0xff00, 1..kTilesMax tiles, the last one holding 1..tile bytes
FC2_BGZF_HD bool piece_ok(uint32_t n_tiles, uint64_t n_bytes, uint32_t tile) {
    if (!tile || tile > kTileMax || !n_tiles || n_tiles > kTilesMax) return false;
    return n_bytes > (uint64_t)(n_tiles - 1) * tile && n_bytes <= (uint64_t)n_tiles * tile;
}

FC2_BGZF_HD bool tile_ok(uint32_t out_len, uint32_t tile) {
    return out_len != 0xFFFFFFFFu && out_len != 0 && out_len <= FC2_DEFLATE_TILE_BOUND(tile) &&
           kOverhead + out_len <= kBlockMax;
}

// the bytes of tile i's block (tile_ok) and of its input
FC2_BGZF_HD uint32_t block_bytes(uint32_t out_len) { return kOverhead + out_len; }
FC2_BGZF_HD uint32_t isize_of(uint32_t i, uint32_t n_tiles, uint64_t n_bytes, uint32_t tile) {
    return i + 1 < n_tiles ? tile : (uint32_t)(n_bytes - (uint64_t)(n_tiles - 1) * tile);
}

// byte k (0..17) of the header of a block of bsize bytes
FC2_BGZF_HD uint8_t head_byte(uint32_t k, uint32_t bsize) {
    switch (k) {
        case 0: return 0x1f;
        case 1: return 0x8b;
        case 2: return 8;
        case 3: return 4;
        case 9: return 0xff;
        case 10: return 6;
        case 12: return 'B';
        case 13: return 'C';
        case 14: return 2;
        case 16: return (uint8_t)((bsize - 1) & 0xffu);
        case 17: return (uint8_t)((bsize - 1) >> 8);
        default: return 0;
    }
}

// byte k (0..7) of the trailer
FC2_BGZF_HD uint8_t tail_byte(uint32_t k, uint32_t crc, uint32_t isize) {
    return (uint8_t)((k < 4 ? crc : isize) >> (8u * (k & 3u)));
}

// The host's form of the whole rule (piece_ok): off[0 .. n_tiles] and *total, and the blocks into out (at
// least n_tiles * (26 + FC2_DEFLATE_TILE_BOUND(tile)) bytes); nothing outside [out, out + *total) is written
inline void frame_piece(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                        uint32_t n_tiles, uint64_t n_bytes, uint32_t tile, uint8_t *out, uint32_t *off, uint32_t *total) {
    bool ok = true;
    for (uint32_t i = 0; i < n_tiles; ++i) ok = ok && tile_ok(out_len[i], tile);
    if (!ok) {
        for (uint32_t i = 0; i <= n_tiles; ++i) off[i] = 0;
        *total = 0;
        return;
    }
    uint32_t at = 0;
    for (uint32_t i = 0; i < n_tiles; ++i) {
        const uint32_t len = out_len[i], bsize = block_bytes(len), isize = isize_of(i, n_tiles, n_bytes, tile);
        uint8_t *d = out + at;
        off[i] = at;
        for (uint32_t k = 0; k < kHead; ++k) d[k] = head_byte(k, bsize);
        const uint8_t *s = slots + (uint64_t)i * stride;
        for (uint32_t k = 0; k < len; ++k) d[kHead + k] = s[k];
        for (uint32_t k = 0; k < kTail; ++k) d[kHead + len + k] = tail_byte(k, crc[i], isize);
        at += bsize;
    }
    off[n_tiles] = at;
    *total = at;
}

}  // namespace bgzf
}  // namespace fc2
