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

// ---- groups: a block made of several tiles (fc2_deflate_launch_groups, fc2_bgzf_frame_groups_launch) ----
//
// The piece's n_bytes are cut into groups of `group` input bytes (1..0xff00, the last group holding the rest)
// and every group into tiles of `tile` bytes: a whole group has tpg = ceil(group / tile) tiles, tile g * tpg + k
// is the k-th of group g, only the last group can have fewer.  Group g becomes one BGZF block at off[g]:
//   18 bytes  the header above with BSIZE - 1
//   the streams of the group's tiles back to back in order (together one raw DEFLATE stream)
//    8 bytes  the group's CRC-32, combined from its tiles' CRCs and lengths (crc_append), then ISIZE: the
//             group's input bytes
// off[] has n_groups + 1 entries, total = off[n_groups].  Every tile must pass tile_ok, and every block's
// 26 + (the sum of its tiles' out_len) must be at most 65536; one failure anywhere leaves the piece unwritten
// as above.
//
// tpg is at most 16, and that is a condition like the one above: a tile of n <= 65535 bytes that does not
// shrink is n + 5 bytes in either form, so a block of 0xff00 bytes stored in 16 tiles is at most
// 65280 + 16 * 5 + 26 = 65386 <= 65536 bytes; with 17 tiles or more nothing is promised, so they are refused.
constexpr uint32_t kTilesPerGroupMax = 16;
constexpr uint32_t kGroupsMax = 0xffff;         // blocks of one piece: total and every offset fit 32 bits
constexpr uint32_t kCrcPoly = 0xEDB88320u;      // the gzip CRC-32's polynomial, bit-reversed as the CRC itself is

FC2_BGZF_HD uint32_t tiles_per_group(uint32_t group, uint32_t tile) { return (group - 1u) / tile + 1u; }
FC2_BGZF_HD uint32_t groups_of(uint64_t n_bytes, uint32_t group) { return (uint32_t)((n_bytes + group - 1u) / group); }
// input bytes of group g of n_groups, and of its k-th tile; the tiles it has
FC2_BGZF_HD uint32_t group_bytes(uint32_t g, uint32_t n_groups, uint64_t n_bytes, uint32_t group) {
    return g + 1 < n_groups ? group : (uint32_t)(n_bytes - (uint64_t)(n_groups - 1) * group);
}
FC2_BGZF_HD uint32_t group_tile_count(uint32_t gbytes, uint32_t tile) { return (gbytes - 1u) / tile + 1u; }
FC2_BGZF_HD uint32_t group_tile_bytes(uint32_t k, uint32_t gbytes, uint32_t tile) {
    const uint32_t before = k * tile;
    return gbytes - before < tile ? gbytes - before : tile;
}

// the arguments a piece of groups can have
FC2_BGZF_HD bool groups_ok(uint32_t n_tiles, uint64_t n_bytes, uint32_t group, uint32_t tile) {
    if (!group || group > kTileMax || !tile || tile > 65536u || !n_bytes) return false;
    if (tiles_per_group(group, tile) > kTilesPerGroupMax) return false;
    const uint64_t n_groups = (n_bytes + group - 1u) / group;
    if (n_groups > kGroupsMax) return false;
    const uint32_t rest = (uint32_t)(n_bytes - (n_groups - 1) * group);
    return n_tiles == (n_groups - 1) * tiles_per_group(group, tile) + group_tile_count(rest, tile);
}

// a * b modulo the CRC polynomial (polynomials over GF(2), bit 31 the coefficient of x^0)
FC2_BGZF_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}
// crc * x^(8 n) modulo the polynomial, by square and multiply: what n more bytes do to the CRC of the bytes
// before them
FC2_BGZF_HD uint32_t crc_shift(uint32_t crc, uint32_t n) {
    uint32_t pw = 0x00800000u;                  // x^8
    for (; n; n >>= 1) {
        if (n & 1u) crc = crc_mul(pw, crc);
        pw = crc_mul(pw, pw);
    }
    return crc;
}
// the CRC-32 of A followed by B (n_b bytes) from theirs: the pre- and post-conditioning cancel (zlib's
// crc32_combine)
FC2_BGZF_HD uint32_t crc_append(uint32_t crc_a, uint32_t crc_b, uint32_t n_b) { return crc_shift(crc_a, n_b) ^ crc_b; }

// The host's form of the rule for groups (groups_ok): off[0 .. n_groups] and *total, the blocks into out (at
// least n_groups * 26 + n_tiles * FC2_DEFLATE_TILE_BOUND(tile) bytes, never more than 65536 a group)
inline void frame_groups(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                         uint32_t n_tiles, uint64_t n_bytes, uint32_t group, uint32_t tile, uint8_t *out, uint32_t *off,
                         uint32_t *total) {
    const uint32_t n_groups = groups_of(n_bytes, group), tpg = tiles_per_group(group, tile);
    bool ok = true;
    for (uint32_t i = 0; i < n_tiles; ++i) ok = ok && tile_ok(out_len[i], tile);
    for (uint32_t g = 0; g < n_groups && ok; ++g) {
        const uint32_t cnt = group_tile_count(group_bytes(g, n_groups, n_bytes, group), tile);
        uint32_t sum = kOverhead;
        for (uint32_t k = 0; k < cnt; ++k) sum += out_len[g * tpg + k];
        ok = sum <= kBlockMax;
    }
    if (!ok) {
        for (uint32_t g = 0; g <= n_groups; ++g) off[g] = 0;
        *total = 0;
        return;
    }
    uint32_t at = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t gbytes = group_bytes(g, n_groups, n_bytes, group), cnt = group_tile_count(gbytes, tile);
        uint8_t *d = out + at;
        off[g] = at;
        uint32_t len = 0, c = 0;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t i = g * tpg + k;
            const uint8_t *s = slots + (uint64_t)i * stride;
            for (uint32_t b = 0; b < out_len[i]; ++b) d[kHead + len + b] = s[b];
            len += out_len[i];
            c = k ? crc_append(c, crc[i], group_tile_bytes(k, gbytes, tile)) : crc[i];
        }
        const uint32_t bsize = block_bytes(len);
        for (uint32_t k = 0; k < kHead; ++k) d[k] = head_byte(k, bsize);
        for (uint32_t k = 0; k < kTail; ++k) d[kHead + len + k] = tail_byte(k, c, gbytes);
        at += bsize;
    }
    off[n_groups] = at;
    *total = at;
}

}  // namespace bgzf
}  // namespace fc2
