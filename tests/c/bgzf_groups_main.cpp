// bgzf_groups_main.cpp -- the host code of BGZF blocks made of several tiles, alone, for a host build with
// sanitizers: (1) crc_append of csrc/fc2_bgzf_frame_impl.h against zlib's crc32 over split buffers; (2)
// frame_groups on the sweep of tests/test_bgzf_frame_groups_host.py into a heap buffer of exactly `total`
// bytes, so a byte written past it is an error of the sanitizer's, the blocks checked field by field, an invalid
// out_len and a block past 65536 bytes leaving the output untouched; (3) the BAM writer's mode 2 with tiles
// (csrc/fc2_bamout.cpp compiled into this program, the device's entry points stubbed out: mode 2 never calls
// them): records through pieces of 1 and 3 blocks of 0xff00 and 4096 bytes in tiles with a history, the file
// read back member by member.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../../find_circ2_amd/csrc/fc2_bamout.cpp"
#include "../../find_circ2_amd/csrc/fc2_bgzf_frame_impl.h"

using namespace fc2::bgzf;

// ---- what fc2_bamout.cpp links against in the library ----
namespace fc2 {
namespace bgz {
Gpu *gpu_open(int, uint32_t, uint32_t, double, int, uint32_t, uint32_t, std::string &err) {
    err = "no device in this program";
    return nullptr;
}
void gpu_close(Gpu *) {}
bool gpu_hung(const Gpu *) { return false; }
bool gpu_submit(Gpu *, int, const char *, size_t, std::string &) { return false; }
Wait gpu_collect(Gpu *, int, const uint8_t *&, size_t &, std::string &) { return FAILED; }
}  // namespace bgz
}  // namespace fc2

extern "C" uint64_t fc2_deflate_group_tiles(uint64_t n_bytes, uint32_t group, uint32_t tile) {
    const uint64_t tpg = (group - 1u) / tile + 1u, rest = n_bytes % group;
    return n_bytes / group * tpg + (rest + tile - 1) / tile;
}
extern "C" int fc2_bgzf_frame_host(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                                   uint32_t n_tiles, uint64_t n_bytes, uint32_t tile, uint8_t *out, uint32_t *off,
                                   uint32_t *total) {
    if (!piece_ok(n_tiles, n_bytes, tile)) return -1;
    frame_piece(slots, stride, out_len, crc, n_tiles, n_bytes, tile, out, off, total);
    return 0;
}
extern "C" int fc2_bgzf_frame_groups_host(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                                          uint32_t n_tiles, uint64_t n_bytes, uint32_t group, uint32_t tile, uint8_t *out,
                                          uint32_t *off, uint32_t *total) {
    *total = 0;
    if (!groups_ok(n_tiles, n_bytes, group, tile) || stride < FC2_DEFLATE_TILE_BOUND(tile)) return -1;
    frame_groups(slots, stride, out_len, crc, n_tiles, n_bytes, group, tile, out, off, total);
    return 0;
}

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

static int fail(const char *what, uint32_t a, uint32_t b) {
    printf("FAILED: %s at %u, %u\n", what, a, b);
    return 1;
}

static int check_combine() {
    std::vector<uint8_t> buf(70000);
    for (uint8_t &b : buf) b = (uint8_t)(rnd() >> 24);
    const uint32_t lens[] = {1, 2, 255, 256, 257, 16320, 65280};
    for (uint32_t nb : lens)
        for (uint32_t na : {1u, 4097u}) {
            const uint32_t a = (uint32_t)crc32(0L, buf.data(), na), b = (uint32_t)crc32(0L, buf.data() + na, nb);
            if (crc_append(a, b, nb) != (uint32_t)crc32(0L, buf.data(), na + nb)) return fail("crc_append", na, nb);
        }
    if (crc_shift(0x12345678u, 0) != 0x12345678u) return fail("crc_shift by nothing", 0, 0);
    return 0;
}

static int check_frame() {
    const uint32_t tile = 64, stride = (FC2_DEFLATE_TILE_BOUND(tile) + 15u) & ~15u;
    for (uint32_t n_groups : {1u, 2u, 3u, 65u})
        for (uint32_t tpg : {1u, 2u, 4u, 16u}) {
            const uint32_t group = tpg * tile - (tpg > 1 ? 7 : 0);
            const uint32_t last = n_groups > 1 || tpg > 1 ? (tpg - 1) * tile + 1 : 7;      // the last tile: 1 byte
            const uint64_t n_bytes = (uint64_t)(n_groups - 1) * group + last;
            const uint32_t n = (uint32_t)fc2_deflate_group_tiles(n_bytes, group, tile);
            if (!groups_ok(n, n_bytes, group, tile) || groups_ok(n + 1, n_bytes, group, tile)) return fail("groups_ok", n_groups, tpg);
            std::vector<uint8_t> slots((size_t)n * stride);
            for (uint8_t &b : slots) b = (uint8_t)(rnd() >> 24);
            std::vector<uint32_t> len(n), crc(n), off(n_groups + 1);
            uint32_t want = 26 * n_groups;
            for (uint32_t i = 0; i < n; ++i) {
                len[i] = i == n / 2 ? tile + 5 : 1 + i % 40;
                crc[i] = rnd();
                want += len[i];
            }
            std::vector<uint8_t> out(want);     // exactly the piece: one byte more is a heap overflow
            uint32_t total = 1;
            frame_groups(slots.data(), stride, len.data(), crc.data(), n, n_bytes, group, tile, out.data(), off.data(), &total);
            if (total != want || off[n_groups] != want) return fail("total", n_groups, tpg);
            uint32_t at = 0;
            for (uint32_t g = 0; g < n_groups; ++g) {
                if (off[g] != at) return fail("offset", n_groups, g);
                const uint32_t gbytes = group_bytes(g, n_groups, n_bytes, group), cnt = group_tile_count(gbytes, tile);
                const uint8_t *b = out.data() + at;
                uint32_t plen = 0, c = 0;
                for (uint32_t k = 0; k < cnt; ++k) {
                    const uint32_t i = g * tpg + k;
                    if (memcmp(b + 18 + plen, slots.data() + (size_t)i * stride, len[i])) return fail("stream", g, k);
                    plen += len[i];
                    c = k ? crc_append(c, crc[i], group_tile_bytes(k, gbytes, tile)) : crc[i];
                }
                uint32_t got_crc, got_isize;
                memcpy(&got_crc, b + 18 + plen, 4);
                memcpy(&got_isize, b + 22 + plen, 4);
                if (b[0] != 0x1f || b[1] != 0x8b || b[12] != 'B' || b[13] != 'C' || (uint32_t)(b[16] | b[17] << 8) != 26 + plen - 1)
                    return fail("header", n_groups, g);
                if (got_crc != c || got_isize != gbytes) return fail("trailer", n_groups, g);
                at += 26 + plen;
            }
            // an invalid length, and a block past 65536 bytes: nothing written (a buffer of one byte)
            std::vector<uint8_t> none(1, 0xC3);
            for (uint32_t bad : {0xFFFFFFFFu, 0u, FC2_DEFLATE_TILE_BOUND(tile) + 1}) {
                std::vector<uint32_t> l2 = len;
                l2[n / 3] = bad;
                frame_groups(slots.data(), stride, l2.data(), crc.data(), n, n_bytes, group, tile, none.data(), off.data(), &total);
                if (total != 0 || none[0] != 0xC3) return fail("an invalid tile", n_groups, tpg);
                for (uint32_t g = 0; g <= n_groups; ++g)
                    if (off[g]) return fail("offsets of an invalid piece", n_groups, g);
            }
        }
    {   // 16 valid tiles (4080 bytes each, at most 4096 of stream) whose block is one byte past 65536
        const uint32_t group = 0xff00, t16 = 0xff00 / 16, st = (FC2_DEFLATE_TILE_BOUND(t16) + 15u) & ~15u;
        std::vector<uint8_t> slots((size_t)16 * st), none(1, 0xC3);
        std::vector<uint32_t> len(16, 4096), crc(16), off(2);
        len[15] = 65510 - 15 * 4096 + 1;
        uint32_t total = 1;
        frame_groups(slots.data(), st, len.data(), crc.data(), 16, group, group, t16, none.data(), off.data(), &total);
        if (total != 0 || none[0] != 0xC3) return fail("a block past 64 KiB", 0, 0);
        len[15] -= 1;
        std::vector<uint8_t> out(65536);
        frame_groups(slots.data(), st, len.data(), crc.data(), 16, group, group, t16, out.data(), off.data(), &total);
        if (total != 65536) return fail("a block of 64 KiB", 0, 0);
    }
    return 0;
}

// the file's gzip members inflated one after the other
static bool inflate_file(const std::string &path, std::string &data, std::vector<uint32_t> &isizes) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    std::vector<uint8_t> blob;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, fp)) > 0;) blob.insert(blob.end(), buf, buf + k);
    fclose(fp);
    size_t at = 0;
    std::vector<uint8_t> out(65536);
    while (at < blob.size()) {
        if (at + 18 > blob.size()) return false;
        const size_t bsize = (size_t)(blob[at + 16] | blob[at + 17] << 8) + 1;
        if (at + bsize > blob.size()) return false;
        z_stream z{};
        if (inflateInit2(&z, -15) != Z_OK) return false;
        z.next_in = blob.data() + at + 18;
        z.avail_in = (uInt)(bsize - 26);
        z.next_out = out.data();
        z.avail_out = (uInt)out.size();
        const int rc = inflate(&z, Z_FINISH);
        const size_t n = out.size() - z.avail_out;
        inflateEnd(&z);
        uint32_t crc, isize;
        memcpy(&crc, blob.data() + at + bsize - 8, 4);
        memcpy(&isize, blob.data() + at + bsize - 4, 4);
        if (rc != Z_STREAM_END || z.avail_in != 0 || isize != n || crc != (uint32_t)crc32(0L, out.data(), (uInt)n)) return false;
        data.append((const char *)out.data(), n);
        isizes.push_back(isize);
        at += bsize;
    }
    return true;
}

static int check_writer(const char *dir) {
    // records of 60..259 bytes: block_size and a body of text-like bytes
    std::vector<std::string> recs;
    size_t bytes = 0;
    while (bytes < 5 * 0xff00 + 777) {
        const uint32_t n = 60 + rnd() % 200;
        std::string r(4 + n, '\0');
        memcpy(&r[0], &n, 4);
        for (uint32_t k = 0; k < n; ++k) r[4 + k] = (char)("ACGTN#IIHG"[rnd() % 10]);
        bytes += r.size();
        recs.push_back(r);
    }
    int run = 0;
    for (uint32_t block : {0xff00u, 4096u})
        for (uint32_t piece_blocks : {1u, 3u})
            for (uint32_t tile : {0u, block / 4, block / 16 + 1}) {
                std::string err, want, got;
                std::vector<uint32_t> want_isize, got_isize;
                const std::string a = std::string(dir) + "/plain" + std::to_string(run) + ".bam",
                                  b = std::string(dir) + "/tiles" + std::to_string(run) + ".bam";
                ++run;
                for (int pass = 0; pass < 2; ++pass) {
                    fc2::bam::Writer *w = fc2::bam::open_writer(pass ? b : a, "@HD\tVN:1.0\n", {"chr1"}, {1000}, err, 1);
                    if (!w) return fail("open_writer", block, tile);
                    // (pass 0: the same cut without tiles, the reference for the bytes and the ISIZE sequence)
                    if (!fc2::bam::set_device(w, 2, 0, block, piece_blocks, 0, 1, pass ? tile : 0, pass ? 32768 : 0, err))
                        return fail("set_device", block, tile);
                    for (const std::string &r : recs)
                        if (!fc2::bam::write_raw(w, (const uint8_t *)r.data(), r.size())) return fail("write_raw", block, tile);
                    uint64_t gp = 0, cp = 0;
                    if (!fc2::bam::close_writer(w, err, &gp, &cp)) return fail("close_writer", block, tile);
                    const size_t piece = (size_t)block * piece_blocks;
                    if (cp != 0 || gp != (bytes + piece - 1) / piece) return fail("pieces", (uint32_t)gp, (uint32_t)cp);
                }
                if (!inflate_file(a, want, want_isize) || !inflate_file(b, got, got_isize)) return fail("inflate", block, tile);
                if (want != got || want_isize != got_isize) return fail("the tiles' file", block, tile);
            }
    // what set_device refuses
    std::string err;
    fc2::bam::Writer *w = fc2::bam::open_writer(std::string(dir) + "/refused.bam", "", {"chr1"}, {1000}, err, 1);
    if (!w) return fail("open_writer", 0, 0);
    if (fc2::bam::set_device(w, 2, 0, 0xff00, 1, 0, 1, 0xff00 / 17, 0, err)) return fail("17 tiles taken", 0, 0);
    if (fc2::bam::set_device(w, 2, 0, 0xff00, 1, 0, 1, 40000, 32768, err)) return fail("tile + hist over 65536 taken", 0, 0);
    if (fc2::bam::set_device(w, 2, 0, 0xff00, 1, 0, 1, 16320, 32769, err)) return fail("hist over 32768 taken", 0, 0);
    if (!fc2::bam::close_writer(w, err)) return fail("close_writer", 0, 0);
    return 0;
}

int main(int argc, char **argv) {
    if (check_combine() || check_frame() || check_writer(argc > 1 ? argv[1] : "/tmp")) return 1;
    printf("ok\n");
    return 0;
}
