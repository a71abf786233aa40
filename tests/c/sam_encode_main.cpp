// sam_encode_main.cpp -- the host code of BAM records from SAM text, alone, for a host build with sanitizers:
// (1) the rule of csrc/fc2_sam_encode_impl.h over the lines of a file (tests/test_sam_encode_host.py writes the
// planted lines, the refused ones and a slice of the mutations: a 4-byte length, then the line) into a heap buffer
// of exactly the batch's total, so a byte written past it is an error of the sanitizer's, every accepted line
// compared with encode_sam; (2) the -B writer's encode stage in its stand-in mode (csrc/fc2_bamout.cpp and
// fc2_bamout_sam.cpp compiled into this program, the device's entry points stubbed out: mode 2 never calls them)
// over the lines encode_sam takes, at batch caps of 1, 2, 63, 64 and 65 lines, the file compared with the plain
// writer's; and with a line encode_sam fails on in the middle: the same message, the same file.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../find_circ2_amd/csrc/fc2_bamout.cpp"
#include "../../find_circ2_amd/csrc/fc2_bamout_sam.cpp"
#include "../../find_circ2_amd/csrc/fc2_bgzf_frame_impl.h"
#include "../../find_circ2_amd/csrc/fc2_sam_encode_impl.h"

// ---- what the two files link against in the library ----
namespace fc2 {
int fail(int code, const std::string &) { return code; }
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
namespace samenc {
std::vector<uint32_t> names_table(const std::vector<std::string> &names) {
    std::vector<const char *> p(names.size());
    std::vector<uint32_t> l(names.size());
    for (size_t i = 0; i < names.size(); ++i) p[i] = names[i].data(), l[i] = (uint32_t)names[i].size();
    return build_table(p.data(), l.data(), (uint32_t)names.size());
}
Gpu *gpu_open(int, uint32_t, uint32_t, double, const std::vector<uint32_t> &, std::string &err) {
    err = "no device in this program";
    return nullptr;
}
void gpu_close(Gpu *) {}
bool gpu_hung(const Gpu *) { return false; }
char *gpu_text(Gpu *, int) { return nullptr; }
uint32_t *gpu_off(Gpu *, int) { return nullptr; }
bool gpu_submit(Gpu *, int, uint32_t, std::string &) { return false; }
Wait gpu_collect(Gpu *, int, const uint32_t *&, const uint8_t *&, size_t &, std::string &) { return FAILED; }
}  // namespace samenc
}  // namespace fc2

extern "C" uint64_t fc2_deflate_group_tiles(uint64_t n_bytes, uint32_t group, uint32_t tile) {
    const uint64_t tpg = (group - 1u) / tile + 1u, rest = n_bytes % group;
    return n_bytes / group * tpg + (rest + tile - 1) / tile;
}
extern "C" int fc2_bgzf_frame_host(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                                   uint32_t n_tiles, uint64_t n_bytes, uint32_t tile, uint8_t *out, uint32_t *off,
                                   uint32_t *total) {
    if (!fc2::bgzf::piece_ok(n_tiles, n_bytes, tile)) return -1;
    fc2::bgzf::frame_piece(slots, stride, out_len, crc, n_tiles, n_bytes, tile, out, off, total);
    return 0;
}
extern "C" int fc2_bgzf_frame_groups_host(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                                          uint32_t n_tiles, uint64_t n_bytes, uint32_t group, uint32_t tile, uint8_t *out,
                                          uint32_t *off, uint32_t *total) {
    *total = 0;
    if (!fc2::bgzf::groups_ok(n_tiles, n_bytes, group, tile) || stride < FC2_DEFLATE_TILE_BOUND(tile)) return -1;
    fc2::bgzf::frame_groups(slots, stride, out_len, crc, n_tiles, n_bytes, group, tile, out, off, total);
    return 0;
}
extern "C" int fc2_sam_encode_host(const uint8_t *text, uint32_t text_bytes, const uint32_t *off, uint32_t n_lines,
                                   const uint32_t *names_table, uint32_t table_bytes, uint8_t *out, uint64_t out_cap,
                                   uint32_t *out_off, uint32_t *size, uint32_t *status, uint32_t *total) {
    if (!n_lines || n_lines > fc2::samenc::kMaxLines || text_bytes > fc2::samenc::kMaxText ||
        out_cap < FC2_SAM_ENC_BOUND(text_bytes, n_lines))
        return -1;
    fc2::samenc::encode_batch(text, text_bytes, off, n_lines, names_table, table_bytes, out, out_cap, out_off, size, status, total);
    return 0;
}

static int fail(const char *what, size_t a, size_t b) {
    printf("FAILED: %s at %zu, %zu\n", what, a, b);
    return 1;
}

static const std::vector<std::string> kNames = {"chr1", "chr2", "chrX", "dup", "chr3", "dup"};

static bool read_lines(const char *path, std::vector<std::string> &lines) {
    FILE *fp = fopen(path, "rb");
    if (!fp) return false;
    uint32_t n;
    while (fread(&n, 4, 1, fp) == 1) {
        std::string s(n, '\0');
        if (n && fread(&s[0], 1, n, fp) != n) { fclose(fp); return false; }
        lines.push_back(s);
    }
    fclose(fp);
    return true;
}

static int check_rule(const std::vector<std::string> &lines, const std::unordered_map<std::string, int> &tid_of) {
    const std::vector<uint32_t> table = fc2::samenc::names_table(kNames);
    const uint32_t tb = (uint32_t)(table.size() * 4);
    size_t accepted = 0;
    for (size_t i0 = 0; i0 < lines.size();) {
        // a batch: up to 1000 lines and 1 MiB; the text in a buffer of exactly its bytes
        size_t i1 = i0, nb = 0;
        while (i1 < lines.size() && i1 - i0 < 1000 && nb + lines[i1].size() <= (1u << 20)) nb += lines[i1++].size();
        if (i1 == i0) return fail("a line over 1 MiB", i0, 0);
        const uint32_t n = (uint32_t)(i1 - i0);
        std::vector<uint8_t> text(nb ? nb : 1);
        std::vector<uint32_t> off(n + 1, 0), out_off(n + 1), size(n), status(n);
        for (uint32_t k = 0; k < n; ++k) {
            memcpy(text.data() + off[k], lines[i0 + k].data(), lines[i0 + k].size());
            off[k + 1] = off[k] + (uint32_t)lines[i0 + k].size();
        }
        uint32_t total = 0;
        std::vector<uint8_t> none(1, 0xC3);      // the sizes first: with no room nothing is written
        fc2::samenc::encode_batch(text.data(), (uint32_t)nb, off.data(), n, table.data(), tb, none.data(), 0, out_off.data(),
                                  size.data(), status.data(), &total);
        if (none[0] != 0xC3) return fail("written without room", i0, 0);
        if (total > FC2_SAM_ENC_BOUND(nb, n)) return fail("the bound", i0, total);
        std::vector<uint8_t> out(total ? total : 1);    // exactly the batch: one byte more is a heap overflow
        uint32_t total2 = 0;
        fc2::samenc::encode_batch(text.data(), (uint32_t)nb, off.data(), n, table.data(), tb, out.data(), total, out_off.data(),
                                  size.data(), status.data(), &total2);
        if (total2 != total || out_off[n] != total) return fail("total", i0, total2);
        for (uint32_t k = 0; k < n; ++k) {
            const std::string &l = lines[i0 + k];
            if ((status[k] == 0) != (size[k] != 0)) return fail("status and size", i0 + k, status[k]);
            if (size[k] > fc2::samenc::record_bound(l.size())) return fail("a record's bound", i0 + k, size[k]);
            if (status[k]) continue;
            std::string rec, err;
            if (!fc2::bam::encode_sam(l.data(), l.data() + l.size(), tid_of, rec, err)) return fail("accepted, but encode_sam fails", i0 + k, 0);
            if (rec.size() != size[k] || memcmp(rec.data(), out.data() + out_off[k], rec.size())) return fail("a wrong byte", i0 + k, size[k]);
            ++accepted;
        }
        i0 = i1;
    }
    if (!accepted || accepted == lines.size()) return fail("both sides of the contract", accepted, lines.size());
    return 0;
}

static std::string slurp(const std::string &path) {
    std::string s;
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return s;
    char buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, fp)) > 0;) s.append(buf, k);
    fclose(fp);
    return s;
}

// the lines through write_sam; stops at the first failure (its message in msg) as the read loop does, then closes
static bool run_writer(const std::string &path, const std::vector<std::string> &lines, const std::unordered_map<std::string, int> &tid_of,
                       int mode, uint32_t max_lines, uint32_t max_text, std::string &msg, uint64_t &g, uint64_t &h) {
    std::string err;
    fc2::bam::Writer *w = fc2::bam::open_writer(path, "@HD\tVN:1.0\n", kNames, {1000, 1000, 1000, 1000, 1000, 1000}, err, 1);
    if (!w) return false;
    if (mode && !fc2::bam::set_encode(w, mode, 0, kNames, &tid_of, max_lines, max_text, 0, err)) return false;
    msg.clear();
    for (const std::string &l : lines)
        if (!fc2::bam::write_sam(w, l.data(), l.data() + l.size(), tid_of, msg)) break;
    std::string cerr_;
    const bool ok = fc2::bam::close_writer(w, cerr_, nullptr, nullptr, &g, &h);
    if (!ok && msg.empty()) msg = cerr_;
    return true;
}

static int check_writer(const std::vector<std::string> &lines, const std::unordered_map<std::string, int> &tid_of, const char *dir) {
    std::vector<std::string> good;
    std::string bad;
    for (const std::string &l : lines) {
        std::string rec, err;
        if (fc2::bam::encode_sam(l.data(), l.data() + l.size(), tid_of, rec, err)) good.push_back(l);
        else if (bad.empty()) bad = l;
    }
    if (good.size() < 500 || bad.empty()) return fail("the lines", good.size(), 0);
    const std::string d(dir);
    std::string msg0, msg;
    uint64_t g = 0, h = 0;
    if (!run_writer(d + "/plain.bam", good, tid_of, 0, 0, 0, msg0, g, h) || !msg0.empty()) return fail("the plain writer", 0, 0);
    const std::string want = slurp(d + "/plain.bam");
    for (uint32_t cap : {1u, 2u, 63u, 64u, 65u}) {
        if (!run_writer(d + "/enc.bam", good, tid_of, 2, cap, cap == 1 ? 0 : 20000, msg, g, h) || !msg.empty()) return fail("the stage", cap, 0);
        if (slurp(d + "/enc.bam") != want) return fail("the stage's file", cap, 0);
        if (g + h <= 4 || !h || (cap > 2 && !g)) return fail("the batches", (size_t)g, (size_t)h);
    }
    // a line of its own batch-filling length goes through the host, in its place
    if (!run_writer(d + "/enc.bam", good, tid_of, 2, 64, 300, msg, g, h) || !msg.empty() || slurp(d + "/enc.bam") != want)
        return fail("lines over the text cap", 0, 0);
    // a failing line in the middle: the message and the file of the plain writer
    std::vector<std::string> broken(good.begin(), good.begin() + 400);
    broken.insert(broken.begin() + 200, bad);
    if (!run_writer(d + "/plain_bad.bam", broken, tid_of, 0, 0, 0, msg0, g, h) || msg0.empty()) return fail("the plain writer's error", 0, 0);
    for (uint32_t cap : {7u, 64u, 1000u}) {
        if (!run_writer(d + "/enc_bad.bam", broken, tid_of, 2, cap, 0, msg, g, h)) return fail("the stage", cap, 1);
        if (msg != msg0) return fail("the stage's message", cap, 0);
        if (slurp(d + "/enc_bad.bam") != slurp(d + "/plain_bad.bam")) return fail("the stage's file after an error", cap, 0);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return fail("usage: sam_encode_main LINES DIR", 0, 0);
    std::vector<std::string> lines;
    if (!read_lines(argv[1], lines) || lines.empty()) return fail("no lines", 0, 0);
    std::unordered_map<std::string, int> tid_of;
    for (size_t i = 0; i < kNames.size(); ++i) tid_of[kNames[i]] = (int)i;
    if (check_rule(lines, tid_of) || check_writer(lines, tid_of, argv[2])) return 1;
    printf("ok\n");
    return 0;
}
