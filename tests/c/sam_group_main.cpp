// sam_group_main.cpp -- the host code of the unspliced fragments of SAM text closed on the device, alone, for a
// host build with sanitizers (csrc/fc2_sam_group.hip compiled into this program; its kernels are never launched):
// (1) the host twin fc2_sam_group_host over generated text -- generator-shaped lines, a third of them damaged, and
// the smallest blocks -- with the text, the starts and the rows in heap buffers of exactly their sizes, so a byte
// read or written past them is an error of the sanitizer's; at cap = n_lines, n_lines - 1 and 0; every closed row
// checked against the starts; (2) the stage's slots at setting 2 (fc2::samgrp, the stand-in without a device):
// every slot taken, submitted, collected and given back, the rows those of the twin; a block of more lines than
// rows, a block over the slot's text, a slot given back uncollected, a stage closed with slots still out; and a
// splitter thread with two parse threads passing 300 blocks through 3 slots.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include -x hip -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tests/c/sam_group_main.cpp -o sam_group_main -lpthread
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../find_circ2_amd/csrc/fc2_sam_group.hip"

namespace fc2 {
int fail(int code, const std::string &) { return code; }
}  // namespace fc2

static int failed(const char *what, size_t a, size_t b) {
    printf("FAILED: %s at %zu, %zu\n", what, a, b);
    return 1;
}

static const std::vector<std::string> kNames = {"chr1", "chr2", "chrX", "dup", "chr3", "dup"};

static std::vector<uint32_t> table_of() {
    std::vector<const char *> p;
    for (const std::string &s : kNames) p.push_back(s.c_str());
    return fc2::samenc::build_table(p.data(), nullptr, (uint32_t)p.size());
}

struct Rng {
    uint64_t s;
    uint32_t next(uint32_t n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((s >> 33) % n);
    }
};

// generator-shaped text: fragments of one to three lines, unmapped lines, a share of the lines damaged
static std::string make_text(uint64_t seed, int n_frags, int damage_of_100, bool newline) {
    Rng r{seed};
    std::string t;
    for (int k = 0; k < n_frags; ++k) {
        const int lines = 1 + (int)r.next(3);
        for (int j = 0; j < lines; ++j) {
            const bool un = r.next(10) == 0;
            std::string f[11] = {"SRR." + std::to_string(k), std::to_string(un ? 4 : (j ? 129 : 65) | (r.next(2) ? 16 : 0)),
                                 un ? "*" : kNames[r.next(5)], "1000", "60", un ? "*" : "60M40S", "=", "2000", "0",
                                 std::string(20 + r.next(90), 'A'), std::string(20, 'I')};
            if ((int)r.next(100) < damage_of_100) {
                switch (r.next(5)) {
                    case 0: f[5] += "Q"; break;
                    case 1: f[1] = "+" + f[1]; break;
                    case 2: f[1] = "1" + std::string(5, '0'); break;
                    case 3: f[0] = r.next(2) ? std::string() : std::string(255, 'q'); break;
                    default: f[10] += "\r"; break;
                }
            }
            const int fields = (int)r.next(100) < damage_of_100 / 4 ? 10 : 11;
            for (int i = 0; i < fields; ++i) t += (i ? "\t" : "") + f[i];
            if (fields == 11 && r.next(2)) t += "\tNM:i:0\tAS:i:60";
            t += "\n";
        }
        if (r.next(40) == 0) t += "\n";
    }
    if (!newline && !t.empty()) t.pop_back();
    return t;
}

struct Rows {
    uint32_t n = 0;
    std::vector<uint32_t> starts;
    std::vector<fc2_sam_head> heads;
    std::vector<fc2_bam_frag> frags;
};

// the twin into buffers of exactly `cap` rows (the text in one of exactly its bytes)
static bool twin(const std::string &text, uint32_t cap, const std::vector<uint32_t> &table, Rows &R) {
    std::vector<uint8_t> exact(text.begin(), text.end());
    R.starts.assign((size_t)cap + 1, 0xA5A5A5A5u);
    R.heads.assign(cap, fc2_sam_head());
    R.frags.assign(cap, fc2_bam_frag());
    static uint8_t none;
    return fc2_sam_group_host(exact.empty() ? &none : exact.data(), (uint32_t)exact.size(), table.data(), (uint32_t)(table.size() * 4),
                              R.starts.data(), cap ? R.heads.data() : reinterpret_cast<fc2_sam_head *>(&none),
                              cap ? R.frags.data() : reinterpret_cast<fc2_bam_frag *>(&none), &R.n, cap) == FC2_OK;
}

static int check_twin(const std::vector<uint32_t> &table) {
    std::vector<std::string> texts = {"", "\n", "x", "\t\t\t\t\t\t\t\t\t\t\n", "a\t0\tchr1\t1\t1\t*\t*\t0\t0\tA\tI", "\n\n\n"};
    for (int k = 0; k < 12; ++k) texts.push_back(make_text(100 + k, 50 + 40 * k, k % 3 ? 33 : 0, k % 4 != 3));
    size_t closed = 0, unusable = 0;
    for (size_t i = 0; i < texts.size(); ++i) {
        const std::string &t = texts[i];
        uint32_t n = 0;
        for (char c : t) n += c == '\n';
        Rows R;
        if (!twin(t, n, table, R) || R.n != n) return failed("the twin", i, R.n);
        for (uint32_t k = 0; k < n; ++k) {
            if (R.starts[k + 1] <= R.starts[k] || R.starts[k + 1] > t.size() || t[R.starts[k + 1] - 1] != '\n') return failed("starts", i, k);
            unusable += R.heads[k].state == 0;
            const fc2_bam_frag &f = R.frags[k];
            if (!f.state) continue;
            ++closed;
            if (k + f.n_records >= n || R.starts[k + f.n_records] - R.starts[k] != f.bytes || f.n_records > FC2_BAM_FRAG_CAP)
                return failed("a closed row", i, k);
            for (uint32_t j = k; j <= k + f.n_records; ++j)
                if (R.heads[j].state != 1) return failed("an unusable line inside a closed fragment", i, j);
        }
        for (uint32_t cap : {n ? n - 1 : 0u, 0u}) {
            if (cap >= n) continue;
            Rows S;
            if (!twin(t, cap, table, S) || S.n != n) return failed("the twin past cap", i, cap);
            for (uint32_t v : S.starts)
                if (v != 0xA5A5A5A5u) return failed("written past cap", i, cap);
        }
    }
    if (closed < 200 || unusable < 200) return failed("both kinds of rows", closed, unusable);
    return 0;
}

static bool same_rows(const Rows &R, const uint32_t *starts, const fc2_bam_frag *frags, uint32_t n) {
    return n == R.n && !memcmp(starts, R.starts.data(), ((size_t)n + 1) * 4) && (!n || !memcmp(frags, R.frags.data(), (size_t)n * sizeof *frags));
}

static int check_slots(const std::vector<uint32_t> &table) {
    using namespace fc2::samgrp;
    std::string err;
    const uint32_t max_text = 6000, cap = 40;
    if (open(3, 0, 3, max_text, cap, 0, table, err) || open(2, 0, 0, max_text, cap, 0, table, err)) return failed("open takes anything", 0, 0);
    Stage *s = open(2, 0, 3, max_text, cap, 0, table, err);
    if (!s) return failed("open", 0, 0);
    const std::string text = make_text(7, 12, 20, true);
    if (text.size() > max_text) return failed("the text", text.size(), 0);
    Rows R;
    uint32_t n = 0;
    for (char c : text) n += c == '\n';
    if (!twin(text, n, table, R) || n > cap) return failed("the twin", n, cap);
    for (int round = 0; round < 3; ++round) {    // the slots are reused
        int slot[3];
        char *t[3];
        for (int k = 0; k < 3; ++k) {
            slot[k] = acquire(s, t[k]);
            if (slot[k] < 0 || !t[k]) return failed("acquire", round, k);
            memcpy(t[k], text.data(), text.size());
        }
        char *none;
        if (acquire(s, none) != -1) return failed("a fourth slot", round, 0);
        for (int k = 0; k < 3; ++k)
            if (!submit(s, slot[k], (uint32_t)text.size())) return failed("submit", round, k);
        if (submit(s, slot[0], 10)) return failed("submit twice", round, 0);
        for (int k = 2; k >= (round == 2 ? 1 : 0); --k) {         // (the last round gives slot 0 back uncollected)
            const uint32_t *st;
            const fc2_bam_frag *fr;
            uint32_t got;
            if (collect(s, slot[k], st, fr, got, err) != DONE || !same_rows(R, st, fr, got)) return failed("collect", round, k);
            if (collect(s, slot[k], st, fr, got, err) != NONE) return failed("collect twice", round, k);
        }
        for (int k = 0; k < 3; ++k) release(s, slot[k]);
    }
    {                                           // more lines than rows; more text than the slot's
        char *t;
        const int k = acquire(s, t);
        memset(t, '\n', cap + 1);
        const uint32_t *st;
        const fc2_bam_frag *fr;
        uint32_t got;
        if (!submit(s, k, cap + 1) || collect(s, k, st, fr, got, err) != NONE) return failed("lines past cap", 0, 0);
        if (!submit(s, k, cap) || collect(s, k, st, fr, got, err) != DONE || got != cap) return failed("lines at cap", got, 0);
        if (submit(s, k, max_text + 1)) return failed("text past the slot", 0, 0);
        // (the slot stays out, and another one queued: close frees them)
        const int k2 = acquire(s, t);
        memcpy(t, text.data(), text.size());
        if (k2 < 0 || !submit(s, k2, (uint32_t)text.size())) return failed("the last submit", 0, 0);
    }
    close(s);
    return 0;
}

// a splitter and two parse threads: 300 blocks through 3 slots, a block whose slot is not free goes without
static int check_threads(const std::vector<uint32_t> &table) {
    using namespace fc2::samgrp;
    std::string err;
    Stage *s = open(2, 0, 3, 8000, 64, 0, table, err);
    if (!s) return failed("open", 1, 0);
    std::vector<std::string> texts;
    std::vector<Rows> want(8);
    for (int k = 0; k < 8; ++k) {
        texts.push_back(make_text(50 + k, 6 + k, 25, true));
        uint32_t n = 0;
        for (char c : texts[k]) n += c == '\n';
        if (texts[k].size() > 8000 || n > 64 || !twin(texts[k], n, table, want[k])) return failed("the texts", k, n);
    }
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::pair<int, int>> todo;       // (slot, text)
    bool done = false;
    int bad = 0, with_rows = 0, without = 0;
    auto parser = [&]() {
        for (;;) {
            std::pair<int, int> job;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return done || !todo.empty(); });
                if (todo.empty()) return;
                job = todo.front();
                todo.pop_front();
            }
            const uint32_t *st;
            const fc2_bam_frag *fr;
            uint32_t got;
            std::string e;
            const bool ok = collect(s, job.first, st, fr, got, e) == DONE && same_rows(want[job.second], st, fr, got);
            release(s, job.first);
            std::lock_guard<std::mutex> lk(m);
            bad += !ok;
            ++with_rows;
        }
    };
    std::thread p1(parser), p2(parser);
    for (int b = 0; b < 300; ++b) {
        char *t;
        const int k = acquire(s, t);
        if (k < 0) {
            ++without;
            std::this_thread::yield();
            continue;
        }
        const std::string &x = texts[b % 8];
        memcpy(t, x.data(), x.size());
        if (!submit(s, k, (uint32_t)x.size())) ++bad;
        {
            std::lock_guard<std::mutex> lk(m);
            todo.emplace_back(k, b % 8);
        }
        cv.notify_one();
    }
    {
        std::lock_guard<std::mutex> lk(m);
        done = true;
    }
    cv.notify_all();
    p1.join();
    p2.join();
    close(s);
    if (bad || with_rows + without != 300 || with_rows < 3) return failed("the threads", bad, with_rows);
    return 0;
}

int main() {
    const std::vector<uint32_t> table = table_of();
    if (check_twin(table) || check_slots(table) || check_threads(table)) return 1;
    printf("ok\n");
    return 0;
}
