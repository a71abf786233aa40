// fc2_bamout_sam.cpp -- the -B writer's encode stage (fc2_bamout.h SamStage, fc2_ingest_set_bam_out_encode): SAM
// lines gathered into batches, a batch encoded on the GPU (fc2_sam_enc_gpu.h) or by fc2_sam_encode_host in its
// place, the records given back to the writer strictly in the lines' order; and fc2_sam_encode_line, the
// per-line entry over encode_sam.  Apart from fc2_bamout.cpp so that the writer itself links against nothing
// of the device's.
#include <string.h>

#include <string>
#include <vector>

#include "../../include/fc2_ingest.h"
#include "fc2_bamout.h"
#include "fc2_common.h"
#include "fc2_sam_enc_gpu.h"

namespace fc2 {
namespace bam {

namespace {

// Batch p fills slot p % kSlots -- the slot's pinned text and offsets in mode 1, vectors of its own in mode 2 --
// and batches [head, next) are in flight.  A batch is begun only when its slot's earlier batch is collected,
// so up to three are in flight while the fourth fills.  collect() takes the oldest: all statuses 0, and its
// records go to the writer as they came back; otherwise (a refusal, a device that failed, or a batch from
// off_from on, which never went to the device) its lines are encoded one by one with encode_sam, the first
// failure ending the stage with encode_sam's message.
struct Batcher : SamStage {
    static constexpr int kSlots = samenc::kSlots;
    static constexpr uint64_t kNever = ~0ull;
    Writer *w = nullptr;
    int mode = 0;
    const std::unordered_map<std::string, int> *tid_of = nullptr;
    uint32_t max_lines = 0, max_text = 0;
    samenc::Gpu *gpu = nullptr;
    std::vector<uint32_t> table;
    struct Slot {
        char *text = nullptr;                   // max_text bytes
        uint32_t *off = nullptr;                // max_lines + 1
        uint32_t n = 0;                         // lines
        // mode 2: the slot's memory and what the host rule made of the batch
        std::vector<char> own_text;
        std::vector<uint32_t> own_off, out_off, size, status;
        std::vector<uint8_t> out;
        uint32_t total = 0;
        bool model_ok = false;
    } slot[kSlots];
    uint64_t head = 0, next = 0;
    bool filling = false;                       // batch `next` has lines and is not submitted yet
    uint64_t off_from = kNever;                 // the host encodes every batch from this one on
    uint64_t gpu_batches = 0, host_batches = 0;
    bool dead = false;                          // a line failed, the device timed out or the file did: nothing more is written
    std::string dead_err;

    ~Batcher() override {
        if (gpu) samenc::gpu_close(gpu);        // (a device that timed out is left alone)
    }

    bool die(const std::string &why, std::string &err) {
        dead = true;
        dead_err = why;
        err = why;
        return false;
    }

    // a batch's lines through encode_sam, each record to the writer; the first failing line ends the stage
    bool host_batch(const Slot &s, std::string &err) {
        ++host_batches;
        std::string rec, e;
        for (uint32_t i = 0; i < s.n; ++i) {
            rec.clear();
            if (!encode_sam(s.text + s.off[i], s.text + s.off[i + 1], *tid_of, rec, e)) return die(e, err);
            if (!write_raw(w, (const uint8_t *)rec.data(), rec.size())) return die("", err);
        }
        return true;
    }

    bool submit(std::string &err) {
        filling = false;
        const uint64_t p = next++;
        Slot &s = slot[p % kSlots];
        if (p >= off_from) return true;
        if (mode == 1) {
            std::string e;
            if (!samenc::gpu_submit(gpu, (int)(p % kSlots), s.n, e)) {
                off_from = p;
                if (samenc::gpu_hung(gpu)) return die("IOError: writing spliced_alignments.bam failed: " + e, err);
            }
        } else {
            s.model_ok = fc2_sam_encode_host((const uint8_t *)s.text, s.off[s.n], s.off, s.n, table.data(),
                                             (uint32_t)(table.size() * 4), s.out.data(), s.out.size(), s.out_off.data(),
                                             s.size.data(), s.status.data(), &s.total) == FC2_OK;
        }
        return true;
    }

    bool collect(std::string &err) {
        const uint64_t p = head++;
        Slot &s = slot[p % kSlots];
        const uint32_t *status = nullptr;
        const uint8_t *bytes = nullptr;
        size_t total = 0;
        bool have = false;
        if (p < off_from) {
            if (mode == 1) {
                std::string e;
                const samenc::Wait wt = samenc::gpu_collect(gpu, (int)(p % kSlots), status, bytes, total, e);
                if (wt == samenc::TIMED_OUT) return die("IOError: writing spliced_alignments.bam failed: " + e, err);
                if (wt == samenc::DONE) have = true;
                else off_from = p;              // the device failed: this batch and every later one on the host
            } else if (s.model_ok) {
                status = s.status.data(), bytes = s.out.data(), total = s.total;
                have = true;
            } else {
                off_from = p;
            }
        }
        if (have)
            for (uint32_t i = 0; i < s.n && have; ++i) have = status[i] == FC2_SAM_ENC_OK;
        bool ok;
        if (have) {
            ++gpu_batches;
            ok = !total || write_raw(w, bytes, total) || die("", err);
        } else {
            ok = host_batch(s, err);
        }
        return ok;
    }

    bool add(const char *line, const char *end, std::string &err) override {
        if (dead) {
            err = dead_err;
            return false;
        }
        const size_t len = (size_t)(end - line);
        if (len > max_text) {                   // no batch holds it: everything before it out, then the line itself
            if (!finish(err)) return false;
            ++host_batches;
            std::string rec, e;
            if (!encode_sam(line, end, *tid_of, rec, e)) return die(e, err);
            return write_raw(w, (const uint8_t *)rec.data(), rec.size()) || die("", err);
        }
        if (filling) {
            const Slot &f = slot[next % kSlots];
            if ((f.n == max_lines || len > max_text - f.off[f.n]) && !submit(err)) return false;
        }
        if (!filling) {                         // a batch begins: its slot's earlier batch out first
            while (next - head >= (uint64_t)kSlots)
                if (!collect(err)) return false;
            slot[next % kSlots].n = 0;
            slot[next % kSlots].off[0] = 0;
            filling = true;
        }
        Slot *s = &slot[next % kSlots];
        if (len) memcpy(s->text + s->off[s->n], line, len);
        s->off[s->n + 1] = s->off[s->n] + (uint32_t)len;
        ++s->n;
        return true;
    }

    bool finish(std::string &err) override {
        if (dead) {
            err = dead_err;
            return false;
        }
        if (filling && !submit(err)) return false;
        while (head < next)
            if (!collect(err)) return false;
        return true;
    }

    void counts(uint64_t &g, uint64_t &h) const override { g = gpu_batches, h = host_batches; }
};

}  // namespace

bool set_encode(Writer *w, int mode, int device, const std::vector<std::string> &names,
                const std::unordered_map<std::string, int> *tid_of, uint32_t max_lines, uint32_t max_text, double timeout_s,
                std::string &err) {
    if (!max_lines) max_lines = FC2_SAM_ENC_MAX_LINES;
    if (!max_text) max_text = FC2_SAM_ENC_MAX_TEXT;
    if (!w || !tid_of || mode < 0 || mode > 2 || (mode == 1 && device < 0) || max_lines > FC2_SAM_ENC_MAX_LINES ||
        max_text > FC2_SAM_ENC_MAX_TEXT || timeout_s < 0) {
        err = "mode is 0, 1 or 2, a batch at most 16384 lines and 4 MiB of text";
        return false;
    }
    if (sam_stage_set(w)) {
        err = "call once, before the first record";
        return false;
    }
    if (!mode) return true;
    Batcher *b = new Batcher();
    b->w = w;
    b->mode = mode;
    b->tid_of = tid_of;
    b->max_lines = max_lines;
    b->max_text = max_text;
    b->table = samenc::names_table(names);
    if (b->table.empty()) {
        err = "the reference names do not fit a table";
        delete b;
        return false;
    }
    if (mode == 1) {
        if (!(b->gpu = samenc::gpu_open(device, max_lines, max_text, timeout_s, b->table, err))) {
            delete b;
            return false;
        }
        for (int k = 0; k < Batcher::kSlots; ++k) {
            b->slot[k].text = samenc::gpu_text(b->gpu, k);
            b->slot[k].off = samenc::gpu_off(b->gpu, k);
        }
    } else {
        for (Batcher::Slot &s : b->slot) {
            s.own_text.resize(max_text);
            s.own_off.resize((size_t)max_lines + 1);
            s.out_off.resize((size_t)max_lines + 1);
            s.size.resize(max_lines);
            s.status.resize(max_lines);
            s.out.resize((size_t)FC2_SAM_ENC_BOUND(max_text, max_lines));
            s.text = s.own_text.data();
            s.off = s.own_off.data();
        }
    }
    attach_sam_stage(w, b);
    return true;
}

}  // namespace bam
}  // namespace fc2

extern "C" int fc2_sam_encode_line(const char *line, uint64_t n, const char *const *names, uint32_t n_names, void *out,
                                   uint64_t cap, uint64_t *out_n) {
    if ((!line && n) || (!names && n_names) || (!out && cap) || !out_n)
        return fc2::fail(FC2_E_PARAM, "fc2_sam_encode_line: null argument");
    *out_n = 0;
    std::unordered_map<std::string, int> tid_of;        // (as the ingest fills its own: the last of equal names wins)
    for (uint32_t i = 0; i < n_names; ++i) {
        if (!names[i]) return fc2::fail(FC2_E_PARAM, "fc2_sam_encode_line: null name");
        tid_of[names[i]] = (int)i;
    }
    std::string rec, err;
    if (!fc2::bam::encode_sam(line, line + n, tid_of, rec, err)) return fc2::fail(FC2_E_FORMAT, err);
    *out_n = rec.size();
    if (rec.size() > cap) return fc2::fail(FC2_E_RANGE, "fc2_sam_encode_line: the record does not fit");
    if (!rec.empty()) memcpy(out, rec.data(), rec.size());
    return FC2_OK;
}
