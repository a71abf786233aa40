// fc2_gzpieces.h -- spliced_reads.fastq.gz written by the native read loop: the text is cut into
// pieces, each compressed as its own gzip member on worker threads and written in order.
// Concatenated members are one valid gzip stream (RFC 1952 2.2), so every reader sees the same
// text as from one member (the Python writer, find_circ2_amd/gzout.py, does the same).  Used from
// one thread (the side that records chunks); the workers only compress.
// In device mode (set_device) a piece is compressed on the GPU instead (fc2_deflate.hip through
// fc2_deflate_gpu.h): it goes up when it is submitted, up to four pieces are in flight, and when its turn to
// be written comes its tiles are wrapped as gzip members here -- one per tile, so a piece is several
// members; with a history (set_device's hist > 0: a tile may refer to the bytes of the piece before it) a piece is
// one member, as a piece from the workers is.  The workers stay: they compress whatever the device path hands back (a piece whose
// launch, copy or kernel failed, and every piece from then on) and the empty member of an empty file.
#pragma once
#include <stdio.h>
#include <zlib.h>

#include "fc2_cpuacct.h"
#include "fc2_deflate.h"
#include "fc2_deflate_gpu.h"

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace fc2 {

class GzPieces {
  public:
    ~GzPieces() {
        std::string err;
        close(err);
    }
    bool is_open() const { return f_ != nullptr; }

    bool open(const char *path, int level, int threads, size_t piece, std::string &err) {
        f_ = fopen(path, "wb");
        if (!f_) { err = std::string("IOError: cannot open '") + path + "' for writing"; return false; }
        level_ = level;
        piece_ = piece ? piece : (size_t(4) << 20);
        const int n = threads > 0 ? threads : 1;
        max_pending_ = 2 * (size_t)n;
        stop_ = false;
        for (int k = 0; k < n; ++k) th_.emplace_back([this] { worker(); });
        return true;
    }

    // device mode: pieces are compressed on GPU `device` from now on, in tiles of `tile` bytes, waiting
    // at most timeout_s seconds for the device, at the compressor's `level`, every tile with the `hist` bytes of
    // its piece before it as its window (0: none) (call right after open()); false and err if tile + hist is
    // over 65536 or the device's buffers cannot be made (the file then stays on the CPU); depth, nice: level 2's
    // search effort (dgz::gpu_open; 0, 0: the level's own); passes: level 2's passes (dgz::gpu_open; 0: one)
    bool set_device(int device, uint32_t tile, double timeout_s, int level, uint32_t hist, std::string &err, uint32_t depth = 0,
                    uint32_t nice = 0, uint32_t passes = 0) {
        if (!f_ || gpu_ || wrote_any_) { err = "GPU gzip: set the device once, after open and before any text"; return false; }
        gpu_ = dgz::gpu_open(device, 2 * piece_, tile ? tile : dgz::kDefaultTile, timeout_s, level, hist, err, depth, nice, passes);   // (append_owned: up to two pieces long)
        device_mode_ = gpu_ != nullptr;
        return device_mode_;
    }
    bool device_mode() const { return device_mode_; }
    // pieces the device compressed, and pieces of the device mode the CPU compressed (0, 0 without it)
    void counts(uint64_t *gpu, uint64_t *cpu) const {
        if (gpu) *gpu = n_gpu_;
        if (cpu) *cpu = n_cpu_;
    }

    // takes the bytes of text (text is left empty, its capacity kept for the caller's next chunk);
    // whole pieces go to the workers, each byte is copied once
    void append(std::string &text) {
        size_t at = 0;
        if (!buf_.empty()) {                    // top up the partial piece left by the last call
            at = std::min(piece_ - buf_.size(), text.size());
            buf_.append(text, 0, at);
            if (buf_.size() >= piece_) {
                submit(std::move(buf_));
                buf_.clear();
            }
        }
        while (text.size() - at >= piece_) {
            submit(text.substr(at, piece_));
            at += piece_;
        }
        buf_.append(text, at, std::string::npos);
        text.clear();
    }

    // takes `text` whole as the next member (after what append() left pending) if it is at most two
    // pieces long, leaving `text` empty with a recycled buffer's capacity: a chunk's range texts go
    // out without being copied
    void append_owned(std::string &text) {
        if (text.empty()) return;
        if (text.size() > 2 * piece_) {         // members stay about a piece long
            append(text);
            return;
        }
        if (!buf_.empty()) {
            submit(std::move(buf_));
            buf_.clear();
        }
        std::string fresh;
        {
            std::lock_guard<std::mutex> lk(m_);
            if (!spare_.empty()) {
                fresh.swap(spare_.back());
                spare_.pop_back();
            }
        }
        fresh.swap(text);                       // text: the recycled buffer, emptied
        text.clear();
        submit(std::move(fresh));
    }

    // compresses what is left, writes every member, stops the workers; false on a write error
    bool close(std::string &err) {
        if (!f_) return true;
        if (!buf_.empty() || !wrote_any_) submit(std::move(buf_));   // an empty file still gets one member
        buf_.clear();
        while (!order_.empty()) write_front();
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_work_.notify_all();
        for (std::thread &t : th_) t.join();
        th_.clear();
        dgz::gpu_close(gpu_);
        gpu_ = nullptr;
        const bool ok = (fclose(f_) == 0) & !werr_;
        f_ = nullptr;
        if (!ok) err = werr_msg_.empty() ? "IOError: writing spliced_reads.fastq.gz failed" : werr_msg_;
        return ok;
    }

  private:
    struct Job {
        std::string in, out;
        bool done = false;
        bool zerr = false;
        int slot = -1;                          // device mode: the slot it is in flight in
        uint64_t index = 0;                     // the piece's number in the file
    };
    FILE *f_ = nullptr;
    int level_ = 6;
    size_t piece_ = size_t(4) << 20, max_pending_ = 2;
    std::string buf_;
    std::deque<std::shared_ptr<Job>> order_;   // submission order: written front first
    std::deque<std::shared_ptr<Job>> work_;    // not yet taken by a worker
    std::mutex m_;
    std::condition_variable cv_work_, cv_done_;
    std::vector<std::thread> th_;
    bool stop_ = false, werr_ = false, wrote_any_ = false;
    std::vector<std::string> spare_;           // compressed inputs' buffers, for append_owned
    dgz::Gpu *gpu_ = nullptr;                  // device mode (set_device); gpu_off_: it failed, the CPU goes on
    bool device_mode_ = false, gpu_off_ = false;
    int next_slot_ = 0;
    bool slot_busy_[dgz::kSlots] = {};
    uint64_t n_gpu_ = 0, n_cpu_ = 0, n_pieces_ = 0;
    std::string werr_msg_;

    void submit(std::string &&data) {
        auto j = std::make_shared<Job>();
        j->in = std::move(data);
        j->index = n_pieces_++;
        if (gpu_ && !gpu_off_ && !j->in.empty() && j->in.size() <= dgz::gpu_max_piece(gpu_)) {
            const int s = next_slot_;
            while (slot_busy_[s]) write_front();    // (the piece in it is ahead of this one in order_)
            if (!gpu_off_) {
                cpu::Scope acct(cpu::GZIP);
                std::string err;
                if (dgz::gpu_submit(gpu_, s, j->in.data(), j->in.size(), err)) {
                    j->slot = s;
                    slot_busy_[s] = true;
                    next_slot_ = (s + 1) % dgz::kSlots;
                } else {
                    gpu_off_ = true;
                }
            }
        }
        if (j->slot < 0) to_workers(j);
        order_.push_back(j);
        wrote_any_ = true;
        while (order_.size() > max_pending_) write_front();
    }

    void to_workers(const std::shared_ptr<Job> &j) {
        if (device_mode_) ++n_cpu_;
        {
            std::lock_guard<std::mutex> lk(m_);
            work_.push_back(j);
        }
        cv_work_.notify_one();
    }

    // the front piece's members from its slot (every wait bounded: dgz::gpu_wait); a piece the device
    // did not finish goes to the workers, and so does every later one
    void collect(const std::shared_ptr<Job> &j) {
        std::string err;
        const dgz::Wait w = dgz::gpu_wait(gpu_, j->slot, err);
        bool ok = w == dgz::DONE;
        if (ok) {
            cpu::Scope acct(cpu::GZIP);
            const size_t n = dgz::gpu_members_size(gpu_, j->slot);
            ok = n != 0;
            if (ok) {
                j->out.resize(n);
                dgz::gpu_members_write(gpu_, j->slot, &j->out[0]);
            }
        }
        slot_busy_[j->slot] = false;
        j->slot = -1;
        if (w == dgz::TIMED_OUT && werr_msg_.empty()) {
            werr_ = true;                       // the file is completed by the CPU, and its close reports this
            werr_msg_ = "IOError: spliced_reads.fastq.gz: piece " + std::to_string(j->index) + ": " + err;
        }
        if (!ok) {
            gpu_off_ = true;
            to_workers(j);
            return;
        }
        ++n_gpu_;
        j->in.clear();
        std::lock_guard<std::mutex> lk(m_);
        j->done = true;
        if (spare_.size() < 2 * max_pending_) spare_.push_back(std::move(j->in));
        std::string().swap(j->in);
    }

    void write_front() {
        std::shared_ptr<Job> j = order_.front();
        if (j->slot >= 0) collect(j);
        {
            std::unique_lock<std::mutex> lk(m_);
            cv_done_.wait(lk, [&] { return j->done; });
        }
        order_.pop_front();
        if (j->zerr || (!j->out.empty() && fwrite(j->out.data(), 1, j->out.size(), f_) != j->out.size())) werr_ = true;
    }

    void worker() {
        for (;;) {
            std::shared_ptr<Job> j;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_work_.wait(lk, [&] { return stop_ || !work_.empty(); });
                if (work_.empty()) return;
                j = work_.front();
                work_.pop_front();
            }
            compress(*j);
            {
                std::lock_guard<std::mutex> lk(m_);
                j->done = true;
            }
            cv_done_.notify_all();
        }
    }

    void compress(Job &j) {
        cpu::Scope acct(cpu::GZIP);
        if (!dfl::gzip_member(j.in, level_, j.out)) j.zerr = true;   // libdeflate, or zlib (fc2_deflate.h)
        j.in.clear();
        std::lock_guard<std::mutex> lk(m_);
        if (spare_.size() < 2 * max_pending_) spare_.push_back(std::move(j.in));
        std::string().swap(j.in);
    }
};

}  // namespace fc2
