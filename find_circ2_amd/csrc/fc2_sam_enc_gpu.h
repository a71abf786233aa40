// fc2_sam_enc_gpu.h -- the host side of BAM records encoded from SAM text on the GPU (fc2_sam_encode.hip), for
// spliced_alignments.bam's encode stage (fc2_bamout_sam.cpp) and fc2_gpu_sam_encode: a batch of lines goes up
// to the device, sam_size_kernel, sam_scan_kernel and sam_write_kernel turn it into the records'
// bytes (the rule: fc2_sam_encode_impl.h), and the batch's total, its statuses and exactly `total` bytes come
// back.  The slot discipline of the BGZF writer (fc2_bgzf_gpu.h): four slots, each with its own stream, device
// and pinned buffers, made once and reused; no wait on the device is unbounded, and a device that did not answer
// in time is not touched again.  Used from one thread at a time.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace fc2 {
namespace samenc {

struct Gpu;
constexpr int kSlots = 4;                       // batches in flight
constexpr double kDefaultTimeout = 60.0;        // seconds a wait for the device may take

// the table of fc2_sam_names_table for these names (name i has id i; of equal names the last counts)
std::vector<uint32_t> names_table(const std::vector<std::string> &names);

// batches of at most max_lines (1..16384) lines and max_text (1..4 MiB) bytes of text, every wait for the
// device at most timeout_s seconds (<= 0: kDefaultTimeout); the table is copied to the device once.  nullptr
// and err on failure
Gpu *gpu_open(int device, uint32_t max_lines, uint32_t max_text, double timeout_s, const std::vector<uint32_t> &table,
              std::string &err);
// frees everything; a device that timed out is not waited for (its buffers are left to the process's end)
void gpu_close(Gpu *g);
// a wait timed out: the device is not touched again, every later call fails
bool gpu_hung(const Gpu *g);
// the slot's pinned batch: max_text bytes of text and max_lines + 1 offsets, the caller's to fill while the
// slot is idle
char *gpu_text(Gpu *g, int slot);
uint32_t *gpu_off(Gpu *g, int slot);

// the n_lines lines in the idle slot's batch (off[0] = 0, off[n_lines] the text's bytes): the upload, the three
// kernels and the download of the total and the statuses queued on its stream.  False (and err) if
// something failed: the slot stays idle
bool gpu_submit(Gpu *g, int slot, uint32_t n_lines, std::string &err);
enum Wait { DONE = 0, FAILED = 1, TIMED_OUT = 2 };
// waits for the slot's batch (at most timeout_s seconds), then downloads exactly its `total` bytes and waits
// for them in the same way; the slot is idle afterwards.  After DONE: the lines' statuses, and the accepted
// records at bytes, total of them, valid until the slot's next gpu_submit
Wait gpu_collect(Gpu *g, int slot, const uint32_t *&status, const uint8_t *&bytes, size_t &total, std::string &err);

}  // namespace samenc
}  // namespace fc2
