// fc2_sam_group_gpu.h -- the host side of the unspliced fragments of SAM text closed on the GPU
// (fc2_sam_group.hip; the rule: fc2_sam_frag_impl.h), for the ingest's splitter and parse threads: a block of
// text is read straight into a slot's pinned text, goes up to the device, the five kernels of
// fc2_sam_group_launch list its lines and make their rows, and the lines' starts and the fragment rows come back
// into the slot's pinned rows.  A slot holds pinned text, device text, device and pinned rows, a stream and an
// event, all made when the slot is first taken and reused afterwards.  Whoever took a slot keeps it until the
// text is no longer read (the parsed records point into it).  No wait on the device is unbounded; a device that
// failed or did not answer in time is not touched again.  mode 2 is the stand-in without a device: the host
// twin fills the same rows at submit, through the same slots.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/fc2_ingest.h"

namespace fc2 {
namespace samgrp {

struct Stage;
constexpr double kDefaultTimeout = 60.0;        // seconds a wait for the device may take

// mode 1: GPU `device`; 2: the host twin.  n_slots slots of max_text bytes of text (at most
// FC2_SAM_GROUP_MAX_TEXT) and cap lines.  nullptr and err on failure
Stage *open(int mode, int device, int n_slots, uint32_t max_text, uint32_t cap, double timeout_s,
            const std::vector<uint32_t> &table, std::string &err);
// waits (bounded) for what is still queued, then frees everything; a device that timed out is left alone
void close(Stage *s);
uint32_t max_text(const Stage *s);
// a free slot and its text (max_text bytes), or -1: none is free, or the device failed earlier.  Any thread
int acquire(Stage *s, char *&text);
// the slot is free again (any thread); what was queued on it is waited for first, bounded
void release(Stage *s, int slot);
// the slot's first n_bytes of text: upload, launches and download queued on its stream.  False: this block has
// no rows (the caller keeps the slot for the text it holds)
bool submit(Stage *s, int slot, uint32_t n_bytes);
enum Wait { DONE = 0, NONE = 1, TIMED_OUT = 2 };
// after submit returned true, once: waits for the rows (at most timeout_s).  DONE: starts[0 .. n_lines] and
// frags[0 .. n_lines), valid until release.  NONE: the block is the host's (the device failed, or the block has
// more lines than cap).  TIMED_OUT (err): the device is not touched again
Wait collect(Stage *s, int slot, const uint32_t *&starts, const fc2_bam_frag *&frags, uint32_t &n_lines, std::string &err);

}  // namespace samgrp
}  // namespace fc2
