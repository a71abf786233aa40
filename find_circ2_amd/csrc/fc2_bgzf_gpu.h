// fc2_bgzf_gpu.h -- the host side of BGZF output compressed on the GPU (fc2_bgzf_out.hip), for
// spliced_alignments.bam's device mode (fc2_bamout.cpp) and fc2_gpu_bgzf: a piece of up to piece_blocks
// blocks goes up to the device, deflate_kernel (fc2_deflate.hip) turns every block's input into a raw
// DEFLATE stream in a slot of its own, bgzf_frame_kernel packs the slots into the finished block stream,
// and only that stream's `total` bytes come back.  The same slot discipline as the gzip writer's
// (fc2_deflate_gpu.h): four slots, each with its own stream, device and pinned buffers, made once and
// reused; no wait on the device is unbounded, and a device that did not answer in time is not touched
// again.  Used from one thread at a time.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace fc2 {
namespace bgz {

struct Gpu;
constexpr int kSlots = 4;                      // pieces in flight
constexpr uint32_t kDefaultBlock = 0xff00;     // the CPU writer's cut (htslib's BGZF_BLOCK_SIZE)
constexpr uint32_t kDefaultPieceBlocks = 64;
constexpr uint32_t kMaxPieceBlocks = 1024;
constexpr double kDefaultTimeout = 60.0;       // seconds a wait for the device may take

// pieces of at most piece_blocks (1..kMaxPieceBlocks) blocks of `block` (1..0xff00) input bytes, every wait
// for the device at most timeout_s seconds (<= 0: kDefaultTimeout), compressed at `level` (1 or 2:
// fc2_deflate_launch_level); nullptr and err on failure.  tile = 0 or tile >= block: a block is one tile, as
// above.  Otherwise every block is cut into ceil(block / tile) <= 16 tiles, tile k of a block having the
// min(hist, k * tile) bytes of its block before it as history (hist 0..32768, tile + hist <= 65536):
// fc2_deflate_launch_groups fills piece_blocks * ceil(block / tile) slots and fc2_bgzf_frame_groups_launch packs
// each block's streams, its combined CRC-32 and ISIZE into one BGZF block; the rest is the same.  `level` may
// carry level 2's search effort (fc2_deflate_launch_deep's depth 1..128 and nice 4..258) as level_with_search(depth,
// nice) gives it; a plain 1 or 2 is the level's own search.  level_with_search(depth, nice, passes) adds level 2's
// passes (fc2_deflate_launch_priced's 1..3), with that search effort or, depth 0, level 2's own.  (All travel in the
// one argument so that gpu_open keeps the signature its callers and stand-ins are written against.)
Gpu *gpu_open(int device, uint32_t block, uint32_t piece_blocks, double timeout_s, int level, uint32_t tile, uint32_t hist,
              std::string &err);
// level 2 with its search effort for gpu_open's `level`: depth in bits 8..15, nice in bits 16..24 (depth 0: plain 2)
constexpr int level_with_search(uint32_t depth, uint32_t nice) {
    return depth ? (int)(2u | (depth & 0xFFu) << 8 | (nice & 0x1FFu) << 16) : 2;
}
// ... and its passes in bits 25..26 (0 and 1: one pass, the word above)
constexpr int level_with_search(uint32_t depth, uint32_t nice, uint32_t passes) {
    return level_with_search(depth, nice) | (int)((passes > 1u ? passes & 3u : 0u) << 25);
}
// frees everything; a device that timed out is not waited for (its buffers are left to the process's end)
void gpu_close(Gpu *g);
// a wait timed out: the device is not touched again, every later call fails
bool gpu_hung(const Gpu *g);

// n bytes (1..block * piece_blocks) into the idle slot: copied to its pinned buffer, then the upload, both
// kernels and the download of the piece's total queued on its stream.  False (and err) if something failed:
// the slot stays idle
bool gpu_submit(Gpu *g, int slot, const char *data, size_t n, std::string &err);
enum Wait { DONE = 0, FAILED = 1, TIMED_OUT = 2 };
// waits for the slot's piece (at most timeout_s seconds), then downloads exactly its `total` bytes and waits
// for them in the same way; the slot is idle afterwards.  After DONE: the piece's blocks at bytes, total of
// them, valid until the slot's next gpu_submit -- total 0: a tile was given up, the caller compresses the piece
Wait gpu_collect(Gpu *g, int slot, const uint8_t *&bytes, size_t &total, std::string &err);

}  // namespace bgz
}  // namespace fc2
