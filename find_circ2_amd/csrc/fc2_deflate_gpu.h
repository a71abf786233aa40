// fc2_deflate_gpu.h -- the host side of the GPU DEFLATE compressor (fc2_deflate.hip) for
// spliced_reads.fastq.gz: pieces of text go up to the device, every tile comes back as a raw DEFLATE
// stream with its CRC-32, and is wrapped here as a gzip member of its own.  Four slots, each with
// its own stream, device and pinned buffers, made once (gpu_open) and reused: the upload, kernel and
// download of the pieces in flight overlap each other and the assembly and write of the pieces
// before.  No wait on the device is unbounded: gpu_wait polls the slot's event against a deadline.
// Used from one thread at a time (fc2_gzpieces.h's submitting side; fc2_gpu_gzip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace fc2 {
namespace dgz {

struct Gpu;
constexpr int kSlots = 4;                      // pieces in flight (128 tiles each: a quarter of the GPU's room)
constexpr uint32_t kDefaultTile = 32768;
constexpr size_t kMemberOverhead = 18;         // a gzip member's header (10) and trailer (8)

constexpr double kDefaultTimeout = 60.0;       // seconds a wait for the device may take

// pieces of at most max_piece bytes in tiles of `tile` bytes (1..65536), every wait for the device
// at most timeout_s seconds (<= 0: kDefaultTimeout), compressed at `level` (1 or 2:
// fc2_deflate_launch_level); nullptr and err on failure.  hist > 0 (at most 32768, tile + hist <= 65536): a piece
// is one launch of fc2_deflate_launch_hist -- every tile but the piece's first has the `hist` bytes before it as
// its window -- and becomes one gzip member (fc2_gzmember_impl.h) instead of one per tile; pieces stay
// independent of each other.  depth, nice (both 0: the level's own search): level 2's search effort,
// fc2_deflate_launch_deep's depth 1..128 and nice 4..258 -- refused unless level is 2.  passes (0: one):
// fc2_deflate_launch_priced's 1..3, with that search effort or level 2's own -- refused unless level is 2
Gpu *gpu_open(int device, size_t max_piece, uint32_t tile, double timeout_s, int level, uint32_t hist, std::string &err,
              uint32_t depth = 0, uint32_t nice = 0, uint32_t passes = 0);
// frees everything; a device that timed out is not waited for (its buffers are left to the process's end)
void gpu_close(Gpu *g);
size_t gpu_max_piece(const Gpu *g);

// n bytes (1..max_piece) into the idle slot: copied to its pinned buffer, then upload, kernel and
// download queued on its stream.  False (and err) if something failed: the slot stays idle
bool gpu_submit(Gpu *g, int slot, const char *data, size_t n, std::string &err);
enum Wait { DONE = 0, FAILED = 1, TIMED_OUT = 2 };
// waits for the slot's piece, at most gpu_open's timeout_s seconds; the slot is idle afterwards
Wait gpu_wait(Gpu *g, int slot, std::string &err);
// after DONE: the bytes of the piece's gzip members -- one per tile, or with a history one in all -- (0: the
// kernel gave a tile up, the CPU must compress the piece), and the members written to dst (that many bytes)
size_t gpu_members_size(const Gpu *g, int slot);
void gpu_members_write(const Gpu *g, int slot, char *dst);

}  // namespace dgz
}  // namespace fc2
