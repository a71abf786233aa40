// fc2_inflate.h -- the BAM input's BGZF blocks inflated on a GPU (fc2_inflate.hip), for the ingest's
// batch reader (fc2_ingest.cpp bgzf_batch): a stream and device buffers for batches of up to
// max_blocks blocks, and a pool of pinned batch buffers the inflated bytes are downloaded into.
// One batch at a time per Gpu (the ingest reads one batch ahead); its chunks on several streams.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/fc2_ingest.h"

namespace fc2 {
namespace inf {

// One BGZF block of a batch as fc2_ingest.cpp's read_blocks read it into `raw` (nothing else decodes a
// header or a trailer): the GPU driver and the CPU threads both inflate from these rows
struct Block {
    size_t at, size;                           // the whole block: raw + at, size bytes
    size_t payload, len;                       // its DEFLATE stream: raw + payload, len bytes
    uint32_t crc, isize;                       // the trailer: CRC-32 and size of the inflated bytes
    uint64_t out;                              // where its bytes lie in the batch: the sum of the ISIZEs before it
};

struct Gpu;

// nullptr (err set) if the device or its buffers cannot be had; pool_cap > 0 opens the pinned pool
// with buffers of that many bytes (the batch buffers: fc2_ingest.cpp's allocator takes them)
Gpu *gpu_open(int device, uint32_t max_blocks, size_t pool_cap, std::string &err);
void gpu_close(Gpu *g);
uint32_t gpu_max_blocks(const Gpu *g);
// A batch of up to max_blocks whole BGZF blocks, inflated into dest back to back (block i at
// blocks[i].out; dest holds max_blocks * 64 KiB): gpu_begin, then gpu_add for each chunk of blocks
// [i0, i1) as they are read (the chunk's bytes are copied, then uploaded, inflated -- CRC-32 and ISIZE
// checked on the device -- and downloaded while the next chunk is read), then gpu_finish, which waits:
// false (err set) if the device failed.  From the first block whose ISIZE exceeds 64 KiB (not BGZF: the
// blocks behind it may lie past what dest holds) that block's chunk and every later chunk of the batch
// are left to the CPU.
// Afterwards gpu_status(g, i) == 0 for each block whose bytes are in dest; the others are the CPU's.
// With walk, the device also lists every inflated block's BAM record starts (bam_walk_kernel: what
// fc2_ingest.cpp's walk_block finds), downloaded with the bytes: after gpu_finish, gpu_walk(g, i, ...)
// for a block with status 0 is its row of `count` ascending offsets into the block and the offset the
// walk leaves the block at (FC2_BAM_WALK_NO_EXIT: nowhere).
// With digest (and walk), the listed records' digest rows (bam_digest_kernel, include/fc2_ingest.h) come
// back too: after gpu_finish, gpu_digest(g, i, count) is block i's `count` rows, one per listed start
// (nullptr: none -- a batch with a block over 64 KiB, or with more rows than the pinned buffer holds).
// With group (which implies walk), the listed records' fragment rows (bam_frag_kernel) come back the same
// way: gpu_frags(g, i, count).  The digest kernel then runs whether or not digest is set -- the fragment
// kernel reads its rows on the device -- but its 32-byte rows are downloaded only with digest.
void gpu_begin(Gpu *g, char *dest, bool walk, bool digest, bool group);
bool gpu_add(Gpu *g, const uint8_t *raw, const Block *blocks, size_t i0, size_t i1);
bool gpu_finish(Gpu *g, std::string &err);
uint32_t gpu_status(const Gpu *g, size_t i);
const uint16_t *gpu_walk(const Gpu *g, size_t i, uint32_t &count, uint32_t &exit);
const fc2_bam_digest *gpu_digest(const Gpu *g, size_t i, uint32_t &count);
const fc2_bam_frag *gpu_frags(const Gpu *g, size_t i, uint32_t &count);

// a pinned buffer of >= n bytes from the pool (nullptr: no pool, too large, or none left)
void *pinned_take(size_t n);
// true if b is one of the pool's buffers
bool pinned_owns(const void *b);
// true if b came from the pool (it goes back to it)
bool pinned_give(void *b);

}  // namespace inf
}  // namespace fc2
