// fc2_bgzf_out.hip -- BGZF output on the GPU: bgzf_frame_kernel packs the slots deflate_kernel
// (fc2_deflate.hip) filled into the finished block stream (the rule: fc2_bgzf_frame_impl.h), the slots of
// the device writer (fc2_bgzf_gpu.h), and fc2_gpu_bgzf (one buffer through the same path).  With tiles inside a
// block (fc2_deflate_launch_groups) bgzf_groups_scan_kernel and bgzf_groups_kernel do the packing: a block is its
// tiles' streams back to back, its CRC-32 combined from theirs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fc2_caller.h"
#include "fc2_bgzf_frame_impl.h"
#include "fc2_bgzf_gpu.h"
#include "fc2_common.h"

namespace {

using namespace fc2::bgzf;

constexpr uint32_t kFrameThreads = 256;

// the little-endian 32-bit value at byte o of the slot (w: its words, the slot 16-byte aligned), from
// aligned words; the second word is read only when a byte of it is wanted
__device__ __forceinline__ uint32_t slot_u32(const uint32_t *__restrict__ w, uint32_t o) {
    const uint32_t i = o >> 2, s = (o & 3u) * 8u;
    const uint32_t lo = w[i];
    if (!s) return lo;
    return (lo >> s) | (w[i + 1] << (32u - s));
}

// One workgroup per tile.  Every workgroup reads all of out_len itself -- a piece has at most a few hundred
// tiles -- for the piece's validity and its own offset, so none waits for another.  It writes its block's
// header and trailer, then its stream: the slot is 16-byte aligned, the destination is not, so the bytes up
// to the destination's next 16-byte boundary and those after its last one go out one by one and everything
// between as whole uint4 stores.  Every store lies in [out + off, out + off + 26 + out_len) of a valid piece,
// and a valid out_len is at most the tile's bound, which is at most stride: every load lies in the tile's
// slot.  Workgroup 0 also writes total and the n_tiles + 1 offsets (zeros for an invalid piece).
__global__ __launch_bounds__(kFrameThreads) void bgzf_frame_kernel(const uint8_t *__restrict__ slots, uint32_t stride,
                                                                   const uint32_t *__restrict__ out_len,
                                                                   const uint32_t *__restrict__ crc, uint32_t n_tiles,
                                                                   uint64_t n_bytes, uint32_t tile, uint8_t *__restrict__ out,
                                                                   uint32_t *__restrict__ off, uint32_t *__restrict__ total) {
    __shared__ uint32_t sum[kFrameThreads];
    __shared__ uint32_t bad[kFrameThreads];
    const uint32_t blk = blockIdx.x, t = threadIdx.x;
    // thread t's share: tiles [t * per, (t + 1) * per), so workgroup 0 can turn the sums into offsets
    const uint32_t per = (n_tiles + kFrameThreads - 1) / kFrameThreads;
    const uint32_t j0 = min(t * per, n_tiles), j1 = min(j0 + per, n_tiles);
    uint32_t below = 0, all = 0, invalid = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t len = out_len[j];
        if (!tile_ok(len, tile)) {
            invalid = 1;
            continue;
        }
        all += block_bytes(len);
        if (j < blk) below += block_bytes(len);
    }
    sum[t] = below;
    bad[t] = invalid;
    __syncthreads();
    for (uint32_t s = kFrameThreads / 2; s; s >>= 1) {
        if (t < s) {
            sum[t] += sum[t + s];
            bad[t] |= bad[t + s];
        }
        __syncthreads();
    }
    const uint32_t at = sum[0];
    const bool valid = bad[0] == 0;
    __syncthreads();

    if (blk == 0) {                             // the offsets: an exclusive scan of the threads' sums, then each share
        sum[t] = all;
        __syncthreads();
        if (t == 0) {
            uint32_t run = 0;
            for (uint32_t k = 0; k < kFrameThreads; ++k) {
                const uint32_t v = sum[k];
                sum[k] = run;
                run += v;
            }
            off[n_tiles] = valid ? run : 0;
            *total = valid ? run : 0;
        }
        __syncthreads();
        uint32_t run = sum[t];
        for (uint32_t j = j0; j < j1; ++j) {
            off[j] = valid ? run : 0;
            if (valid) run += block_bytes(out_len[j]);
        }
    }
    if (!valid || blk >= n_tiles) return;

    const uint32_t len = out_len[blk], bsize = block_bytes(len);
    uint8_t *const b = out + at;
    if (t < kHead) b[t] = head_byte(t, bsize);
    else if (t >= 32 && t < 32 + kTail)
        b[kHead + len + (t - 32)] = tail_byte(t - 32, crc[blk], isize_of(blk, n_tiles, n_bytes, tile));

    const uint8_t *const s = slots + (uint64_t)blk * stride;
    const uint32_t *const w = reinterpret_cast<const uint32_t *>(s);
    uint8_t *const d = b + kHead;
    const uint32_t lead = min(len, (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u));
    const uint32_t whole = (len - lead) / 16u;                  // uint4 stores at d + lead + 16 * m
    const uint32_t tail0 = lead + whole * 16u;
    if (t < lead) d[t] = s[t];
    if (t >= 64 && t < 64 + (len - tail0)) d[tail0 + (t - 64)] = s[tail0 + (t - 64)];      // (fewer than 16)
    for (uint32_t m = t; m < whole; m += kFrameThreads) {
        const uint32_t o = lead + m * 16u;
        uint4 v;
        v.x = slot_u32(w, o);
        v.y = slot_u32(w, o + 4);
        v.z = slot_u32(w, o + 8);
        v.w = slot_u32(w, o + 12);
        *reinterpret_cast<uint4 *>(d + o) = v;
    }
}

int check_frame_args(const char *who, const void *slots, uint32_t stride, const void *out_len, const void *crc,
                     uint32_t n_tiles, uint64_t n_bytes, uint32_t tile, const void *out, const void *off, const void *total) {
    const std::string w(who);
    if (!slots || !out_len || !crc || !out || !off || !total) return fc2::fail(FC2_E_PARAM, w + ": null argument");
    if (!piece_ok(n_tiles, n_bytes, tile))
        return fc2::fail(FC2_E_PARAM, w + ": tile must be 1..0xff00, n_tiles 1..65535, and n_bytes end in the last tile");
    if (stride < FC2_DEFLATE_TILE_BOUND(tile)) return fc2::fail(FC2_E_PARAM, w + ": stride below FC2_DEFLATE_TILE_BOUND(tile)");
    return FC2_OK;
}

}  // namespace

extern "C" int fc2_bgzf_frame_launch(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                                     uint32_t n_tiles, uint64_t n_bytes, uint32_t tile, uint8_t *out, uint32_t *off,
                                     uint32_t *total, void *stream) {
    if (int rc = check_frame_args("fc2_bgzf_frame_launch", slots, stride, out_len, crc, n_tiles, n_bytes, tile, out, off, total))
        return rc;
    if (((uintptr_t)slots & 15u) || (stride & 15u))
        return fc2::fail(FC2_E_PARAM, "fc2_bgzf_frame_launch: the slots must lie on 16-byte boundaries");
    hipLaunchKernelGGL(bgzf_frame_kernel, dim3(n_tiles), dim3(kFrameThreads), 0, (hipStream_t)stream, slots, stride, out_len,
                       crc, n_tiles, n_bytes, tile, out, off, total);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_bgzf_frame_launch: ") + hipGetErrorString(e));
}

extern "C" int fc2_bgzf_frame_host(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                                   uint32_t n_tiles, uint64_t n_bytes, uint32_t tile, uint8_t *out, uint32_t *off,
                                   uint32_t *total) {
    if (total) *total = 0;
    if (int rc = check_frame_args("fc2_bgzf_frame_host", slots, stride, out_len, crc, n_tiles, n_bytes, tile, out, off, total))
        return rc;
    frame_piece(slots, stride, out_len, crc, n_tiles, n_bytes, tile, out, off, total);
    return FC2_OK;
}

// ---- groups: a block of several tiles ----------------------------------------------------------------

namespace {

// A piece of 1024 blocks of 16 tiles has 16384 out_len entries: if every workgroup summed all of them for its
// offset, as bgzf_frame_kernel does with its 64, a piece would read 16 M entries where 16 K are needed.  So the
// offsets come from one workgroup that runs first, on the same stream: thread t sums the blocks of its share of
// the groups (each group's tiles checked with tile_ok, each block against 65536), the shares' sums are scanned,
// and off[0 .. n_groups] and total are written -- zeros if anything was invalid.  bgzf_groups_kernel then reads
// only off[g], total (0: the piece stays unwritten) and its own group's entries; no workgroup waits for another.
__global__ __launch_bounds__(kFrameThreads) void bgzf_groups_scan_kernel(const uint32_t *__restrict__ out_len,
                                                                         uint32_t n_groups, uint64_t n_bytes,
                                                                         uint32_t group, uint32_t tile,
                                                                         uint32_t *__restrict__ off,
                                                                         uint32_t *__restrict__ total) {
    __shared__ uint32_t sum[kFrameThreads];
    __shared__ uint32_t bad[kFrameThreads];
    const uint32_t t = threadIdx.x, tpg = tiles_per_group(group, tile);
    const uint32_t per = (n_groups + kFrameThreads - 1) / kFrameThreads;
    const uint32_t g0 = min(t * per, n_groups), g1 = min(g0 + per, n_groups);
    uint32_t all = 0, invalid = 0;
    for (uint32_t g = g0; g < g1; ++g) {
        const uint32_t cnt = group_tile_count(group_bytes(g, n_groups, n_bytes, group), tile);
        uint32_t b = kOverhead;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t len = out_len[g * tpg + k];
            if (tile_ok(len, tile)) b += len;   // (at most 16 * 65552: no overflow)
            else invalid = 1;
        }
        if (b > kBlockMax) invalid = 1;
        all += b;
    }
    sum[t] = all;
    bad[t] = invalid;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0, any = 0;
        for (uint32_t k = 0; k < kFrameThreads; ++k) {
            const uint32_t v = sum[k];
            sum[k] = run;
            run += v;
            any |= bad[k];
        }
        bad[0] = any;
        off[n_groups] = any ? 0 : run;
        *total = any ? 0 : run;
    }
    __syncthreads();
    const bool valid = bad[0] == 0;
    uint32_t run = sum[t];
    for (uint32_t g = g0; g < g1; ++g) {
        off[g] = valid ? run : 0;
        if (!valid) continue;
        const uint32_t cnt = group_tile_count(group_bytes(g, n_groups, n_bytes, group), tile);
        run += kOverhead;
        for (uint32_t k = 0; k < cnt; ++k) run += out_len[g * tpg + k];
    }
}

// One workgroup per block, after bgzf_groups_scan_kernel.  The group's (at most 16) stream lengths and their
// running sum are put into LDS; thread k < cnt also brings tile k's CRC to the group's end (crc_shift by the
// input bytes behind the tile), and the XOR of those is the group's CRC -- crc_append unrolled, no input read.
// Each tile's stream is copied as in bgzf_frame_kernel: its slot is 16-byte aligned, its destination -- where
// the previous tile's stream ended -- is not, so the lead up to the destination's next 16-byte boundary and the
// tail behind its last one go byte by byte and the rest as whole uint4 stores.  Every store lies in
// [out + off[g], out + off[g + 1]) of a valid piece; every load in a slot, a valid out_len being at most stride.
__global__ __launch_bounds__(kFrameThreads) void bgzf_groups_kernel(const uint8_t *__restrict__ slots, uint32_t stride,
                                                                    const uint32_t *__restrict__ out_len,
                                                                    const uint32_t *__restrict__ crc, uint32_t n_groups,
                                                                    uint64_t n_bytes, uint32_t group, uint32_t tile,
                                                                    uint8_t *__restrict__ out,
                                                                    const uint32_t *__restrict__ off,
                                                                    const uint32_t *__restrict__ total) {
    __shared__ uint32_t lens[kTilesPerGroupMax], at[kTilesPerGroupMax + 1], part[kTilesPerGroupMax];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    if (g >= n_groups || *total == 0) return;   // (uniform)
    const uint32_t tpg = tiles_per_group(group, tile), first = g * tpg;
    const uint32_t gbytes = group_bytes(g, n_groups, n_bytes, group), cnt = group_tile_count(gbytes, tile);
    if (t < cnt) {
        lens[t] = out_len[first + t];
        const uint32_t behind = gbytes - (t * tile + group_tile_bytes(t, gbytes, tile));
        part[t] = crc_shift(crc[first + t], behind);
    }
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < cnt; ++k) {
            at[k] = run;
            run += lens[k];
        }
        at[cnt] = run;
    }
    __syncthreads();
    const uint32_t len = at[cnt], bsize = block_bytes(len);
    uint8_t *const b = out + off[g];
    if (t < kHead) b[t] = head_byte(t, bsize);
    else if (t >= 32 && t < 32 + kTail) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < cnt; ++k) c ^= part[k];
        b[kHead + len + (t - 32)] = tail_byte(t - 32, c, gbytes);
    }
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t n = lens[k];
        const uint8_t *const s = slots + (uint64_t)(first + k) * stride;
        const uint32_t *const w = reinterpret_cast<const uint32_t *>(s);
        uint8_t *const d = b + kHead + at[k];
        const uint32_t lead = min(n, (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u));
        const uint32_t whole = (n - lead) / 16u;                // uint4 stores at d + lead + 16 * m
        const uint32_t tail0 = lead + whole * 16u;
        if (t < lead) d[t] = s[t];
        if (t >= 64 && t < 64 + (n - tail0)) d[tail0 + (t - 64)] = s[tail0 + (t - 64)];    // (fewer than 16)
        for (uint32_t m = t; m < whole; m += kFrameThreads) {
            const uint32_t o = lead + m * 16u;
            uint4 v;
            v.x = slot_u32(w, o);
            v.y = slot_u32(w, o + 4);
            v.z = slot_u32(w, o + 8);
            v.w = slot_u32(w, o + 12);
            *reinterpret_cast<uint4 *>(d + o) = v;
        }
    }
}

int check_groups_args(const char *who, const void *slots, uint32_t stride, const void *out_len, const void *crc,
                      uint32_t n_tiles, uint64_t n_bytes, uint32_t group, uint32_t tile, const void *out, const void *off,
                      const void *total) {
    const std::string w(who);
    if (!slots || !out_len || !crc || !out || !off || !total) return fc2::fail(FC2_E_PARAM, w + ": null argument");
    if (!groups_ok(n_tiles, n_bytes, group, tile))
        return fc2::fail(FC2_E_PARAM, w + ": group must be 1..0xff00, tile 1..65536 with at most 16 tiles a group, at most "
                                          "65535 groups, and n_tiles the tiles of n_bytes");
    if (stride < FC2_DEFLATE_TILE_BOUND(tile)) return fc2::fail(FC2_E_PARAM, w + ": stride below FC2_DEFLATE_TILE_BOUND(tile)");
    return FC2_OK;
}

}  // namespace

extern "C" int fc2_bgzf_frame_groups_launch(const uint8_t *slots, uint32_t stride, const uint32_t *out_len,
                                            const uint32_t *crc, uint32_t n_tiles, uint64_t n_bytes, uint32_t group,
                                            uint32_t tile, uint8_t *out, uint32_t *off, uint32_t *total, void *stream) {
    if (int rc = check_groups_args("fc2_bgzf_frame_groups_launch", slots, stride, out_len, crc, n_tiles, n_bytes, group, tile,
                                   out, off, total))
        return rc;
    if (((uintptr_t)slots & 15u) || (stride & 15u))
        return fc2::fail(FC2_E_PARAM, "fc2_bgzf_frame_groups_launch: the slots must lie on 16-byte boundaries");
    const uint32_t n_groups = groups_of(n_bytes, group);
    hipLaunchKernelGGL(bgzf_groups_scan_kernel, dim3(1), dim3(kFrameThreads), 0, (hipStream_t)stream, out_len, n_groups, n_bytes,
                       group, tile, off, total);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bgzf_groups_kernel, dim3(n_groups), dim3(kFrameThreads), 0, (hipStream_t)stream, slots, stride,
                           out_len, crc, n_groups, n_bytes, group, tile, out, off, total);
        e = hipGetLastError();
    }
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_bgzf_frame_groups_launch: ") + hipGetErrorString(e));
}

extern "C" int fc2_bgzf_frame_groups_host(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                                          uint32_t n_tiles, uint64_t n_bytes, uint32_t group, uint32_t tile, uint8_t *out,
                                          uint32_t *off, uint32_t *total) {
    if (total) *total = 0;
    if (int rc = check_groups_args("fc2_bgzf_frame_groups_host", slots, stride, out_len, crc, n_tiles, n_bytes, group, tile, out,
                                   off, total))
        return rc;
    frame_groups(slots, stride, out_len, crc, n_tiles, n_bytes, group, tile, out, off, total);
    return FC2_OK;
}

// ---- the device writer's slots ---------------------------------------------------------------------

namespace fc2 {
namespace bgz {

struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    uint8_t *h_src = nullptr, *h_out = nullptr, *d_src = nullptr, *d_slots = nullptr, *d_out = nullptr;
    uint32_t *h_total = nullptr, *d_meta = nullptr;      // d_meta: out_len | crc | off (max_tiles + 1) | total
    void *d_scratch = nullptr;
    size_t n = 0;                              // the piece's bytes
    uint32_t tiles = 0;
    bool busy = false;
};

struct Gpu {
    int device = 0;
    uint32_t block = kDefaultBlock, stride = 0, max_tiles = 0;
    size_t max_piece = 0, out_cap = 0;
    double timeout_s = kDefaultTimeout;
    int level = 1;                             // fc2_deflate_launch_level's
    uint32_t tile = 0, hist = 0, tpg = 1;      // tile > 0: blocks of tpg tiles (fc2_deflate_launch_groups); 0: a block is a tile
    uint32_t depth = 0, nice = 0;              // depth > 0: fc2_deflate_launch_deep with these (level 2 only)
    uint32_t passes = 0;                       // > 1: fc2_deflate_launch_priced with these (level 2 only)
    bool hung = false;                         // a wait timed out: the device is not touched again
    Slot slot[kSlots];
};

static bool hip_ok(hipError_t e, const char *what, std::string &err) {
    if (e == hipSuccess) return true;
    err = std::string("GPU BGZF: ") + what + ": " + hipGetErrorString(e);
    return false;
}

// the slot's event against the deadline: DONE, FAILED (err), or TIMED_OUT (err; g->hung set)
static Wait wait_event(Gpu *g, Slot &s, std::string &err) {
    const auto t0 = std::chrono::steady_clock::now();
    const double limit = g->timeout_s;
    int spins = 0;
    for (;;) {
        const hipError_t e = hipEventQuery(s.done);
        if (e == hipSuccess) return DONE;
        if (e != hipErrorNotReady) {
            hip_ok(e, "kernel", err);
            return FAILED;
        }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) {
            g->hung = true;
            err = "GPU BGZF: the device did not answer within " + std::to_string((int)limit) + " s";
            return TIMED_OUT;
        }
        // a piece takes a millisecond or two of kernel time and its copies: look again soon, then sleep longer
        if (++spins < 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
        else std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

Gpu *gpu_open(int device, uint32_t block, uint32_t piece_blocks, double timeout_s, int level, uint32_t tile, uint32_t hist,
              std::string &err) {
    // (level_with_search: level 2's search effort and passes ride in the level's upper bits)
    const uint32_t depth = ((uint32_t)level >> 8) & 0xFFu, nice = ((uint32_t)level >> 16) & 0x1FFu;
    const uint32_t passes = ((uint32_t)level >> 25) & 3u;
    if (level > 0 && (depth || nice || passes)) level &= 0xFF;
    if (!block || block > bgzf::kTileMax || !piece_blocks || piece_blocks > kMaxPieceBlocks || device < 0 || level < 1 ||
        level > 2) {
        err = "GPU BGZF: bad block size, piece size, device or level";
        return nullptr;
    }
    if ((depth || nice) && (level != 2 || depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX ||
                            nice < FC2_DEFLATE_NICE_MIN || nice > FC2_DEFLATE_NICE_MAX)) {
        err = "GPU BGZF: the search effort needs level 2, depth 1..128 and nice 4..258";
        return nullptr;
    }
    if (passes && level != 2) {
        err = "GPU BGZF: passes need level 2";
        return nullptr;
    }
    if (tile >= block) tile = 0;                // (a block is one tile: today's launches, and no history to have)
    if (tile && (hist > 32768u || tile + hist > 65536u || bgzf::tiles_per_group(block, tile) > bgzf::kTilesPerGroupMax)) {
        err = "GPU BGZF: at most 16 tiles a block, a history of at most 32768 bytes, tile and history at most 65536 together";
        return nullptr;
    }
    Gpu *g = new Gpu();
    g->device = device;
    g->block = block;
    g->tile = tile;
    g->hist = tile ? hist : 0;
    g->tpg = tile ? bgzf::tiles_per_group(block, tile) : 1;
    g->stride = (FC2_DEFLATE_TILE_BOUND(tile ? tile : block) + 15u) & ~15u;  // slots on 16-byte boundaries
    g->max_tiles = piece_blocks * g->tpg;
    g->max_piece = (size_t)block * piece_blocks;
    g->out_cap = tile ? (size_t)piece_blocks * bgzf::kBlockMax      // (a block of tiles is framed only if it fits)
                      : (size_t)piece_blocks * (bgzf::kOverhead + FC2_DEFLATE_TILE_BOUND(block));
    g->timeout_s = timeout_s > 0 ? timeout_s : kDefaultTimeout;
    g->level = level;
    g->depth = depth;
    g->passes = passes;
    g->nice = nice;
    const size_t slots = (size_t)g->max_tiles * g->stride, meta = ((size_t)g->max_tiles * 3 + 2) * sizeof(uint32_t),
                 scratch = (size_t)fc2_deflate_scratch_bytes(g->max_piece, tile ? tile : block);
    bool ok = hip_ok(hipSetDevice(device), "hipSetDevice", err);
    for (int k = 0; k < kSlots && ok; ++k) {
        Slot &s = g->slot[k];
        ok = hip_ok(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), "stream", err) &&
             hip_ok(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "event", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_src, g->max_piece, hipHostMallocDefault), "pinned input", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_out, g->out_cap, hipHostMallocDefault), "pinned output", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_total, sizeof(uint32_t), hipHostMallocDefault), "pinned total", err) &&
             hip_ok(hipMalloc((void **)&s.d_src, g->max_piece), "device input", err) &&
             hip_ok(hipMalloc((void **)&s.d_slots, slots), "device slots", err) &&
             hip_ok(hipMalloc((void **)&s.d_out, g->out_cap), "device output", err) &&
             hip_ok(hipMalloc((void **)&s.d_meta, meta), "device table", err) &&
             hip_ok(hipMalloc(&s.d_scratch, scratch), "device scratch", err);
    }
    if (!ok) {
        gpu_close(g);
        return nullptr;
    }
    return g;
}

void gpu_close(Gpu *g) {
    if (!g) return;
    if (!g->hung && hipSetDevice(g->device) == hipSuccess) {
        for (Slot &s : g->slot) {
            if (s.busy) {                       // (a piece nobody collected: bounded like every wait here)
                std::string err;
                if (wait_event(g, s, err) == TIMED_OUT) break;
                s.busy = false;
            }
        }
        if (!g->hung) {
            for (Slot &s : g->slot) {
                if (s.d_scratch) (void)hipFree(s.d_scratch);
                if (s.d_meta) (void)hipFree(s.d_meta);
                if (s.d_out) (void)hipFree(s.d_out);
                if (s.d_slots) (void)hipFree(s.d_slots);
                if (s.d_src) (void)hipFree(s.d_src);
                if (s.h_total) (void)hipHostFree(s.h_total);
                if (s.h_out) (void)hipHostFree(s.h_out);
                if (s.h_src) (void)hipHostFree(s.h_src);
                if (s.done) (void)hipEventDestroy(s.done);
                if (s.stream) (void)hipStreamDestroy(s.stream);
            }
        }
    }
    delete g;
}

bool gpu_hung(const Gpu *g) { return g->hung; }

bool gpu_submit(Gpu *g, int k, const char *data, size_t n, std::string &err) {
    if (g->hung || k < 0 || k >= kSlots || g->slot[k].busy || !n || n > g->max_piece) {
        err = "GPU BGZF: no slot for the piece";
        return false;
    }
    Slot &s = g->slot[k];
    if (!hip_ok(hipSetDevice(g->device), "hipSetDevice", err)) return false;
    memcpy(s.h_src, data, n);
    s.n = n;
    s.tiles = g->tile ? (uint32_t)fc2_deflate_group_tiles(n, g->block, g->tile) : (uint32_t)((n + g->block - 1) / g->block);
    *s.h_total = 0;
    uint32_t *const d_len = s.d_meta, *const d_crc = s.d_meta + g->max_tiles, *const d_off = s.d_meta + 2 * (size_t)g->max_tiles,
                    *const d_total = d_off + g->max_tiles + 1;
    // (whatever was queued on the stream before a failure still runs: from the first call on the slot
    // counts as busy, and a failure drains the stream before the slot's buffers can be used again)
    s.busy = true;
    auto compress = [&] {
        if (g->passes > 1)                      // (level 2's own search where none is set)
            return fc2_deflate_launch_priced(s.d_src, n, g->tile ? g->block : 0, g->tile ? g->tile : g->block, g->hist, s.d_slots,
                                             g->stride, d_len, d_crc, s.d_scratch, s.stream,
                                             g->depth ? g->depth : FC2_DEFLATE_LEVEL2_DEPTH,
                                             g->depth ? g->nice : FC2_DEFLATE_LEVEL2_NICE, g->passes);
        if (g->depth)                           // (group = block: one tile a block is fc2_deflate_launch_level's shape)
            return fc2_deflate_launch_deep(s.d_src, n, g->tile ? g->block : 0, g->tile ? g->tile : g->block, g->hist, s.d_slots,
                                           g->stride, d_len, d_crc, s.d_scratch, s.stream, g->depth, g->nice);
        return g->tile ? fc2_deflate_launch_groups(s.d_src, n, g->block, g->tile, g->hist, s.d_slots, g->stride, d_len, d_crc,
                                                   s.d_scratch, s.stream, g->level)
                       : fc2_deflate_launch_level(s.d_src, n, g->block, s.d_slots, g->stride, d_len, d_crc, s.d_scratch, s.stream,
                                                  g->level);
    };
    auto frame = [&] {
        return g->tile ? fc2_bgzf_frame_groups_launch(s.d_slots, g->stride, d_len, d_crc, s.tiles, n, g->block, g->tile, s.d_out,
                                                      d_off, d_total, s.stream)
                       : fc2_bgzf_frame_launch(s.d_slots, g->stride, d_len, d_crc, s.tiles, n, g->block, s.d_out, d_off, d_total,
                                               s.stream);
    };
    const bool ok =
        hip_ok(hipMemcpyAsync(s.d_src, s.h_src, n, hipMemcpyHostToDevice, s.stream), "upload", err) &&
        (compress() == FC2_OK || ((err = "GPU BGZF: the compressor's launch failed"), false)) &&
        (frame() == FC2_OK || ((err = "GPU BGZF: the framing launch failed"), false)) &&
        hip_ok(hipMemcpyAsync(s.h_total, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream), "download", err) &&
        hip_ok(hipEventRecord(s.done, s.stream), "event", err);
    if (!ok) {
        std::string ignored;
        (void)hipEventRecord(s.done, s.stream);
        if (wait_event(g, s, ignored) == TIMED_OUT) err = ignored;
        s.busy = false;
        return false;
    }
    return true;
}

Wait gpu_collect(Gpu *g, int k, const uint8_t *&bytes, size_t &total, std::string &err) {
    bytes = nullptr;
    total = 0;
    if (g->hung) {
        err = "GPU BGZF: the device timed out earlier";
        return FAILED;
    }
    if (k < 0 || k >= kSlots || !g->slot[k].busy) {
        err = "GPU BGZF: nothing to wait for";
        return FAILED;
    }
    Slot &s = g->slot[k];
    if (!hip_ok(hipSetDevice(g->device), "hipSetDevice", err)) {
        s.busy = false;
        return FAILED;
    }
    Wait w = wait_event(g, s, err);
    if (w == TIMED_OUT) return w;               // (the slot stays busy: the device is not touched again)
    if (w == DONE) {
        const size_t t = *s.h_total;
        if (t > g->out_cap) {                   // (not what the kernel can write: the rule bounds it)
            err = "GPU BGZF: a piece's size is out of range";
            w = FAILED;
        } else if (t) {
            // now that the piece's size is known: exactly that many bytes, on the same stream
            if (!hip_ok(hipMemcpyAsync(s.h_out, s.d_out, t, hipMemcpyDeviceToHost, s.stream), "download", err) ||
                !hip_ok(hipEventRecord(s.done, s.stream), "event", err)) {
                (void)hipEventRecord(s.done, s.stream);
                std::string ignored;
                if (wait_event(g, s, ignored) == TIMED_OUT) {
                    err = ignored;
                    return TIMED_OUT;
                }
                w = FAILED;
            } else {
                w = wait_event(g, s, err);
                if (w == TIMED_OUT) return w;
                if (w == DONE) {
                    bytes = s.h_out;
                    total = t;
                }
            }
        }
    }
    s.busy = false;
    return w;
}

}  // namespace bgz
}  // namespace fc2

// ---- one buffer through the device writer's path ---------------------------------------------------

namespace {

// n (<= block * piece_blocks) bytes as BGZF blocks of `block` input bytes from zlib, appended to out: what a
// piece becomes when the device hands it back
bool cpu_piece(const char *p, size_t n, uint32_t block, std::vector<uint8_t> &out) {
    z_stream zs{};
    if (deflateInit2(&zs, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    bool ok = true;
    for (size_t at = 0; at < n && ok; at += block) {
        const size_t k = std::min<size_t>(block, n - at), base = out.size();
        out.resize(base + kBlockMax);
        deflateReset(&zs);
        zs.next_in = (Bytef *)(p + at);
        zs.avail_in = (uInt)k;
        zs.next_out = out.data() + base + kHead;
        zs.avail_out = kBlockMax - kOverhead;
        ok = deflate(&zs, Z_FINISH) == Z_STREAM_END;
        const uint32_t len = kBlockMax - kOverhead - zs.avail_out;
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)(p + at), (uInt)k);
        for (uint32_t b = 0; b < kHead; ++b) out[base + b] = head_byte(b, block_bytes(len));
        for (uint32_t b = 0; b < kTail; ++b) out[base + kHead + len + b] = tail_byte(b, crc, (uint32_t)k);
        out.resize(base + block_bytes(len));
    }
    deflateEnd(&zs);
    return ok;
}

}  // namespace

extern "C" uint64_t fc2_gpu_bgzf_bound(uint64_t n, uint32_t block) {
    if (!block || block > kTileMax) return 0;
    const uint64_t blocks = (n + block - 1) / block;
    return n + blocks * (kOverhead + 16);       // a block per `block` bytes: the stream at its worst and the 26 bytes around it
}

extern "C" uint64_t fc2_gpu_bgzf_tiles_bound(uint64_t n, uint32_t block, uint32_t tile) {
    if (!block || block > kTileMax) return 0;
    if (!tile || tile >= block) return fc2_gpu_bgzf_bound(n, block);
    const uint64_t blocks = (n + block - 1) / block;
    return n + blocks * (kOverhead + 16ull * tiles_per_group(block, tile));     // every tile's stream at its worst
}

extern "C" int fc2_gpu_bgzf(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, void *out,
                            uint64_t cap, uint64_t *out_n) {
    return fc2_gpu_bgzf_level(device, in, n, block, piece_blocks, 1, out, cap, out_n);
}

extern "C" int fc2_gpu_bgzf_level(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, int level,
                                  void *out, uint64_t cap, uint64_t *out_n) {
    return fc2_gpu_bgzf_tiles(device, in, n, block, piece_blocks, 0, 0, level, out, cap, out_n);
}

namespace {
int gpu_bgzf(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, uint32_t tile, uint32_t hist, int level,
             uint32_t depth, uint32_t nice, void *out, uint64_t cap, uint64_t *out_n, uint32_t passes = 0);
}  // namespace

extern "C" int fc2_gpu_bgzf_tiles(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, uint32_t tile,
                                  uint32_t hist, int level, void *out, uint64_t cap, uint64_t *out_n) {
    return gpu_bgzf(device, in, n, block, piece_blocks, tile, hist, level, 0, 0, out, cap, out_n);
}

extern "C" int fc2_gpu_bgzf_deep(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, uint32_t tile,
                                 uint32_t hist, uint32_t depth, uint32_t nice, void *out, uint64_t cap, uint64_t *out_n) {
    if (depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX || nice < FC2_DEFLATE_NICE_MIN ||
        nice > FC2_DEFLATE_NICE_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_bgzf_deep: depth is 1..128, nice 4..258");
    return gpu_bgzf(device, in, n, block, piece_blocks, tile, hist, 2, depth, nice, out, cap, out_n);
}

extern "C" int fc2_gpu_bgzf_priced(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, uint32_t tile,
                                   uint32_t hist, uint32_t depth, uint32_t nice, uint32_t passes, void *out, uint64_t cap,
                                   uint64_t *out_n) {
    if (passes < FC2_DEFLATE_PASSES_MIN || passes > FC2_DEFLATE_PASSES_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_bgzf_priced: passes is 1..3");
    if (depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX || nice < FC2_DEFLATE_NICE_MIN ||
        nice > FC2_DEFLATE_NICE_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_bgzf_priced: depth is 1..128, nice 4..258");
    return gpu_bgzf(device, in, n, block, piece_blocks, tile, hist, 2, depth, nice, out, cap, out_n, passes);
}

namespace {
int gpu_bgzf(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, uint32_t tile, uint32_t hist, int level,
             uint32_t depth, uint32_t nice, void *out, uint64_t cap, uint64_t *out_n, uint32_t passes) {
    using namespace fc2;
    if (!block || block > kTileMax || piece_blocks > bgz::kMaxPieceBlocks || device < 0 || !out || !out_n || (!in && n) ||
        level < 1 || level > 2)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_bgzf: bad arguments (block is 1..0xff00, piece_blocks at most 1024)");
    if (tile && tile < block && (hist > 32768u || tile + hist > 65536u || tiles_per_group(block, tile) > kTilesPerGroupMax))
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_bgzf_tiles: at most 16 tiles a block, hist 0..32768, tile + hist <= 65536");
    *out_n = 0;
    if (!n) return FC2_OK;
    if (!piece_blocks) piece_blocks = bgz::kDefaultPieceBlocks;
    std::string err;
    bgz::Gpu *g = bgz::gpu_open(device, block, piece_blocks, 0, depth ? bgz::level_with_search(depth, nice, passes) : level, tile, hist, err);
    if (!g) return fc2::fail(FC2_E_HIP, "fc2_gpu_bgzf: " + err);
    const char *src = static_cast<const char *>(in);
    uint8_t *o = static_cast<uint8_t *>(out);
    const uint64_t piece = (uint64_t)block * piece_blocks, pieces = (n + piece - 1) / piece;
    uint64_t at = 0;
    int rc = FC2_OK;
    // piece p goes into slot p % kSlots; before a slot is reused, its piece (p - kSlots) is collected: up to
    // four pieces in flight, written in order
    auto collect = [&](uint64_t p) {
        const uint8_t *bytes = nullptr;
        size_t total = 0;
        const bgz::Wait w = bgz::gpu_collect(g, (int)(p % bgz::kSlots), bytes, total, err);
        if (w != bgz::DONE)
            return fc2::fail(w == bgz::TIMED_OUT ? FC2_E_IO : FC2_E_HIP, "fc2_gpu_bgzf: piece " + std::to_string(p) + ": " + err);
        std::vector<uint8_t> cpu;
        if (!total) {                           // a tile given up: this piece from the CPU
            const uint64_t b0 = p * piece;
            if (!cpu_piece(src + b0, (size_t)std::min<uint64_t>(piece, n - b0), block, cpu))
                return fc2::fail(FC2_E_IO, "fc2_gpu_bgzf: cannot compress");
            bytes = cpu.data();
            total = cpu.size();
        }
        if (total > cap - at) return fc2::fail(FC2_E_RANGE, "fc2_gpu_bgzf: the output does not fit");
        memcpy(o + at, bytes, total);
        at += total;
        return (int)FC2_OK;
    };
    uint64_t head = 0;
    for (uint64_t p = 0; p < pieces && rc == FC2_OK; ++p) {
        if (p - head == (uint64_t)bgz::kSlots) rc = collect(head++);
        const uint64_t b0 = p * piece;
        if (rc == FC2_OK && !bgz::gpu_submit(g, (int)(p % bgz::kSlots), src + b0, (size_t)std::min<uint64_t>(piece, n - b0), err))
            rc = fc2::fail(FC2_E_HIP, "fc2_gpu_bgzf: " + err);
    }
    while (rc == FC2_OK && head < pieces) rc = collect(head++);
    bgz::gpu_close(g);
    if (rc == FC2_OK) *out_n = at;
    return rc;
}
}  // namespace
