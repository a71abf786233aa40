// fc2_deflate_gpu.hip -- fc2_deflate_gpu.h: the slots of the GPU gzip writer, and fc2_gpu_gzip (one
// buffer through the same path).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>

#include "../../include/fc2_caller.h"
#include "fc2_common.h"
#include "fc2_cpuacct.h"
#include "fc2_deflate.h"
#include "fc2_deflate_gpu.h"
#include "fc2_gzmember_impl.h"

namespace fc2 {
namespace dgz {

namespace {
constexpr uint32_t kGaveUp = 0xFFFFFFFFu;      // fc2_deflate_launch's out_len of a tile it gave up
}  // namespace

struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    uint8_t *h_src = nullptr, *h_dst = nullptr, *d_src = nullptr, *d_dst = nullptr;
    uint32_t *h_meta = nullptr, *d_meta = nullptr;       // out_len | crc
    void *d_scratch = nullptr;
    size_t n = 0;                              // the piece's bytes
    uint32_t tiles = 0;
    bool busy = false;
};

struct Gpu {
    int device = 0;
    uint32_t tile = kDefaultTile, stride = 0, max_tiles = 0;
    size_t max_piece = 0;
    double timeout_s = kDefaultTimeout;
    int level = 1;
    uint32_t hist = 0;                         // > 0: fc2_deflate_launch_hist, and a piece is one member
    uint32_t depth = 0, nice = 0;              // depth > 0: fc2_deflate_launch_deep with these (level 2 only)
    uint32_t passes = 0;                       // > 1: fc2_deflate_launch_priced with these (level 2 only)
    bool hung = false;                         // a wait timed out: the device is not touched again
    Slot slot[kSlots];
};

static bool hip_ok(hipError_t e, const char *what, std::string &err) {
    if (e == hipSuccess) return true;
    err = std::string("GPU gzip: ") + what + ": " + hipGetErrorString(e);
    return false;
}

Gpu *gpu_open(int device, size_t max_piece, uint32_t tile, double timeout_s, int level, uint32_t hist, std::string &err,
              uint32_t depth, uint32_t nice, uint32_t passes) {
    if (!tile || tile > 65536 || !max_piece || device < 0 || level < 1 || level > 2 || hist > 32768 || tile + hist > 65536) {
        err = "GPU gzip: bad tile, history, piece size, device or level";
        return nullptr;
    }
    if ((depth || nice) && (level != 2 || depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX ||
                            nice < FC2_DEFLATE_NICE_MIN || nice > FC2_DEFLATE_NICE_MAX)) {
        err = "GPU gzip: the search effort needs level 2, depth 1..128 and nice 4..258";
        return nullptr;
    }
    if (passes && (level != 2 || passes < FC2_DEFLATE_PASSES_MIN || passes > FC2_DEFLATE_PASSES_MAX)) {
        err = "GPU gzip: passes need level 2 and are 1..3";
        return nullptr;
    }
    Gpu *g = new Gpu();
    g->device = device;
    g->tile = tile;
    g->stride = (FC2_DEFLATE_TILE_BOUND(tile) + 15u) & ~15u;   // slots on 16-byte boundaries: whole vector stores
    g->max_piece = max_piece;
    g->timeout_s = timeout_s > 0 ? timeout_s : kDefaultTimeout;
    g->level = level;
    g->hist = hist;
    g->depth = depth;
    g->nice = nice;
    g->passes = passes;
    g->max_tiles = (uint32_t)((max_piece + tile - 1) / tile);
    const size_t dst = (size_t)g->max_tiles * g->stride, meta = (size_t)g->max_tiles * 2 * sizeof(uint32_t);
    bool ok = hip_ok(hipSetDevice(device), "hipSetDevice", err);
    for (int k = 0; k < kSlots && ok; ++k) {
        Slot &s = g->slot[k];
        ok = hip_ok(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), "stream", err) &&
             hip_ok(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "event", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_src, max_piece, hipHostMallocDefault), "pinned input", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_dst, dst, hipHostMallocDefault), "pinned output", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_meta, meta, hipHostMallocDefault), "pinned table", err) &&
             hip_ok(hipMalloc((void **)&s.d_src, max_piece), "device input", err) &&
             hip_ok(hipMalloc((void **)&s.d_dst, dst), "device output", err) &&
             hip_ok(hipMalloc((void **)&s.d_meta, meta), "device table", err) &&
             hip_ok(hipMalloc(&s.d_scratch, (size_t)fc2_deflate_scratch_bytes(max_piece, tile)), "device scratch", err);
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
            if (s.busy) {                       // (a piece nobody waited for: bounded like every wait here)
                std::string err;
                if (gpu_wait(g, (int)(&s - g->slot), err) == TIMED_OUT) break;
            }
        }
        if (!g->hung) {
            for (Slot &s : g->slot) {
                if (s.d_scratch) (void)hipFree(s.d_scratch);
                if (s.d_meta) (void)hipFree(s.d_meta);
                if (s.d_dst) (void)hipFree(s.d_dst);
                if (s.d_src) (void)hipFree(s.d_src);
                if (s.h_meta) (void)hipHostFree(s.h_meta);
                if (s.h_dst) (void)hipHostFree(s.h_dst);
                if (s.h_src) (void)hipHostFree(s.h_src);
                if (s.done) (void)hipEventDestroy(s.done);
                if (s.stream) (void)hipStreamDestroy(s.stream);
            }
        }
    }
    delete g;
}

size_t gpu_max_piece(const Gpu *g) { return g->max_piece; }

bool gpu_submit(Gpu *g, int k, const char *data, size_t n, std::string &err) {
    if (g->hung || k < 0 || k >= kSlots || g->slot[k].busy || !n || n > g->max_piece) {
        err = "GPU gzip: no slot for the piece";
        return false;
    }
    Slot &s = g->slot[k];
    if (!hip_ok(hipSetDevice(g->device), "hipSetDevice", err)) return false;
    memcpy(s.h_src, data, n);
    s.n = n;
    s.tiles = (uint32_t)((n + g->tile - 1) / g->tile);
    const size_t w = sizeof(uint32_t);
    // (whatever was queued on the stream before a failure still runs: from the first call on the slot
    // counts as busy, and a failure drains the stream before the slot's buffers can be used again)
    s.busy = true;
    const bool ok =
        hip_ok(hipMemcpyAsync(s.d_src, s.h_src, n, hipMemcpyHostToDevice, s.stream), "upload", err) &&
        ((g->passes > 1
              ? fc2_deflate_launch_priced(s.d_src, n, 0, g->tile, g->hist, s.d_dst, g->stride, s.d_meta, s.d_meta + g->max_tiles,
                                          s.d_scratch, s.stream, g->depth ? g->depth : FC2_DEFLATE_LEVEL2_DEPTH,
                                          g->depth ? g->nice : FC2_DEFLATE_LEVEL2_NICE, g->passes)
          : g->depth ? fc2_deflate_launch_deep(s.d_src, n, 0, g->tile, g->hist, s.d_dst, g->stride, s.d_meta,
                                             s.d_meta + g->max_tiles, s.d_scratch, s.stream, g->depth, g->nice)
                   : fc2_deflate_launch_hist(s.d_src, n, g->tile, g->hist, s.d_dst, g->stride, s.d_meta,
                                             s.d_meta + g->max_tiles, s.d_scratch, s.stream, g->level)) == FC2_OK ||
         ((err = "GPU gzip: launch failed"), false)) &&
        hip_ok(hipMemcpyAsync(s.h_dst, s.d_dst, (size_t)s.tiles * g->stride, hipMemcpyDeviceToHost, s.stream), "download", err) &&
        hip_ok(hipMemcpyAsync(s.h_meta, s.d_meta, s.tiles * w, hipMemcpyDeviceToHost, s.stream), "download", err) &&
        hip_ok(hipMemcpyAsync(s.h_meta + g->max_tiles, s.d_meta + g->max_tiles, s.tiles * w, hipMemcpyDeviceToHost, s.stream),
               "download", err) &&
        hip_ok(hipEventRecord(s.done, s.stream), "event", err);
    if (!ok) {
        std::string ignored;
        (void)hipEventRecord(s.done, s.stream);
        if (gpu_wait(g, k, ignored) == TIMED_OUT) err = ignored;
        return false;
    }
    return true;
}

Wait gpu_wait(Gpu *g, int k, std::string &err) {
    Slot &s = g->slot[k];
    if (g->hung) {
        err = "GPU gzip: the device timed out earlier";
        return FAILED;
    }
    if (!s.busy) {
        err = "GPU gzip: nothing to wait for";
        return FAILED;
    }
    if (!hip_ok(hipSetDevice(g->device), "hipSetDevice", err)) {
        s.busy = false;
        return FAILED;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const double limit = g->timeout_s;
    int spins = 0;
    for (;;) {
        const hipError_t e = hipEventQuery(s.done);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) {
            hip_ok(e, "kernel", err);
            s.busy = false;
            return FAILED;
        }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) {
            g->hung = true;
            err = "GPU gzip: the device did not answer within " + std::to_string((int)limit) + " s";
            return TIMED_OUT;
        }
        // a piece takes a millisecond or two of kernel time and its copies: look again soon, then sleep longer
        if (++spins < 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
        else std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    s.busy = false;
    return DONE;
}

size_t gpu_members_size(const Gpu *g, int k) {
    const Slot &s = g->slot[k];
    if (g->hist) return (size_t)gzm::member_size(s.h_meta, s.tiles, s.n, g->tile);   // one member (fc2_gzmember_impl.h)
    size_t total = 0;
    for (uint32_t i = 0; i < s.tiles; ++i) {
        const uint32_t len = s.h_meta[i];
        if (len == kGaveUp || len == 0 || len > FC2_DEFLATE_TILE_BOUND(g->tile)) return 0;
        total += kMemberOverhead + len;
    }
    return total;
}

void gpu_members_write(const Gpu *g, int k, char *dst) {
    static const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    const Slot &s = g->slot[k];
    uint8_t *d = reinterpret_cast<uint8_t *>(dst);
    if (g->hist) {
        gzm::member_write(s.h_dst, g->stride, s.h_meta, s.h_meta + g->max_tiles, s.tiles, s.n, g->tile, d);
        return;
    }
    for (uint32_t i = 0; i < s.tiles; ++i) {
        const uint32_t len = s.h_meta[i], crc = s.h_meta[g->max_tiles + i];
        const uint64_t at = (uint64_t)i * g->tile;
        const uint32_t isize = (uint32_t)(s.n - at < g->tile ? s.n - at : g->tile);
        memcpy(d, head, 10);
        memcpy(d + 10, s.h_dst + (size_t)i * g->stride, len);
        d += 10 + len;
        for (int b = 0; b < 4; ++b) d[b] = (uint8_t)(crc >> (8 * b));
        for (int b = 0; b < 4; ++b) d[4 + b] = (uint8_t)(isize >> (8 * b));
        d += 8;
    }
}

}  // namespace dgz
}  // namespace fc2

extern "C" uint64_t fc2_gpu_gzip_bound(uint64_t n, uint32_t tile) {
    if (!tile || tile > 65536) return 0;
    const uint64_t tiles = (n + tile - 1) / tile;
    // a member per tile: the stream at its worst and the 18 bytes around it; an empty input: one empty member
    return n + tiles * (16 + fc2::dgz::kMemberOverhead) + 64;
}

extern "C" int fc2_gpu_gzip(int device, const void *in, uint64_t n, uint32_t tile, void *out, uint64_t cap, uint64_t *out_n) {
    return fc2_gpu_gzip_level(device, in, n, tile, 1, out, cap, out_n);
}

extern "C" int fc2_gpu_gzip_level(int device, const void *in, uint64_t n, uint32_t tile, int level, void *out, uint64_t cap,
                                  uint64_t *out_n) {
    return fc2_gpu_gzip_hist(device, in, n, tile, 0, level, out, cap, out_n);
}

namespace {
int gpu_gzip(int device, const void *in, uint64_t n, uint32_t tile, uint32_t hist, int level, uint32_t depth, uint32_t nice,
             void *out, uint64_t cap, uint64_t *out_n, uint32_t passes = 0);
}  // namespace

extern "C" int fc2_gpu_gzip_hist(int device, const void *in, uint64_t n, uint32_t tile, uint32_t hist, int level, void *out,
                                 uint64_t cap, uint64_t *out_n) {
    return gpu_gzip(device, in, n, tile, hist, level, 0, 0, out, cap, out_n);
}

extern "C" int fc2_gpu_gzip_deep(int device, const void *in, uint64_t n, uint32_t tile, uint32_t hist, uint32_t depth,
                                 uint32_t nice, void *out, uint64_t cap, uint64_t *out_n) {
    if (depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX || nice < FC2_DEFLATE_NICE_MIN ||
        nice > FC2_DEFLATE_NICE_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_gzip_deep: depth is 1..128, nice 4..258");
    return gpu_gzip(device, in, n, tile, hist, 2, depth, nice, out, cap, out_n);
}

extern "C" int fc2_gpu_gzip_priced(int device, const void *in, uint64_t n, uint32_t tile, uint32_t hist, uint32_t depth,
                                   uint32_t nice, uint32_t passes, void *out, uint64_t cap, uint64_t *out_n) {
    if (passes < FC2_DEFLATE_PASSES_MIN || passes > FC2_DEFLATE_PASSES_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_gzip_priced: passes is 1..3");
    if (depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX || nice < FC2_DEFLATE_NICE_MIN ||
        nice > FC2_DEFLATE_NICE_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_gzip_priced: depth is 1..128, nice 4..258");
    return gpu_gzip(device, in, n, tile, hist, 2, depth, nice, out, cap, out_n, passes);
}

namespace {
int gpu_gzip(int device, const void *in, uint64_t n, uint32_t tile, uint32_t hist, int level, uint32_t depth, uint32_t nice,
             void *out, uint64_t cap, uint64_t *out_n, uint32_t passes) {
    using namespace fc2;
    if (!tile || tile > 65536 || device < 0 || !out || !out_n || (!in && n) || level < 1 || level > 2 || hist > 32768 ||
        tile + hist > 65536)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_gzip: bad arguments");
    *out_n = 0;
    char *o = static_cast<char *>(out);
    uint64_t at = 0;
    if (!n) {                                   // one empty member, from the CPU
        std::string m;
        if (!dfl::gzip_member(std::string(), 1, m)) return fc2::fail(FC2_E_IO, "fc2_gpu_gzip: cannot compress");
        if (m.size() > cap) return fc2::fail(FC2_E_RANGE, "fc2_gpu_gzip: the output does not fit");
        memcpy(o, m.data(), m.size());
        *out_n = m.size();
        return FC2_OK;
    }
    const size_t piece = size_t(4) << 20;
    std::string err;
    dgz::Gpu *g = dgz::gpu_open(device, piece, tile, 0, level, hist, err, depth, nice, passes);
    if (!g) return fc2::fail(FC2_E_HIP, "fc2_gpu_gzip: " + err);
    const char *src = static_cast<const char *>(in);
    const uint64_t pieces = (n + piece - 1) / piece;
    int rc = FC2_OK;
    // piece p goes into slot p % kSlots while piece p - 1 is assembled: two of the slots are in use at a time
    for (uint64_t p = 0; p <= pieces && rc == FC2_OK; ++p) {
        if (p < pieces) {
            const uint64_t b0 = p * piece;
            if (!dgz::gpu_submit(g, (int)(p % dgz::kSlots), src + b0, (size_t)std::min<uint64_t>(piece, n - b0), err))
                rc = fc2::fail(FC2_E_HIP, "fc2_gpu_gzip: " + err);
        }
        if (p > 0 && rc == FC2_OK) {
            const int k = (int)((p - 1) % dgz::kSlots);
            const dgz::Wait w = dgz::gpu_wait(g, k, err);
            if (w != dgz::DONE) {
                rc = fc2::fail(w == dgz::TIMED_OUT ? FC2_E_IO : FC2_E_HIP, "fc2_gpu_gzip: piece " + std::to_string(p - 1) + ": " + err);
                break;
            }
            const size_t sz = dgz::gpu_members_size(g, k);
            if (sz) {
                if (sz > cap - at) { rc = fc2::fail(FC2_E_RANGE, "fc2_gpu_gzip: the output does not fit"); break; }
                dgz::gpu_members_write(g, k, o + at);
                at += sz;
            } else {                            // a tile given up: this piece from the CPU
                const uint64_t b0 = (p - 1) * piece;
                std::string m;
                if (!dfl::gzip_member(std::string(src + b0, (size_t)std::min<uint64_t>(piece, n - b0)), 1, m)) {
                    rc = fc2::fail(FC2_E_IO, "fc2_gpu_gzip: cannot compress");
                    break;
                }
                if (m.size() > cap - at) { rc = fc2::fail(FC2_E_RANGE, "fc2_gpu_gzip: the output does not fit"); break; }
                memcpy(o + at, m.data(), m.size());
                at += m.size();
            }
        }
    }
    dgz::gpu_close(g);
    if (rc == FC2_OK) *out_n = at;
    return rc;
}
}  // namespace
