// fc2_sam_group.hip -- unspliced fragments of SAM text closed on the GPU: sam_nl_count_kernel counts the `\n` of
// every segment of a block, sam_nl_scan_kernel turns the counts into offsets, sam_nl_fill_kernel writes the
// lines' starts in place, sam_head_kernel makes every line's head row (a wavefront a line) and sam_frag_kernel
// every line's fragment row (a lane a line) -- the rule: fc2_sam_frag_impl.h; the host entry over the same
// rule, and the slots of the ingest's stage (fc2_sam_group_gpu.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fc2_ingest.h"
#include "fc2_common.h"
#include "fc2_sam_frag_impl.h"
#include "fc2_sam_group_gpu.h"

namespace {

using namespace fc2::samfrag;

constexpr uint32_t kThreads = 256, kWavesPerBlock = kThreads / 64;
constexpr uint32_t kSeg = FC2_SAM_GROUP_SEG;
constexpr uint32_t kScanThreads = 1024;         // each sums at most 16 of a block's 16384 segment counts
constexpr uint32_t kHeadBlocks = 4096, kFragBlocks = 1024;     // the grids' limits: the kernels stride

// the device's group: a wavefront
struct Wave {
    static constexpr uint32_t width = 64;
    __host__ __device__ uint32_t lane() const {
#if defined(__HIP_DEVICE_COMPILE__)
        return threadIdx.x & 63u;
#else
        return 0;
#endif
    }
    __host__ __device__ uint64_t ballot(bool p) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return __ballot(p);
#else
        return p ? 1u : 0u;
#endif
    }
};

// A wavefront a segment: 64 bytes a ballot, the `\n` among them counted.  Segment s is text[s * kSeg ..
// min((s + 1) * kSeg, n_bytes)); lane 0 stores the count.
__global__ __launch_bounds__(kThreads) void sam_nl_count_kernel(const uint8_t *__restrict__ text, uint32_t n_bytes,
                                                                uint32_t n_segs, uint32_t *__restrict__ cnt) {
    const uint32_t s = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (s >= n_segs) return;
    const uint32_t a = s * kSeg, b = min(a + kSeg, n_bytes);
    uint32_t c = 0;
    for (uint32_t p = a; p < b; p += 64) {
        const uint32_t i = p + lane;
        c += (uint32_t)__popcll(__ballot(i < b && text[i] == '\n'));
    }
    if (lane == 0) cnt[s] = c;
}

// One workgroup: the counts become the segments' first line numbers (in place), cnt[n_segs] and *n_lines the
// sum; starts[0] = 0 where the lines fit the rows (n_lines <= cap).
__global__ __launch_bounds__(kScanThreads) void sam_nl_scan_kernel(uint32_t *__restrict__ cnt, uint32_t n_segs,
                                                                   uint32_t *__restrict__ starts, uint32_t *__restrict__ n_lines,
                                                                   uint32_t cap) {
    __shared__ uint32_t sum[kScanThreads];
    const uint32_t t = threadIdx.x, per = (n_segs + kScanThreads - 1) / kScanThreads;
    const uint32_t j0 = min(t * per, n_segs), j1 = min(j0 + per, n_segs);
    uint32_t mine = 0;
    for (uint32_t j = j0; j < j1; ++j) mine += cnt[j];
    sum[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
        const uint32_t v = t >= d ? sum[t - d] : 0;
        __syncthreads();
        sum[t] += v;
        __syncthreads();
    }
    uint32_t run = sum[t] - mine;
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t c = cnt[j];
        cnt[j] = run;
        run += c;
    }
    if (t == kScanThreads - 1) {
        cnt[n_segs] = sum[t];
        *n_lines = sum[t];
        if (sum[t] <= cap) starts[0] = 0;
    }
}

// A wavefront a segment again: the k-th `\n` of the text, at byte i, gives starts[k + 1] = i + 1; its number is
// the segment's first one, the `\n` of the ballots before and those of the lanes below.  k + 1 <= n_lines <= cap.
__global__ __launch_bounds__(kThreads) void sam_nl_fill_kernel(const uint8_t *__restrict__ text, uint32_t n_bytes,
                                                               uint32_t n_segs, const uint32_t *__restrict__ cnt,
                                                               uint32_t *__restrict__ starts, uint32_t cap) {
    const uint32_t s = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (s >= n_segs || cnt[n_segs] > cap) return;
    const uint32_t a = s * kSeg, b = min(a + kSeg, n_bytes);
    uint32_t k = cnt[s];
    for (uint32_t p = a; p < b; p += 64) {
        const uint32_t i = p + lane;
        const bool nl = i < b && text[i] == '\n';
        const uint64_t m = __ballot(nl);
        if (nl) starts[k + (uint32_t)__popcll(m & ((1ull << lane) - 1)) + 1] = i + 1;
        k += (uint32_t)__popcll(m);
    }
}

// A wavefront a line, four lines a workgroup at a time.  The line's number is the same in all 64 lanes, so is
// everything head_row branches on; loads lie in the line, which the listing placed inside the text; lane 0
// stores the row.
__global__ __launch_bounds__(kThreads) void sam_head_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ starts,
                                                            const uint32_t *__restrict__ n_lines, uint32_t cap,
                                                            const uint32_t *__restrict__ table, uint32_t table_bytes,
                                                            fc2_sam_head *__restrict__ rows) {
    const uint32_t n = *n_lines;
    if (n > cap) return;
    const Wave g;
    for (uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); i < n; i += gridDim.x * kWavesPerBlock) {
        const fc2_sam_head row = head_row(g, text, starts[i], starts[i + 1] - 1, table, table_bytes);
        if (g.lane() == 0) rows[i] = row;
    }
}

// A line a lane: the walk back and forward over the head rows, the names compared in the text.
__global__ __launch_bounds__(kThreads) void sam_frag_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ starts,
                                                            const uint32_t *__restrict__ n_lines, uint32_t cap,
                                                            const fc2_sam_head *__restrict__ rows,
                                                            fc2_bam_frag *__restrict__ frag_rows) {
    const uint32_t n = *n_lines;
    if (n > cap) return;
    const Tables T = {text, starts, rows, n};
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) frag_rows[i] = frag_row(T, i);
}

int check_args(const char *who, const void *text, uint32_t n_bytes, const void *table, uint32_t table_bytes, const void *starts,
               const void *line_rows, const void *frag_rows, const void *n_lines) {
    const std::string w(who);
    if ((!text && n_bytes) || !table || !starts || !line_rows || !frag_rows || !n_lines) return fc2::fail(FC2_E_PARAM, w + ": null argument");
    if (n_bytes > FC2_SAM_GROUP_MAX_TEXT) return fc2::fail(FC2_E_PARAM, w + ": a block is at most 16 MiB of text");
    if (table_bytes < 8 || (table_bytes & 3u)) return fc2::fail(FC2_E_PARAM, w + ": not a table of fc2_sam_names_table");
    return FC2_OK;
}

}  // namespace

extern "C" int fc2_sam_group_launch(const uint8_t *text, uint32_t n_bytes, const uint32_t *names_table, uint32_t table_bytes,
                                    uint32_t *starts, fc2_sam_head *line_rows, fc2_bam_frag *frag_rows, uint32_t *n_lines_out,
                                    uint32_t cap, uint32_t *scratch, void *stream) {
    if (int rc = check_args("fc2_sam_group_launch", text, n_bytes, names_table, table_bytes, starts, line_rows, frag_rows, n_lines_out))
        return rc;
    if (!scratch) return fc2::fail(FC2_E_PARAM, "fc2_sam_group_launch: null argument");
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t n_segs = (n_bytes + kSeg - 1) / kSeg, seg_grid = (n_segs + kWavesPerBlock - 1) / kWavesPerBlock;
    hipError_t e = hipSuccess;
    if (n_segs) {
        hipLaunchKernelGGL(sam_nl_count_kernel, dim3(seg_grid), dim3(kThreads), 0, s, text, n_bytes, n_segs, scratch);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sam_nl_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, scratch, n_segs, starts, n_lines_out, cap);
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_segs && cap) {
        hipLaunchKernelGGL(sam_nl_fill_kernel, dim3(seg_grid), dim3(kThreads), 0, s, text, n_bytes, n_segs, scratch, starts, cap);
        e = hipGetLastError();
        if (e == hipSuccess) {
            const uint32_t grid = std::min((cap + kWavesPerBlock - 1) / kWavesPerBlock, kHeadBlocks);
            hipLaunchKernelGGL(sam_head_kernel, dim3(grid), dim3(kThreads), 0, s, text, starts, n_lines_out, cap, names_table,
                               table_bytes, line_rows);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            const uint32_t grid = std::min((cap + kThreads - 1) / kThreads, kFragBlocks);
            hipLaunchKernelGGL(sam_frag_kernel, dim3(grid), dim3(kThreads), 0, s, text, starts, n_lines_out, cap, line_rows, frag_rows);
            e = hipGetLastError();
        }
    }
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_sam_group_launch: ") + hipGetErrorString(e));
}

extern "C" int fc2_sam_group_host(const uint8_t *text, uint32_t n_bytes, const uint32_t *names_table, uint32_t table_bytes,
                                  uint32_t *starts, fc2_sam_head *line_rows, fc2_bam_frag *frag_rows, uint32_t *n_lines_out,
                                  uint32_t cap) {
    if (n_lines_out) *n_lines_out = 0;
    if (int rc = check_args("fc2_sam_group_host", text, n_bytes, names_table, table_bytes, starts, line_rows, frag_rows, n_lines_out))
        return rc;
    if (names_table[1] != table_bytes) return fc2::fail(FC2_E_PARAM, "fc2_sam_group_host: not a table of fc2_sam_names_table");
    group_text(text, n_bytes, names_table, table_bytes, starts, line_rows, frag_rows, n_lines_out, cap);
    return FC2_OK;
}

// ---- the stage's slots -----------------------------------------------------------------------------------

namespace fc2 {
namespace samgrp {

struct Slot {
    bool made = false, queued = false;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    char *h_text = nullptr;
    uint32_t *h_rows = nullptr;                 // n_lines | starts (cap + 1) | frag rows (cap)
    uint8_t *d_text = nullptr;
    uint32_t *d_rows = nullptr;                 // the same three, then the head rows and the scratch
    std::vector<fc2_sam_head> heads;            // mode 2: the twin's head rows
};

struct Stage {
    int mode = 0, device = 0;
    uint32_t max_text = 0, cap = 0, table_bytes = 0;
    double timeout_s = kDefaultTimeout;
    std::vector<uint32_t> table;
    uint32_t *d_table = nullptr;
    std::atomic<bool> dead{false};              // a HIP call failed: every later block is the host's
    std::atomic<bool> hung{false};              // a wait timed out: the device is not touched again
    std::mutex m;
    std::vector<int> free_slots;                // (taken from the back: few slots are ever made while the reader keeps up)
    std::vector<Slot> slot;
};

static size_t row_words(const Stage *s) { return 2 + (size_t)s->cap + 2 * (size_t)s->cap; }      // (cap is even: the rows are 8-byte aligned)

static bool hip_ok(hipError_t e) { return e == hipSuccess; }

static void free_slot(Stage *s, Slot &t) {
    if (s->mode == 2) {
        free(t.h_text);
        free(t.h_rows);
    } else {
        if (t.d_rows) (void)hipFree(t.d_rows);
        if (t.d_text) (void)hipFree(t.d_text);
        if (t.h_rows) (void)hipHostFree(t.h_rows);
        if (t.h_text) (void)hipHostFree(t.h_text);
        if (t.done) (void)hipEventDestroy(t.done);
        if (t.stream) (void)hipStreamDestroy(t.stream);
    }
    t = Slot();
}

// the slot's buffers, when it is first taken
static bool make_slot(Stage *s, Slot &t) {
    const size_t rows = row_words(s) * sizeof(uint32_t);
    if (s->mode == 2) {
        t.h_text = static_cast<char *>(malloc(s->max_text));
        t.h_rows = static_cast<uint32_t *>(malloc(rows));
        t.heads.resize(s->cap);
        t.made = t.h_text && t.h_rows;
    } else {
        const size_t dev_words = row_words(s) + 4 * (size_t)s->cap + (size_t)FC2_SAM_GROUP_SCRATCH(s->max_text);
        t.made = hip_ok(hipSetDevice(s->device)) && hip_ok(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking)) &&
                 hip_ok(hipEventCreateWithFlags(&t.done, hipEventDisableTiming)) &&
                 hip_ok(hipHostMalloc((void **)&t.h_text, s->max_text, hipHostMallocDefault)) &&
                 hip_ok(hipHostMalloc((void **)&t.h_rows, rows, hipHostMallocDefault)) &&
                 hip_ok(hipMalloc((void **)&t.d_text, s->max_text)) &&
                 hip_ok(hipMalloc((void **)&t.d_rows, dev_words * sizeof(uint32_t)));
    }
    if (!t.made) free_slot(s, t);
    return t.made;
}

// the slot's event against the deadline
static Wait wait_event(Stage *s, Slot &t, std::string &err) {
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    for (;;) {
        const hipError_t e = hipEventQuery(t.done);
        if (e == hipSuccess) return DONE;
        if (e != hipErrorNotReady) {
            s->dead = true;
            return NONE;
        }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > s->timeout_s) {
            s->hung = true;
            err = "GPU SAM group: the device did not answer within " + std::to_string((int)s->timeout_s) + " s";
            return TIMED_OUT;
        }
        if (++spins < 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
        else std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

Stage *open(int mode, int device, int n_slots, uint32_t max_text, uint32_t cap, double timeout_s, const std::vector<uint32_t> &table,
            std::string &err) {
    if ((mode != 1 && mode != 2) || device < 0 || n_slots < 1 || !max_text || max_text > FC2_SAM_GROUP_MAX_TEXT || table.size() < 2) {
        err = "GPU SAM group: bad mode, device, slots, text or table";
        return nullptr;
    }
    Stage *s = new Stage();
    s->mode = mode;
    s->device = device;
    s->max_text = max_text;
    s->cap = (cap + 1) & ~1u;
    s->timeout_s = timeout_s > 0 ? timeout_s : kDefaultTimeout;
    s->table = table;
    s->table_bytes = (uint32_t)(table.size() * 4);
    s->slot.resize((size_t)n_slots);
    for (int k = n_slots - 1; k >= 0; --k) s->free_slots.push_back(k);
    if (mode == 1) {
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_table, s->table_bytes);
        if (e == hipSuccess) e = hipMemcpy(s->d_table, table.data(), s->table_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            err = std::string("GPU SAM group: ") + hipGetErrorString(e);
            if (s->d_table) (void)hipFree(s->d_table);
            delete s;
            return nullptr;
        }
    }
    return s;
}

void close(Stage *s) {
    if (!s) return;
    if (s->mode == 2) {
        for (Slot &t : s->slot) free_slot(s, t);
    } else if (!s->hung && hipSetDevice(s->device) == hipSuccess) {
        for (Slot &t : s->slot) {
            if (t.made && t.queued) {            // (a block nobody collected: bounded like every wait here)
                std::string err;
                if (wait_event(s, t, err) == TIMED_OUT) break;
                t.queued = false;
            }
        }
        if (!s->hung) {
            for (Slot &t : s->slot) free_slot(s, t);
            if (s->d_table) (void)hipFree(s->d_table);
        }
    }
    delete s;
}

uint32_t max_text(const Stage *s) { return s->max_text; }

int acquire(Stage *s, char *&text) {
    text = nullptr;
    if (s->dead || s->hung) return -1;
    int k;
    {
        std::lock_guard<std::mutex> lk(s->m);
        if (s->free_slots.empty()) return -1;
        k = s->free_slots.back();
        s->free_slots.pop_back();
    }
    Slot &t = s->slot[(size_t)k];
    if (!t.made && !make_slot(s, t)) {
        s->dead = true;
        std::lock_guard<std::mutex> lk(s->m);
        s->free_slots.push_back(k);
        return -1;
    }
    text = t.h_text;
    return k;
}

void release(Stage *s, int k) {
    if (k < 0 || (size_t)k >= s->slot.size()) return;
    Slot &t = s->slot[(size_t)k];
    if (t.queued) {
        if (s->hung) return;                    // (its buffers may still be written: the slot never comes back)
        std::string err;
        if (s->mode == 1 && (hipSetDevice(s->device) != hipSuccess || wait_event(s, t, err) == TIMED_OUT)) return;
        t.queued = false;
    }
    std::lock_guard<std::mutex> lk(s->m);
    s->free_slots.push_back(k);
}

bool submit(Stage *s, int k, uint32_t n_bytes) {
    if (k < 0 || (size_t)k >= s->slot.size() || s->dead || s->hung || n_bytes > s->max_text) return false;
    Slot &t = s->slot[(size_t)k];
    if (!t.made || t.queued) return false;
    uint32_t *const h_n = t.h_rows, *const h_starts = h_n + 1;
    fc2_bam_frag *const h_frags = reinterpret_cast<fc2_bam_frag *>(t.h_rows + 2 + s->cap);
    *h_n = 0xFFFFFFFFu;
    if (s->mode == 2) {
        if (fc2_sam_group_host(reinterpret_cast<const uint8_t *>(t.h_text), n_bytes, s->table.data(), s->table_bytes, h_starts,
                               t.heads.data(), h_frags, h_n, s->cap) != FC2_OK)
            return false;
        t.queued = true;
        return true;
    }
    uint32_t *const d_n = t.d_rows, *const d_starts = d_n + 1;
    fc2_bam_frag *const d_frags = reinterpret_cast<fc2_bam_frag *>(t.d_rows + 2 + s->cap);
    fc2_sam_head *const d_heads = reinterpret_cast<fc2_sam_head *>(t.d_rows + row_words(s));
    uint32_t *const d_scratch = t.d_rows + row_words(s) + 4 * (size_t)s->cap;
    if (!hip_ok(hipSetDevice(s->device))) {
        s->dead = true;
        return false;
    }
    // (whatever was queued on the stream before a failure still runs: from the first call on the slot counts as
    // queued, and release() or collect() drains the stream before the buffers are used again)
    t.queued = true;
    const bool ok = (!n_bytes || hip_ok(hipMemcpyAsync(t.d_text, t.h_text, n_bytes, hipMemcpyHostToDevice, t.stream))) &&
                    fc2_sam_group_launch(t.d_text, n_bytes, s->d_table, s->table_bytes, d_starts, d_heads, d_frags, d_n, s->cap, d_scratch,
                                         t.stream) == FC2_OK &&
                    hip_ok(hipMemcpyAsync(t.h_rows, t.d_rows, row_words(s) * sizeof(uint32_t), hipMemcpyDeviceToHost, t.stream));
    if (!ok) s->dead = true;
    if (!hip_ok(hipEventRecord(t.done, t.stream))) s->dead = true;
    return true;                                // (collect waits for the event either way, and answers NONE after a failure)
}

Wait collect(Stage *s, int k, const uint32_t *&starts, const fc2_bam_frag *&frags, uint32_t &n_lines, std::string &err) {
    starts = nullptr;
    frags = nullptr;
    n_lines = 0;
    if (k < 0 || (size_t)k >= s->slot.size() || !s->slot[(size_t)k].queued) return NONE;
    Slot &t = s->slot[(size_t)k];
    if (s->mode == 1) {
        if (s->hung) return NONE;               // (the slot stays queued: it never comes back)
        if (!hip_ok(hipSetDevice(s->device))) {
            s->dead = true;
            return NONE;
        }
        const Wait w = wait_event(s, t, err);
        if (w == TIMED_OUT) return w;
        t.queued = false;
        if (w != DONE || s->dead) return NONE;
    } else {
        t.queued = false;
    }
    const uint32_t n = t.h_rows[0];
    if (n > s->cap) return NONE;                // more lines than rows (0xFFFFFFFF: nothing came back)
    starts = t.h_rows + 1;
    frags = reinterpret_cast<const fc2_bam_frag *>(t.h_rows + 2 + s->cap);
    n_lines = n;
    return DONE;
}

}  // namespace samgrp
}  // namespace fc2
