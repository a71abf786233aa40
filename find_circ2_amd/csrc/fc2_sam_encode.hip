// fc2_sam_encode.hip -- BAM records from SAM text on the GPU: sam_size_kernel decides every line of a batch and
// sizes its record, sam_scan_kernel turns the sizes into offsets, sam_write_kernel writes the accepted records
// back to back (the rule: fc2_sam_encode_impl.h); the host entry over the same rule, the names' table, the
// slots of the writer's encode stage (fc2_sam_enc_gpu.h), and fc2_gpu_sam_encode (any number of lines through
// the same slots).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fc2_ingest.h"
#include "fc2_common.h"
#include "fc2_sam_enc_gpu.h"
#include "fc2_sam_encode_impl.h"

namespace {

using namespace fc2::samenc;

constexpr uint32_t kThreads = 256, kWavesPerBlock = kThreads / 64;
constexpr uint32_t kScanThreads = 1024;         // each sums at most 16 of a batch's 16384 sizes

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

// A wavefront a line, four lines a workgroup.  The line index is the same in all 64 lanes, so is everything
// parse() branches on: the ballots in find_tab see the whole wavefront.  Loads lie in the line, which line_of
// has placed inside the text; lane 0 stores the line's two words.
__global__ __launch_bounds__(kThreads) void sam_size_kernel(const uint8_t *__restrict__ text, uint32_t text_bytes,
                                                            const uint32_t *__restrict__ off, uint32_t n_lines,
                                                            const uint32_t *__restrict__ table, uint32_t table_bytes,
                                                            uint32_t *__restrict__ size, uint32_t *__restrict__ status) {
    const uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (i >= n_lines) return;
    const Wave g;
    uint32_t a, b, st = FC2_SAM_ENC_OFFSETS, sz = 0;
    if (line_of(off, i, text_bytes, a, b)) {
        const Plan P = parse(g, text, a, b, table, table_bytes);
        st = P.status, sz = P.size;
    }
    if (g.lane() == 0) status[i] = st, size[i] = sz;
}

// One workgroup: thread t sums its share of the sizes, the shares are scanned in LDS, and every thread writes
// its share's offsets; out_off[n_lines] and *total are the sum (at most 2 * 4 MiB + 40 * 16384: 32 bits hold it).
__global__ __launch_bounds__(kScanThreads) void sam_scan_kernel(const uint32_t *__restrict__ size, uint32_t n_lines,
                                                                uint32_t *__restrict__ out_off, uint32_t *__restrict__ total) {
    __shared__ uint32_t sum[kScanThreads];
    const uint32_t t = threadIdx.x, per = (n_lines + kScanThreads - 1) / kScanThreads;
    const uint32_t j0 = min(t * per, n_lines), j1 = min(j0 + per, n_lines);
    uint32_t mine = 0;
    for (uint32_t j = j0; j < j1; ++j) mine += size[j];
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
        out_off[j] = run;
        run += size[j];
    }
    if (t == kScanThreads - 1) out_off[n_lines] = sum[t], *total = sum[t];
}

// A wavefront a line again: the line is parsed as in the sizing pass (the same code on the same bytes: the
// same plan), and an accepted line's record goes to out + out_off[i], its runs of bytes -- name, packed bases,
// qualities, Z values -- spread over the lanes.  Every store lies in [out + out_off[i], out + out_off[i] +
// size[i]), which the scan placed below *total, and a record that would pass out_cap is left out.
__global__ __launch_bounds__(kThreads) void sam_write_kernel(const uint8_t *__restrict__ text, uint32_t text_bytes,
                                                             const uint32_t *__restrict__ off, uint32_t n_lines,
                                                             const uint32_t *__restrict__ table, uint32_t table_bytes,
                                                             const uint32_t *__restrict__ out_off, uint8_t *__restrict__ out,
                                                             uint64_t out_cap) {
    const uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (i >= n_lines) return;
    const Wave g;
    uint32_t a, b;
    if (!line_of(off, i, text_bytes, a, b)) return;
    const Plan P = parse(g, text, a, b, table, table_bytes);
    if (P.status != FC2_SAM_ENC_OK) return;
    const uint32_t at = out_off[i];
    if ((uint64_t)at + P.size > out_cap) return;
    write(g, text, P, out + at);
}

int check_args(const char *who, const void *text, uint32_t text_bytes, const void *off, uint32_t n_lines, const void *table,
               uint32_t table_bytes, const void *out, uint64_t out_cap, const void *out_off, const void *size,
               const void *status, const void *total) {
    const std::string w(who);
    if (!text || !off || !table || !out || !out_off || !size || !status || !total) return fc2::fail(FC2_E_PARAM, w + ": null argument");
    if (!n_lines || n_lines > kMaxLines || text_bytes > kMaxText)
        return fc2::fail(FC2_E_PARAM, w + ": a batch is 1..16384 lines and at most 4 MiB of text");
    if (table_bytes < 8 || (table_bytes & 3u)) return fc2::fail(FC2_E_PARAM, w + ": not a table of fc2_sam_names_table");
    if (out_cap < FC2_SAM_ENC_BOUND(text_bytes, n_lines))
        return fc2::fail(FC2_E_PARAM, w + ": out_cap below FC2_SAM_ENC_BOUND(text_bytes, n_lines)");
    return FC2_OK;
}

}  // namespace

extern "C" int fc2_sam_encode_launch(const uint8_t *text, uint32_t text_bytes, const uint32_t *off, uint32_t n_lines,
                                     const uint32_t *names_table, uint32_t table_bytes, uint8_t *out, uint64_t out_cap,
                                     uint32_t *out_off, uint32_t *size, uint32_t *status, uint32_t *total, void *stream) {
    if (int rc = check_args("fc2_sam_encode_launch", text, text_bytes, off, n_lines, names_table, table_bytes, out, out_cap,
                            out_off, size, status, total))
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t grid = (n_lines + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(sam_size_kernel, dim3(grid), dim3(kThreads), 0, s, text, text_bytes, off, n_lines, names_table,
                       table_bytes, size, status);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sam_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, size, n_lines, out_off, total);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sam_write_kernel, dim3(grid), dim3(kThreads), 0, s, text, text_bytes, off, n_lines, names_table,
                           table_bytes, out_off, out, out_cap);
        e = hipGetLastError();
    }
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_sam_encode_launch: ") + hipGetErrorString(e));
}

extern "C" int fc2_sam_encode_host(const uint8_t *text, uint32_t text_bytes, const uint32_t *off, uint32_t n_lines,
                                   const uint32_t *names_table, uint32_t table_bytes, uint8_t *out, uint64_t out_cap,
                                   uint32_t *out_off, uint32_t *size, uint32_t *status, uint32_t *total) {
    if (total) *total = 0;
    if (int rc = check_args("fc2_sam_encode_host", text, text_bytes, off, n_lines, names_table, table_bytes, out, out_cap,
                            out_off, size, status, total))
        return rc;
    if (names_table[1] != table_bytes) return fc2::fail(FC2_E_PARAM, "fc2_sam_encode_host: not a table of fc2_sam_names_table");
    encode_batch(text, text_bytes, off, n_lines, names_table, table_bytes, out, out_cap, out_off, size, status, total);
    return FC2_OK;
}

// ---- the names' table ----------------------------------------------------------------------------------

std::vector<uint32_t> fc2::samenc::names_table(const std::vector<std::string> &names) {
    std::vector<const char *> p(names.size());
    std::vector<uint32_t> l(names.size());
    for (size_t i = 0; i < names.size(); ++i) p[i] = names[i].data(), l[i] = (uint32_t)names[i].size();
    return build_table(p.data(), l.data(), (uint32_t)names.size());
}

extern "C" int fc2_sam_names_table(const char *const *names, const uint32_t *lens, uint32_t n_names, uint32_t *table,
                                   uint64_t cap, uint64_t *need) {
    if ((!names && n_names) || !need) return fc2::fail(FC2_E_PARAM, "fc2_sam_names_table: null argument");
    for (uint32_t i = 0; i < n_names; ++i)
        if (!names[i]) return fc2::fail(FC2_E_PARAM, "fc2_sam_names_table: null name");
    const std::vector<uint32_t> t = build_table(names, lens, n_names);
    if (t.empty()) return fc2::fail(FC2_E_RANGE, "fc2_sam_names_table: the names do not fit a table");
    *need = (uint64_t)t.size() * 4;
    if (!table) return FC2_OK;
    if (cap < *need) return fc2::fail(FC2_E_RANGE, "fc2_sam_names_table: the table does not fit");
    memcpy(table, t.data(), t.size() * 4);
    return FC2_OK;
}

// ---- the encode stage's slots ----------------------------------------------------------------------------

namespace fc2 {
namespace samenc {

struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    char *h_text = nullptr;
    uint32_t *h_off = nullptr, *h_st = nullptr;         // h_st: total, then the statuses
    uint8_t *h_out = nullptr, *d_text = nullptr, *d_out = nullptr;
    uint32_t *d_meta = nullptr;                 // off (max_lines + 1) | out_off (max_lines + 1) | size | total, status
    uint32_t n_lines = 0;
    bool busy = false;
};

struct Gpu {
    int device = 0;
    uint32_t max_lines = 0, max_text = 0, table_bytes = 0;
    size_t out_cap = 0;
    double timeout_s = kDefaultTimeout;
    uint32_t *d_table = nullptr;
    bool hung = false;                          // a wait timed out: the device is not touched again
    Slot slot[kSlots];
};

static bool hip_ok(hipError_t e, const char *what, std::string &err) {
    if (e == hipSuccess) return true;
    err = std::string("GPU SAM encode: ") + what + ": " + hipGetErrorString(e);
    return false;
}

// the slot's event against the deadline: DONE, FAILED (err), or TIMED_OUT (err; g->hung set)
static Wait wait_event(Gpu *g, Slot &s, std::string &err) {
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    for (;;) {
        const hipError_t e = hipEventQuery(s.done);
        if (e == hipSuccess) return DONE;
        if (e != hipErrorNotReady) {
            hip_ok(e, "kernel", err);
            return FAILED;
        }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > g->timeout_s) {
            g->hung = true;
            err = "GPU SAM encode: the device did not answer within " + std::to_string((int)g->timeout_s) + " s";
            return TIMED_OUT;
        }
        if (++spins < 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
        else std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

Gpu *gpu_open(int device, uint32_t max_lines, uint32_t max_text, double timeout_s, const std::vector<uint32_t> &table,
              std::string &err) {
    if (device < 0 || !max_lines || max_lines > kMaxLines || !max_text || max_text > kMaxText || table.size() < 2) {
        err = "GPU SAM encode: bad device, batch caps or table";
        return nullptr;
    }
    Gpu *g = new Gpu();
    g->device = device;
    g->max_lines = max_lines;
    g->max_text = max_text;
    g->table_bytes = (uint32_t)(table.size() * 4);
    g->out_cap = (size_t)FC2_SAM_ENC_BOUND(max_text, max_lines);
    g->timeout_s = timeout_s > 0 ? timeout_s : kDefaultTimeout;
    const size_t words = (size_t)max_lines + 1, meta = (2 * words + 2 * (size_t)max_lines + 1) * sizeof(uint32_t);
    bool ok = hip_ok(hipSetDevice(device), "hipSetDevice", err) &&
              hip_ok(hipMalloc((void **)&g->d_table, g->table_bytes), "device table", err) &&
              hip_ok(hipMemcpy(g->d_table, table.data(), g->table_bytes, hipMemcpyHostToDevice), "table upload", err);
    for (int k = 0; k < kSlots && ok; ++k) {
        Slot &s = g->slot[k];
        ok = hip_ok(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), "stream", err) &&
             hip_ok(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "event", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_text, max_text, hipHostMallocDefault), "pinned text", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_off, words * sizeof(uint32_t), hipHostMallocDefault), "pinned offsets", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_st, words * sizeof(uint32_t), hipHostMallocDefault), "pinned statuses", err) &&
             hip_ok(hipHostMalloc((void **)&s.h_out, g->out_cap, hipHostMallocDefault), "pinned output", err) &&
             hip_ok(hipMalloc((void **)&s.d_text, max_text), "device text", err) &&
             hip_ok(hipMalloc((void **)&s.d_out, g->out_cap), "device output", err) &&
             hip_ok(hipMalloc((void **)&s.d_meta, meta), "device tables", err);
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
            if (s.busy) {                       // (a batch nobody collected: bounded like every wait here)
                std::string err;
                if (wait_event(g, s, err) == TIMED_OUT) break;
                s.busy = false;
            }
        }
        if (!g->hung) {
            for (Slot &s : g->slot) {
                if (s.d_meta) (void)hipFree(s.d_meta);
                if (s.d_out) (void)hipFree(s.d_out);
                if (s.d_text) (void)hipFree(s.d_text);
                if (s.h_out) (void)hipHostFree(s.h_out);
                if (s.h_st) (void)hipHostFree(s.h_st);
                if (s.h_off) (void)hipHostFree(s.h_off);
                if (s.h_text) (void)hipHostFree(s.h_text);
                if (s.done) (void)hipEventDestroy(s.done);
                if (s.stream) (void)hipStreamDestroy(s.stream);
            }
            if (g->d_table) (void)hipFree(g->d_table);
        }
    }
    delete g;
}

bool gpu_hung(const Gpu *g) { return g->hung; }
char *gpu_text(Gpu *g, int k) { return g->slot[k].h_text; }
uint32_t *gpu_off(Gpu *g, int k) { return g->slot[k].h_off; }

bool gpu_submit(Gpu *g, int k, uint32_t n_lines, std::string &err) {
    if (g->hung || k < 0 || k >= kSlots || g->slot[k].busy || !n_lines || n_lines > g->max_lines) {
        err = "GPU SAM encode: no slot for the batch";
        return false;
    }
    Slot &s = g->slot[k];
    const uint32_t text_bytes = s.h_off[n_lines];
    if (s.h_off[0] != 0 || text_bytes > g->max_text) {
        err = "GPU SAM encode: the batch's text is out of range";
        return false;
    }
    if (!hip_ok(hipSetDevice(g->device), "hipSetDevice", err)) return false;
    const size_t words = (size_t)g->max_lines + 1;
    uint32_t *const d_off = s.d_meta, *const d_out_off = d_off + words, *const d_size = d_out_off + words,
                    *const d_total = d_size + g->max_lines, *const d_status = d_total + 1;
    s.n_lines = n_lines;
    s.h_st[0] = 0;
    // (whatever was queued on the stream before a failure still runs: from the first call on the slot counts
    // as busy, and a failure drains the stream before the slot's buffers can be used again)
    s.busy = true;
    const bool ok =
        (!text_bytes || hip_ok(hipMemcpyAsync(s.d_text, s.h_text, text_bytes, hipMemcpyHostToDevice, s.stream), "upload", err)) &&
        hip_ok(hipMemcpyAsync(d_off, s.h_off, ((size_t)n_lines + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s.stream), "upload", err) &&
        (fc2_sam_encode_launch(s.d_text, text_bytes, d_off, n_lines, g->d_table, g->table_bytes, s.d_out, g->out_cap, d_out_off,
                               d_size, d_status, d_total, s.stream) == FC2_OK ||
         ((err = "GPU SAM encode: the launch failed"), false)) &&
        hip_ok(hipMemcpyAsync(s.h_st, d_total, ((size_t)n_lines + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream), "download", err) &&
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

Wait gpu_collect(Gpu *g, int k, const uint32_t *&status, const uint8_t *&bytes, size_t &total, std::string &err) {
    status = nullptr;
    bytes = nullptr;
    total = 0;
    if (g->hung) {
        err = "GPU SAM encode: the device timed out earlier";
        return FAILED;
    }
    if (k < 0 || k >= kSlots || !g->slot[k].busy) {
        err = "GPU SAM encode: nothing to wait for";
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
        const size_t t = s.h_st[0];
        if (t > g->out_cap) {                   // (not what the kernels can write: the rule bounds it)
            err = "GPU SAM encode: a batch's size is out of range";
            w = FAILED;
        } else if (t) {
            // now that the batch's size is known: exactly that many bytes, on the same stream
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
            }
        }
        if (w == DONE) {
            status = s.h_st + 1;
            bytes = s.h_out;
            total = t;
        }
    }
    s.busy = false;
    return w;
}

}  // namespace samenc
}  // namespace fc2

// ---- any number of lines through the stage's slots ------------------------------------------------------

extern "C" uint64_t fc2_gpu_sam_encode_bound(uint64_t text_bytes, uint64_t n_lines) {
    return FC2_SAM_ENC_BOUND(text_bytes, n_lines);
}

extern "C" int fc2_gpu_sam_encode(int device, const void *text, const uint32_t *off, uint64_t n_lines, const char *const *names,
                                  uint32_t n_names, uint32_t batch_lines, void *out, uint64_t cap, uint64_t *out_n,
                                  uint32_t *status) {
    using namespace fc2;
    if (device < 0 || !off || (!text && n_lines && off[n_lines] > off[0]) || (!names && n_names) || !out || !out_n || !status ||
        batch_lines > kMaxLines)
        return fc2::fail(FC2_E_PARAM, "fc2_gpu_sam_encode: bad arguments (batch_lines is at most 16384)");
    *out_n = 0;
    if (!n_lines) return FC2_OK;
    for (uint64_t i = 0; i < n_lines; ++i)
        if (off[i] > off[i + 1]) return fc2::fail(FC2_E_PARAM, "fc2_gpu_sam_encode: the offsets must ascend");
    if (cap < FC2_SAM_ENC_BOUND((uint64_t)off[n_lines] - off[0], n_lines))
        return fc2::fail(FC2_E_RANGE, "fc2_gpu_sam_encode: cap below fc2_gpu_sam_encode_bound");
    if (!batch_lines) batch_lines = kMaxLines;
    std::vector<uint32_t> table = build_table(names, nullptr, n_names);
    std::string err;
    samenc::Gpu *g = samenc::gpu_open(device, batch_lines, kMaxText, 0, table, err);
    if (!g) return fc2::fail(FC2_E_HIP, "fc2_gpu_sam_encode: " + err);
    const char *src = static_cast<const char *>(text);
    uint8_t *o = static_cast<uint8_t *>(out);
    uint64_t at = 0;
    int rc = FC2_OK;
    // batch p goes into slot p % kSlots; before a slot is filled again, its batch (p - kSlots) is collected: the
    // records reach `out` in line order
    std::vector<std::pair<uint64_t, uint32_t>> flight;   // (first line, lines) of batches head .. next
    uint64_t head = 0, next = 0;
    auto collect = [&]() {
        const std::pair<uint64_t, uint32_t> b = flight[(size_t)head];
        const uint32_t *st = nullptr;
        const uint8_t *bytes = nullptr;
        size_t total = 0;
        const samenc::Wait w = samenc::gpu_collect(g, (int)(head % samenc::kSlots), st, bytes, total, err);
        ++head;
        if (w != samenc::DONE)
            return fc2::fail(w == samenc::TIMED_OUT ? FC2_E_IO : FC2_E_HIP, "fc2_gpu_sam_encode: " + err);
        if (total > cap - at) return fc2::fail(FC2_E_RANGE, "fc2_gpu_sam_encode: the output does not fit");
        memcpy(o + at, bytes, total);
        at += total;
        memcpy(status + b.first, st, (size_t)b.second * sizeof(uint32_t));
        return (int)FC2_OK;
    };
    uint64_t i = 0;
    while (i < n_lines && rc == FC2_OK) {
        if ((uint64_t)off[i + 1] - off[i] > kMaxText) {  // (no batch holds it: refused here, in its place)
            status[i++] = FC2_SAM_ENC_LONG;
            continue;
        }
        if (next - head == (uint64_t)samenc::kSlots) rc = collect();
        if (rc != FC2_OK) break;
        const int k = (int)(next % samenc::kSlots);
        char *bt = samenc::gpu_text(g, k);
        uint32_t *bo = samenc::gpu_off(g, k);
        uint32_t n = 0, bytes = 0;
        const uint64_t first = i;
        bo[0] = 0;
        while (i < n_lines && n < batch_lines) {
            const uint64_t len = (uint64_t)off[i + 1] - off[i];
            if (len > kMaxText - bytes) break;   // (a line over 4 MiB ends the batch too: the loop above takes it)
            if (len) memcpy(bt + bytes, src + off[i], (size_t)len);
            bytes += (uint32_t)len;
            bo[++n] = bytes;
            ++i;
        }
        flight.emplace_back(first, n);
        if (!samenc::gpu_submit(g, k, n, err)) rc = fc2::fail(FC2_E_HIP, "fc2_gpu_sam_encode: " + err);
        else ++next;
    }
    while (rc == FC2_OK && head < next) rc = collect();
    samenc::gpu_close(g);
    if (rc == FC2_OK) *out_n = at;
    return rc;
}
