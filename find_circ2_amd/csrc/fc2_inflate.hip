// fc2_inflate.hip -- BGZF blocks inflated on the GPU: the BAM input of the read loop
// (fc2_ingest.cpp bgzf_batch; the reference reads it through pysam/htslib, find_circ.py:461-469).
//
// A BGZF block (SAM/BAM spec 4.1) is a gzip member of at most 64 KiB holding at most 64 KiB of
// output, independent of every other block: one wavefront per block.  The DEFLATE stream (RFC 1951)
// is serial, so it is decoded wave-uniformly and kept in scalar registers: the payload is read 64
// words at a time, one word per lane (a refill is a v_readlane, the next 64 words already in flight),
// and every table entry read from LDS is made scalar (readfirstlane), so the decode's control flow is
// scalar branches.  The lanes work side by side where the work is parallel: building a Huffman
// code's tables (a ballot ranks the symbols of each length; each lane fills its own codes' entries),
// the bytes of a match (every source byte precedes the match -- p - dist + j mod dist -- so one
// iteration moves 64 bytes even for overlapping copies), stored blocks, and the stores to HBM.
// The output goes through a 16 KiB ring in LDS flushed to HBM 4 KiB at a time; a match reaching
// farther back (DEFLATE's window is 32 KiB) reads the stored output.  Fast tables of 9 and 7 bits
// (longer codes: the canonical test from there on) keep a workgroup at 20 KB of LDS: eight a CU,
// two waves a SIMD, one decoding while the other waits.  A table entry carries the symbol's
// meaning (literal / length or distance base and its extra-bit count / end of block), so a length
// or a distance is one lookup and one shift.  Every access is bounds-checked: a malformed block sets
// its status word, as does one whose CRC-32 or ISIZE the device finds wrong; the host inflates any
// block the GPU refused on the CPU, and checks CRC-32 and ISIZE only on the blocks it inflates itself.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fc2_ingest.h"
#include "fc2_bam_frag_impl.h"
#include "fc2_common.h"
#include "fc2_devcrc.h"
#include "fc2_inflate.h"

namespace {

constexpr uint32_t kOutMax = 65536;            // BGZF ISIZE limit
constexpr uint32_t kRing = 16384;              // the LDS ring: half DEFLATE's window (farther: HBM)
constexpr uint32_t kRingMask = kRing - 1;
constexpr uint32_t kFlush = 4096;              // ring -> HBM granule
constexpr int kLitBits = 9;                    // fast-table bits: literal/length code
constexpr int kDistBits = 7;                   // distance code, and the code-length code

enum : uint32_t { INF_OK = 0, INF_BAD_TYPE = 1, INF_BAD_STORED = 2, INF_BAD_COUNTS = 3, INF_BAD_CODE = 4,
                  INF_BAD_DIST = 5, INF_OVERFLOW = 6, INF_OVERRUN = 7, INF_SHORT = 8, INF_TOO_BIG = 9,
                  INF_BAD_CLCODE = 10, INF_BAD_CLSYM = 11, INF_BAD_REPEAT = 12, INF_NO_EOB = 13,
                  INF_BAD_LITCODE = 14, INF_BAD_DISTCODE = 15, INF_BAD_CRC = 16 };

// a table entry: codeword length (0: not in the fast table), extra-bit count, kind, value
enum : uint32_t { K_LIT = 0, K_LEN = 1, K_EOB = 2, K_BAD = 3 };
enum Table { T_LIT, T_DIST, T_CL };

__device__ __forceinline__ uint32_t entry(uint32_t len, uint32_t extra, uint32_t kind, uint32_t value) {
    return len | (extra << 4) | (kind << 8) | (value << 16);
}

struct Lds {                                   // 19968 B: eight workgroups a CU, two waves a SIMD
    uint8_t ring[kRing];
    uint32_t lfast[1 << kLitBits];
    uint32_t dfast[1 << kDistBits];            // (also the code-length code's table)
    uint32_t cnt[16];                          // codes per length, while a code is built
    uint16_t lsym[288], dsym[32];              // symbols in canonical order (codes past the fast tables)
    uint8_t lens[320];
};

__constant__ uint16_t kLBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59,
                                    67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t kLExt[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769,
                                    1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDExt[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11,
                                  12, 12, 13, 13};
__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// what symbol s of a table means (len: its codeword length)
__device__ __forceinline__ uint32_t meaning(Table t, uint32_t s, uint32_t len) {
    if (t == T_CL) return entry(len, 0, K_LIT, s);
    if (t == T_DIST) return s < 30 ? entry(len, kDExt[s], K_LEN, kDBase[s]) : entry(len, 0, K_BAD, 0);
    if (s < 256) return entry(len, 0, K_LIT, s);
    if (s == 256) return entry(len, 0, K_EOB, 0);
    return s < 286 ? entry(len, kLExt[s - 257], K_LEN, kLBase[s - 257]) : entry(len, 0, K_BAD, 0);
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the bit reader: wave-uniform, over a window of 64 payload words held one per lane (`win`: lane
// i holds word base + i) -- a refill is a v_readlane, not a dependent global load -- with the next
// window (`nxt`) loaded while this one is read.  `w` = the 32-bit words holding the block's payload,
// bit 0 of `pos` = bit 0 of w[0]; words past `last` read as 0 (no load past the payload)
struct Bits {
    const uint32_t *w;
    uint32_t pos, end;                         // bit positions
    uint64_t bb;                               // the bits at pos.. (nb of them)
    int nb;
    uint32_t wi;                               // next word to load into bb
    uint32_t base, last;                       // word index of lane 0's word in win; the last word
    uint32_t win, nxt;                         // this lane's word of the window, and of the next one
    int lane;
};

__device__ __forceinline__ uint32_t load_word(const Bits &b, uint32_t k) { return k <= b.last ? b.w[k] : 0u; }
__device__ __forceinline__ void window(Bits &b, uint32_t base) {
    b.base = base;
    b.win = load_word(b, base + (uint32_t)b.lane);
    b.nxt = load_word(b, base + 64u + (uint32_t)b.lane);
}
__device__ __forceinline__ uint32_t word(Bits &b, uint32_t k) {
    if (k - b.base >= 64u) {                   // (a k below base -- a seek back into bb -- reloads)
        if (k - b.base < 128u) {
            b.base += 64u;
            b.win = b.nxt;
            b.nxt = load_word(b, b.base + 64u + (uint32_t)b.lane);
        } else {
            window(b, k & ~63u);
        }
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)b.win, (int)(k - b.base));
}
__device__ __forceinline__ void seek(Bits &b, uint32_t bitpos) {
    b.pos = bitpos;
    b.wi = bitpos >> 5;
    const uint32_t sh = bitpos & 31u;
    const uint32_t lo = word(b, b.wi);
    const uint32_t hi = word(b, b.wi + 1);
    b.bb = ((uint64_t)lo | ((uint64_t)hi << 32)) >> sh;
    b.nb = 64 - (int)sh;
    b.wi += 2;
}
__device__ __forceinline__ uint32_t peek(Bits &b) {  // afterwards >= 33 valid bits
    if (b.nb <= 32) {
        b.bb |= (uint64_t)word(b, b.wi++) << b.nb;
        b.nb += 32;
    }
    return (uint32_t)b.bb;
}
__device__ __forceinline__ void drop(Bits &b, int n) {
    b.bb >>= n;
    b.nb -= n;
    b.pos += (uint32_t)n;
}
__device__ __forceinline__ uint32_t bits(Bits &b, int n) {  // n <= 16
    const uint32_t v = peek(b) & ((1u << n) - 1u);
    drop(b, n);
    return v;
}

// a canonical code's per-length numbers, lane l holding those of length l: the count, the first
// code (MSB-first) and the index in sym[] of the first symbol
struct CodeV {
    uint32_t cnt, first, index;
};

// the entry of the next symbol (0: no such code); consumes its codeword and extra bits and puts the
// decoded value (base + extra bits, or the literal / code-length symbol) into `val`.  A code longer
// than the fast table is found by the canonical test from length F + 1 on (RFC 1951 3.2.2)
template <int F>
__device__ __forceinline__ uint32_t decode(Bits &b, const uint32_t *fast, const CodeV &cv, const uint16_t *sym, Table t,
                                           uint32_t &val) {
    const uint32_t v = peek(b);
    uint32_t e = uni(fast[v & ((1u << F) - 1u)]);
    if (!(e & 15u)) {
        e = 0;
        const uint32_t rv = __builtin_bitreverse32(v);
        for (int l = F + 1; l <= 15; ++l) {
            const uint32_t code = rv >> (32 - l);
            const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)cv.first, l);
            if (code - f < (uint32_t)__builtin_amdgcn_readlane((int)cv.cnt, l)) {
                const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)cv.index, l) + code - f;
                e = meaning(t, uni(sym[k]), (uint32_t)l);
                break;
            }
        }
        if (!e) return 0;
    }
    const int cl = (int)(e & 15u), ex = (int)((e >> 4) & 15u);
    val = (e >> 16) + ((uint32_t)(b.bb >> cl) & ((1u << ex) - 1u));
    drop(b, cl + ex);
    return e;
}

// the canonical code of lens[0, n) (RFC 1951 3.2.2): the fast table's entries for codes of up to F
// bits (each lane fills its own symbols'), codes per length (cnt, and in cnt_v: lane l holds the
// count of length l), the symbols in canonical order (sym); false if over-subscribed, or incomplete
// other than by having no symbol at all or a single codeword of length 1 (what libdeflate accepts of
// every code and zlib of these two; a codeword such a code lacks is refused when it comes)
template <int F>
__device__ bool build(const uint8_t *lens, int n, uint32_t *fast, uint32_t *cnt, uint16_t *sym, Table t, int lane,
                      CodeV &cv) {
    if (lane < 16) cnt[lane] = 0;
    for (int i = lane; i < (1 << F); i += 64) fast[i] = 0;
    __syncthreads();
    for (int s = lane; s < n; s += 64) {
        const uint32_t l = lens[s];
        if (l) atomicAdd(&cnt[l], 1u);
    }
    __syncthreads();
    uint32_t cnt_v = lane < 16 ? cnt[lane] : 0u;
    cnt_v = lane == 0 ? 0u : cnt_v;
    cv.cnt = cnt_v;
    uint32_t start[16], next[16];              // scalar: the next sym[] slot and the next code per length
    int left = 1;
    uint32_t idx = 0, code = 0;
#pragma unroll
    for (int l = 1; l < 16; ++l) {
        const uint32_t nl = (uint32_t)__builtin_amdgcn_readlane((int)cnt_v, l);
        const uint32_t np = (uint32_t)__builtin_amdgcn_readlane((int)cnt_v, l - 1);
        left = (left << 1) - (int)nl;
        code = (code + np) << 1;               // RFC 1951 3.2.2 step 2
        start[l] = idx;
        next[l] = code;
        if (lane == l) {
            cv.first = code;
            cv.index = idx;
        }
        idx += nl;
    }
    const uint32_t n1 = (uint32_t)__builtin_amdgcn_readlane((int)cnt_v, 1);
    if (left < 0 || (left > 0 && idx > n1)) {  // over-subscribed (once negative, left only falls), or
        __syncthreads();                       // incomplete with more than the one 1-bit codeword
        return false;                          // (scalar: left, idx and n1 come from readlanes)
    }
    for (int base = 0; base < n; base += 64) {
        const int s = base + lane;
        const uint32_t l = s < n ? lens[s] : 0u;
#pragma unroll
        for (int ll = 1; ll < 16; ++ll) {
            const uint64_t m = __ballot(l == (uint32_t)ll);
            if (!m) continue;
            if (l == (uint32_t)ll) {
                const uint32_t r = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                sym[start[ll] + r] = (uint16_t)s;
                if (ll <= F) {
                    const uint32_t c = next[ll] + r;
                    const uint32_t rev = __builtin_bitreverse32(c) >> (32 - ll);
                    const uint32_t e = meaning(t, (uint32_t)s, (uint32_t)ll);
                    for (uint32_t k = rev; k < (1u << F); k += 1u << ll) fast[k] = e;
                }
            }
            const uint32_t c = (uint32_t)__popcll(m);
            start[ll] += c;
            next[ll] += c;
        }
    }
    __syncthreads();
    return true;
}

// ring bytes [flushed, upto) -> dst, in rows of 1024: whole 4 KiB granules, and with `all` the tail
// too (16 bytes a lane: the slot is 64 KiB, the bytes past isize are not read); every stored byte
// goes into the running raw CRC R
__device__ void flush(const Lds &L, uint8_t *dst, uint32_t &flushed, uint32_t upto, bool all, int lane, uint32_t &R) {
    __syncthreads();
    const uint32_t limit = all ? upto : flushed + (upto - flushed) / kFlush * kFlush;
    const uint32_t o = 16u * (uint32_t)lane;
    while (limit - flushed >= 1024u) {
        const uint4 v = *reinterpret_cast<const uint4 *>(L.ring + (flushed & kRingMask) + o);
        *reinterpret_cast<uint4 *>(dst + flushed + o) = v;
        const uint32_t c = crc_word(crc_word(crc_word(crc_word(0u, v.x), v.y), v.z), v.w);
        R = multmodp(kX2n[13], R) ^ wave_fold(c);   // x^8192: one row
        flushed += 1024u;
    }
    if (all && upto > flushed) {                  // the last row, t < 1024 bytes
        const uint32_t t = upto - flushed, r = flushed & kRingMask;
        if (o < t) *reinterpret_cast<uint4 *>(dst + flushed + o) = *reinterpret_cast<const uint4 *>(L.ring + r + o);
        for (uint32_t i = 0; i < t; ++i) {        // byte by byte, on every lane alike (once a block)
            R ^= uni(L.ring[r + i]);
#pragma unroll
            for (int b = 0; b < 8; ++b) R = mulx(R);
        }
        flushed = upto;
    }
    __threadfence_block();                     // the stored rows visible to the wave's far-match loads
}

// block i: payload src + off[i] (len[i] bytes of raw DEFLATE), output into dst + i * 64 KiB
// (isize[i] bytes) and checked against crc[i] (when crc is given), status[i] = INF_OK or the failure
__global__ __launch_bounds__(64) void inflate_kernel(const uint8_t *__restrict__ src, const uint32_t *__restrict__ off,
                                                     const uint32_t *__restrict__ len,
                                                     const uint32_t *__restrict__ isize,
                                                     const uint32_t *__restrict__ crc, uint8_t *__restrict__ dst,
                                                     uint32_t *__restrict__ status) {
    extern __shared__ __align__(16) uint8_t smem[];
    Lds &L = *reinterpret_cast<Lds *>(smem);
    const uint32_t blk = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const uint32_t o = off[blk], want = isize[blk];
    uint8_t *out = dst + (uint64_t)blk * kOutMax;
    uint32_t st = INF_OK;
    if (want > kOutMax || len[blk] >= (1u << 28)) st = INF_TOO_BIG;
    const uint32_t n = st == INF_OK ? len[blk] : 0u;   // (nothing is read of a refused block)
    Bits b;
    b.w = reinterpret_cast<const uint32_t *>(src + (o & ~3u));
    b.end = (o & 3u) * 8u + n * 8u;
    b.last = ((o & 3u) + n) >> 2;               // the word holding the first byte past the payload
    b.lane = lane;
    window(b, 0);
    seek(b, (o & 3u) * 8u);
    uint32_t p = 0, flushed = 0;                // output bytes so far; of them, stored to HBM
    uint32_t R = 0;                             // raw CRC of the stored bytes
    CodeV lcv = {0, 0, 0}, dcv = {0, 0, 0};
    bool last = false;
    while (st == INF_OK && !last) {
        if (b.pos + 3 > b.end) { st = INF_OVERRUN; break; }
        last = bits(b, 1) != 0;
        const uint32_t type = bits(b, 2);
        if (type == 0) {                        // stored: LEN, NLEN, then LEN bytes
            seek(b, (b.pos + 7u) & ~7u);
            if (b.pos + 32 > b.end) { st = INF_OVERRUN; break; }
            const uint32_t sl = bits(b, 16), nl = bits(b, 16);
            if (sl != (~nl & 0xFFFFu)) { st = INF_BAD_STORED; break; }
            if (b.pos + sl * 8u > b.end) { st = INF_OVERRUN; break; }
            if (p + sl > want) { st = INF_OVERFLOW; break; }
            const uint8_t *s = reinterpret_cast<const uint8_t *>(b.w) + (b.pos >> 3);
            for (uint32_t done = 0; done < sl;) {   // pieces of 4 KiB: the ring's unflushed bytes stay < 8 KiB
                const uint32_t k = min(sl - done, kFlush);
                for (uint32_t j = (uint32_t)lane; j < k; j += 64) L.ring[(p + j) & kRingMask] = s[done + j];
                p += k;
                done += k;
                if (p - flushed >= kFlush) flush(L, out, flushed, p, false, lane, R);
            }
            seek(b, b.pos + sl * 8u);
            continue;
        }
        if (type == 3) { st = INF_BAD_TYPE; break; }
        if (type == 1) {                        // fixed codes (RFC 1951 3.2.6)
            // (32 distance codes, so that the code is complete: meaning() marks 30 and 31 bad)
            for (int s = lane; s < 288 + 32; s += 64)
                L.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
            __syncthreads();
            if (!build<kLitBits>(L.lens, 288, L.lfast, L.cnt, L.lsym, T_LIT, lane, lcv) ||
                !build<kDistBits>(L.lens + 288, 32, L.dfast, L.cnt, L.dsym, T_DIST, lane, dcv)) {
                st = INF_BAD_LITCODE;
                break;
            }
        } else {                                // dynamic codes (3.2.7)
            if (b.pos + 14 > b.end) { st = INF_OVERRUN; break; }
            const int nlen = (int)bits(b, 5) + 257, ndist = (int)bits(b, 5) + 1, ncode = (int)bits(b, 4) + 4;
            if (nlen > 286 || ndist > 30) { st = INF_BAD_COUNTS; break; }
            if (lane < 19) L.lens[lane] = 0;
            __syncthreads();
            for (int k = 0; k < ncode; ++k) {   // the code-length code's lengths, 3 bits each
                const uint32_t v = bits(b, 3);
                if (lane == 0) L.lens[kClOrder[k]] = (uint8_t)v;
            }
            __syncthreads();
            if (!build<7>(L.lens, 19, L.dfast, L.cnt, L.dsym, T_CL, lane, dcv)) { st = INF_BAD_CLCODE; break; }
            const int total = nlen + ndist;
            int k = 0;
            while (k < total) {
                if (b.pos > b.end) { st = INF_OVERRUN; break; }
                uint32_t sym;
                if (!decode<7>(b, L.dfast, dcv, L.dsym, T_CL, sym)) { st = INF_BAD_CLSYM; break; }
                if (sym < 16) {
                    if (lane == 0) L.lens[k] = (uint8_t)sym;
                    ++k;
                    continue;
                }
                uint32_t val = 0;
                int rep;
                if (sym == 16) {
                    if (k == 0) { st = INF_BAD_REPEAT; break; }
                    __syncthreads();
                    val = uni(L.lens[k - 1]);
                    rep = 3 + (int)bits(b, 2);
                } else if (sym == 17) {
                    rep = 3 + (int)bits(b, 3);
                } else {
                    rep = 11 + (int)bits(b, 7);
                }
                if (k + rep > total) { st = INF_BAD_REPEAT; break; }
                for (int r = lane; r < rep; r += 64) L.lens[k + r] = (uint8_t)val;
                k += rep;
            }
            if (st != INF_OK) break;
            if (b.pos > b.end) { st = INF_OVERRUN; break; }
            __syncthreads();
            if (uni(L.lens[256]) == 0) { st = INF_NO_EOB; break; }
            if (!build<kLitBits>(L.lens, nlen, L.lfast, L.cnt, L.lsym, T_LIT, lane, lcv)) {
                st = INF_BAD_LITCODE;
                break;
            }
            if (!build<kDistBits>(L.lens + nlen, ndist, L.dfast, L.cnt, L.dsym, T_DIST, lane, dcv)) {
                st = INF_BAD_DISTCODE;
                break;
            }
        }
        // the compressed data of this block
        for (;;) {
            if (b.pos > b.end) { st = INF_OVERRUN; break; }
            uint32_t val;
            const uint32_t e = decode<kLitBits>(b, L.lfast, lcv, L.lsym, T_LIT, val);
            const uint32_t kind = (e >> 8) & 0xFFu;
            if (!e || kind == K_BAD) { st = INF_BAD_CODE; break; }
            if (kind == K_LIT) {
                if (p >= want) { st = INF_OVERFLOW; break; }
                if (lane == 0) L.ring[p & kRingMask] = (uint8_t)val;
                ++p;
            } else if (kind == K_EOB) {
                break;
            } else {
                const uint32_t mlen = val;
                uint32_t dist;
                const uint32_t de = decode<kDistBits>(b, L.dfast, dcv, L.dsym, T_DIST, dist);
                if (!de || ((de >> 8) & 0xFFu) == K_BAD || dist > p) { st = INF_BAD_DIST; break; }
                if (p + mlen > want) { st = INF_OVERFLOW; break; }
                // every source byte precedes p: one iteration moves 64 bytes, overlapping copies too.
                // A source the ring no longer holds (dist + mlen > 16 KiB: it is more than 16 KiB
                // - 258 back, past the unflushed 4 KiB + 258) is read from the stored output
                if (dist + mlen <= kRing) {
                    for (uint32_t j = (uint32_t)lane; j < mlen; j += 64)
                        L.ring[(p + j) & kRingMask] = L.ring[(p - dist + (j < dist ? j : j % dist)) & kRingMask];
                } else {
                    for (uint32_t j = (uint32_t)lane; j < mlen; j += 64)
                        L.ring[(p + j) & kRingMask] = out[p - dist + (j < dist ? j : j % dist)];
                }
                p += mlen;
            }
            if (p - flushed >= kFlush) flush(L, out, flushed, p, false, lane, R);
        }
    }
    if (st == INF_OK && p != want) st = INF_SHORT;
    if (st == INF_OK && b.pos > b.end) st = INF_OVERRUN;
    if (st == INF_OK) {
        flush(L, out, flushed, p, true, lane, R);
        if (crc && (R ^ multmodp(x8n(want), 0xFFFFFFFFu) ^ 0xFFFFFFFFu) != crc[blk]) st = INF_BAD_CRC;
    }
    if (lane == 0) status[blk] = st;
}

// block i's bytes (slot i of `slots`, isize[i] of them) to out + ooff[i], for the blocks inflated
// (status 0): 16 bytes a thread, whole uint4 stores where the destination is aligned
__global__ __launch_bounds__(256) void compact_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ isize,
                                                      const uint32_t *__restrict__ ooff,
                                                      const uint32_t *__restrict__ status, uint8_t *__restrict__ out) {
    const uint32_t blk = blockIdx.y;
    const uint32_t b0 = 16u * (blockIdx.x * 256u + threadIdx.x);
    const uint32_t n = isize[blk];
    if (status[blk] != INF_OK || b0 >= n) return;
    const uint4 v = *reinterpret_cast<const uint4 *>(slots + (uint64_t)blk * kOutMax + b0);
    uint8_t *d = out + ooff[blk] + b0;
    if (b0 + 16u <= n && ((uintptr_t)d & 15u) == 0) {
        *reinterpret_cast<uint4 *>(d) = v;
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t k = min(16u, n - b0);
    for (uint32_t i = 0; i < k; ++i) d[i] = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
}

// ---- the BAM record starts of the inflated blocks (fc2_ingest.cpp walk_block, on the device) ------
// One wavefront per block, reading the block where the inflate kernel left it: its slot, in L2 or
// HBM, no LDS (the chain of block sizes is ~250 dependent loads a block, and a chunk's 256 wavefronts
// wait for them side by side; staging 64 KiB a block in LDS would leave room for two of these
// workgroups a CU and none for the inflate kernel's eight).  Every read is below min(isize, 64 KiB)
// of the block's own slot and every write inside its own output row, whatever the bytes say.

constexpr uint32_t kWalkCap = FC2_BAM_WALK_CAP;
static_assert((kOutMax - 4) / 36 + 1 <= kWalkCap, "a block's record starts fit a row");

// the little-endian 32-bit field at byte o of the slot (w: its words), from aligned words, so a
// record start at any byte residue reads the same way; o + 4 <= 64 KiB
__device__ __forceinline__ uint32_t walk_u32(const uint32_t *__restrict__ w, uint32_t o) {
    const uint32_t i = o >> 2, s = (o & 3u) * 8u;
    const uint32_t lo = w[i];
    if (!s) return lo;
    return (lo >> s) | (w[i + 1] << (32u - s));
}

// bam_plausible (fc2_ingest.cpp) at byte o of a block of n bytes
__device__ bool walk_plausible(const uint32_t *__restrict__ w, uint32_t o, uint32_t n) {
    if (o > n || n - o < 36u) return false;
    const uint32_t avail = n - o;
    const int32_t bs = (int32_t)walk_u32(w, o);
    if (bs < 32 || bs >= (1 << 28)) return false;
    const int32_t ref = (int32_t)walk_u32(w, o + 4), pos = (int32_t)walk_u32(w, o + 8);
    const uint32_t lname = walk_u32(w, o + 12) & 0xFFu, ncig = walk_u32(w, o + 16) & 0xFFFFu;
    const int32_t lseq = (int32_t)walk_u32(w, o + 20), nref = (int32_t)walk_u32(w, o + 24),
                  npos = (int32_t)walk_u32(w, o + 28);
    if (ref < -1 || pos < -1 || lname < 1 || lseq < 0 || nref < -1 || npos < -1) return false;
    if (32ull + lname + 4ull * ncig + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > (uint64_t)bs) return false;
    if (36u + lname > avail) return true;
    const uint8_t *p = reinterpret_cast<const uint8_t *>(w) + o + 36u;     // lname bytes, all below n
    if (p[lname - 1] != 0) return false;
    for (uint32_t k = 0; k + 1 < lname; ++k)
        if (p[k] < 0x21 || p[k] > 0x7e) return false;
    return true;
}

__global__ __launch_bounds__(64) void bam_walk_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ isize,
                                                      const uint32_t *__restrict__ status, uint16_t *__restrict__ starts,
                                                      uint32_t *__restrict__ count, uint32_t *__restrict__ exit_at) {
    const uint32_t blk = blockIdx.x, lane = threadIdx.x;
    if (status && status[blk] != INF_OK) {      // not inflated: the host walks it once the CPU has
        if (lane == 0) count[blk] = 0, exit_at[blk] = FC2_BAM_WALK_NO_EXIT;
        return;
    }
    const uint32_t n = min(isize[blk], kOutMax);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(slots + (uint64_t)blk * kOutMax);
    uint16_t *row = starts + (uint64_t)blk * kWalkCap;
    // the first plausible record followed by a plausible one (or by the block's end): 64 offsets a
    // step, the lowest lane that holds wins; at most n / 64 steps
    uint32_t o = FC2_BAM_WALK_NO_EXIT;
    for (uint32_t b = 0; b + 36u <= n; b += 64u) {
        const uint32_t c = b + lane;
        bool ok = walk_plausible(w, c, n);
        if (ok) {
            const uint32_t nx = c + 4u + walk_u32(w, c);                    // (block_size < 2^28)
            ok = nx + 36u > n || walk_plausible(w, nx, n);
        }
        const unsigned long long m = __ballot(ok);
        if (m) {
            o = b + (uint32_t)__ffsll(m) - 1u;
            break;
        }
    }
    o = uni(o);
    uint32_t cnt = 0, ex = FC2_BAM_WALK_NO_EXIT;
    if (o != FC2_BAM_WALK_NO_EXIT) {
        // block_size to block_size: every step advances at least 36 bytes, so at most kWalkCap steps
        // (o stays below 64 KiB + 4 + 2^31: no overflow)
        bool cut = false;
        while (cnt < kWalkCap && o + 4u <= n) {
            const int32_t bs = (int32_t)uni(walk_u32(w, o));
            if (bs < 32) { cut = true; break; }
            if (lane == 0) row[cnt] = (uint16_t)o;
            ++cnt;
            o += 4u + (uint32_t)bs;
        }
        if (!cut) ex = o;
    }
    if (lane == 0) count[blk] = cnt, exit_at[blk] = ex;
}

// ---- the record digest: parse_bam_body's derived fields (fc2_ingest.cpp), on the device ------------
// One wavefront per BGZF block, no LDS (it runs beside the inflate kernel's eight 20 KB workgroups a
// CU); the lanes stride over the block's listed record starts, one record a lane.  A record is read
// from the chunk's contiguous stream, not from the slots: it may run on through the following blocks.
// The lanes' records differ in their CIGAR and tag counts, so the loops diverge, and a lane's loads
// are its own (a record's bytes share cache lines with the neighbouring lanes' records: L2 takes the
// re-reads); fields are composed from byte loads, since a record starts at any byte residue and the
// stream itself at any address.
//
// Bounds.  Loads: dg_u8 / dg_u16 / dg_u32 are only called with offsets the caller has shown to be
// below `lim`, the record's own end (at + 4 + block_size), after lim <= n_bytes was checked -- the
// block_size itself after at + 4 <= n_bytes -- so every load is inside [bytes, bytes + n_bytes)
// whatever the bytes say.  Loops: the CIGAR loop runs n_cigar_op <= 65535 times over words the field
// check placed below lim; the tag loop advances at least 4 bytes a turn and the Z / H scan one byte a
// turn, both towards lim <= n_bytes; the status loop visits each block once.  Stores: lane k of block
// blk writes rows[first[blk] + k] with k < min(count[blk], cap), below first[blk + 1] <= first[n_blocks],
// the launch's counted rows; first[blk] (and first[n_blocks], by the last block) by lane 0.

constexpr uint32_t kDigestMaxBlocks = FC2_BAM_DIGEST_MAX_BLOCKS;
static_assert(sizeof(fc2_bam_digest) == 32, "a digest row is 32 bytes");

__device__ __forceinline__ uint32_t dg_u8(const uint8_t *__restrict__ b, uint64_t o) { return b[o]; }
__device__ __forceinline__ uint32_t dg_u16(const uint8_t *__restrict__ b, uint64_t o) {
    return dg_u8(b, o) | (dg_u8(b, o + 1) << 8);
}
__device__ __forceinline__ uint32_t dg_u32(const uint8_t *__restrict__ b, uint64_t o) {
    return dg_u8(b, o) | (dg_u8(b, o + 1) << 8) | (dg_u8(b, o + 2) << 16) | (dg_u8(b, o + 3) << 24);
}

// an AS / XS value's bytes as its type says (the tag walk has checked that they lie below lim)
__device__ __forceinline__ uint32_t dg_tag_bits(const uint8_t *__restrict__ b, uint64_t p, uint32_t ty) {
    switch (ty) {
        case 'c': return (uint32_t)(int32_t)(int8_t)dg_u8(b, p);
        case 'C': return dg_u8(b, p);
        case 's': return (uint32_t)(int32_t)(int16_t)dg_u16(b, p);
        case 'S': return dg_u16(b, p);
        case 'i': case 'I': case 'f': return dg_u32(b, p);
        default: return 0;                      // A Z H B
    }
}

// the row of the record start at byte `at` of the stream; false: state 0 (r.block_size may be set)
__device__ bool digest_record(const uint8_t *__restrict__ bytes, uint32_t n_bytes, uint64_t at,
                              const uint32_t *__restrict__ ooff, const uint32_t *__restrict__ status, uint32_t blk,
                              uint32_t n_blocks, fc2_bam_digest &r) {
    if (at + 4 > n_bytes) return false;
    const uint32_t bs = dg_u32(bytes, at);
    r.block_size = bs;
    if (bs < 32u || bs >= (1u << 28)) return false;
    const uint64_t b = at + 4, lim = b + bs;    // the record's body: [b, lim)
    if (lim > n_bytes) return false;
    if (status)                                 // every block it touches was inflated on the device
        for (uint32_t j = blk; j < n_blocks && (j == blk || ooff[j] < lim); ++j)
            if (status[j] != INF_OK) return false;
    const int64_t pos = (int32_t)dg_u32(bytes, b + 4);
    const uint32_t l_name = dg_u8(bytes, b + 8), n_cig = dg_u16(bytes, b + 12), flag = dg_u16(bytes, b + 14);
    const int64_t l_seq = (int32_t)dg_u32(bytes, b + 16);
    if (l_seq < 0 || 32 + (int64_t)l_name + 4 * (int64_t)n_cig + (l_seq + 1) / 2 + l_seq > (int64_t)bs) return false;
    if (l_name == 0 || dg_u8(bytes, b + 32 + l_name - 1) != 0) return false;
    // cigar_info: the reference span, the clips before the first M, the soft clips at both ends
    uint64_t p = b + 32 + l_name;
    uint64_t ref_span = 0, astart = 0, lead = 0, trail = 0;
    bool stop = false, leading = true;
    for (uint32_t k = 0; k < n_cig; ++k, p += 4) {
        const uint32_t c = dg_u32(bytes, p), op = c & 0xFu, len = c >> 4;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_span += len;
        if (!stop) {
            if (op == 4 || op == 5) astart += len;
            else if (op == 0) stop = true;
        }
        if (leading) {
            if (op == 4) lead += len;
            else if (op != 5) leading = false;
        }
        if (op == 4) trail += len;              // (the soft clips of the trailing run of S / H)
        else if (op != 5) trail = 0;
    }
    if ((ref_span | astart | lead | trail) >> 31) return false;
    r.astart = (int32_t)astart;
    r.aend = ((flag & 4u) || n_cig == 0) ? -1 : pos + (int64_t)ref_span;
    // finish_rec: len(seq[lead : len(seq) - trail]) with Python's slice semantics
    if (l_seq > 0) {
        const int64_t n = l_seq;
        int64_t s0 = (int64_t)lead, e0 = n - (int64_t)trail;
        if (e0 < 0) e0 += n;
        s0 = s0 > n ? n : s0;
        e0 = e0 < 0 ? 0 : (e0 > n ? n : e0);
        r.qlen = (int32_t)(e0 > s0 ? e0 - s0 : 0);
        r.has_qual = dg_u8(bytes, p + (uint64_t)(l_seq + 1) / 2) != 0xFFu;
    } else {
        r.qlen = -1;
        r.has_qual = 0;
    }
    p += (uint64_t)(l_seq + 1) / 2 + (uint64_t)l_seq;
    // scan_bam_tags / aux_value_size over [p, lim)
    uint32_t n_as = 0, n_xs = 0;
    while (p < lim) {
        if (lim - p < 3) return false;
        const uint32_t t0 = dg_u8(bytes, p), t1 = dg_u8(bytes, p + 1), ty = dg_u8(bytes, p + 2);
        p += 3;
        const uint64_t left = lim - p;
        uint64_t n;
        switch (ty) {
            case 'c': case 'C': case 'A': n = 1; break;
            case 's': case 'S': n = 2; break;
            case 'i': case 'I': case 'f': n = 4; break;
            case 'Z': case 'H': {
                uint64_t z = p;
                while (z < lim && dg_u8(bytes, z) != 0) ++z;
                if (z == lim) return false;
                n = z - p + 1;
                break;
            }
            case 'B': {
                if (left < 5) return false;
                const uint32_t sub = dg_u8(bytes, p);
                const uint32_t w = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u
                                 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
                const int32_t cnt = (int32_t)dg_u32(bytes, p + 1);
                if (!w || cnt < 0) return false;
                n = 5 + (uint64_t)w * (uint32_t)cnt;
                break;
            }
            default: return false;
        }
        if (n > left) return false;
        const bool as = t0 == 'A' && t1 == 'S', xs = t0 == 'X' && t1 == 'S';
        if (as) {
            if (n_as++) return false;           // first and last would differ: the host's logic
            r.as_type = (uint8_t)ty;
            r.as_bits = dg_tag_bits(bytes, p, ty);
        }
        if (xs) {
            if (n_xs++) return false;
            r.xs_type = (uint8_t)ty;
            r.xs_bits = dg_tag_bits(bytes, p, ty);
        }
        p += n;
    }
    return true;
}

__global__ __launch_bounds__(64) void bam_digest_kernel(const uint8_t *__restrict__ bytes, uint32_t n_bytes,
                                                        const uint32_t *__restrict__ ooff, const uint32_t *__restrict__ status,
                                                        const uint16_t *__restrict__ starts, const uint32_t *__restrict__ count,
                                                        fc2_bam_digest *__restrict__ rows, uint32_t *__restrict__ first,
                                                        uint32_t n_blocks) {
    const uint32_t blk = blockIdx.x, lane = threadIdx.x;
    // first[blk]: the rows of the blocks before this one, summed across the wave (n_blocks <= 1024:
    // at most 16 counts a lane)
    uint32_t f = 0;
    for (uint32_t j = lane; j < blk; j += 64u) f += min(count[j], kWalkCap);
    for (int d = 32; d; d >>= 1) f += __shfl_xor(f, d, 64);
    const uint32_t cnt = min(count[blk], kWalkCap);
    if (lane == 0) {
        first[blk] = f;
        if (blk + 1 == n_blocks) first[n_blocks] = f + cnt;
    }
    const uint16_t *row = starts + (uint64_t)blk * kWalkCap;
    const uint32_t o0 = ooff[blk];
    for (uint32_t k = lane; k < cnt; k += 64u) {
        fc2_bam_digest r;
        r.state = r.as_type = r.xs_type = r.has_qual = 0;
        r.block_size = 0;
        r.astart = r.qlen = 0;
        r.as_bits = r.xs_bits = 0;
        r.aend = 0;
        if (digest_record(bytes, n_bytes, (uint64_t)o0 + row[k], ooff, status, blk, n_blocks, r)) {
            r.state = 1;
        } else {                                // the host parses it: block_size and zeros
            const uint32_t bs = r.block_size;
            r.as_type = r.xs_type = r.has_qual = 0;
            r.astart = r.qlen = 0;
            r.as_bits = r.xs_bits = 0;
            r.aend = 0;
            r.block_size = bs;
        }
        rows[(uint64_t)f + k] = r;
    }
}

// ---- the fragment rows: unspliced fragments closed on the device (fc2_bam_frag_impl.h) -------------
// The digest kernel's shape: one wavefront per BGZF block, no LDS, no wait on another workgroup (the
// digest rows it reads were written by the launch before it on the stream); the lanes stride over the
// block's listed starts, one head a lane.  A fragment crosses blocks, so the records are read from the
// chunk's contiguous bytes and the neighbouring records' digest rows are reached through a (block, k)
// cursor over count[] / starts[] / first[].  The lanes' walks differ in length and their loads are
// their own; fields are composed from byte loads (a record starts at any byte residue).
//
// Bounds.  Loads: a record is read only after frag_load has found its digest row in state 1 and shown
// its end -- at + 4 + the row's block_size -- to be at most n_bytes and its name to lie inside it; the
// fixed fields and the name bytes are below that end, so every load is inside [bytes, bytes + n_bytes)
// whatever bytes and rows hold.  starts / count / first / ooff are read at block indices below n_blocks
// and start indices below min(count, cap); digest rows below first[j] + min(count[j], cap) <=
// first[n_blocks].  Loops: the back walk takes at most 5 steps, the forward walk at most
// FC2_BAM_FRAG_CAP + 1; a step's cursor visits each block and each of a block's starts at most once.
// Stores: lane k of block i writes only frag_rows[first[i] + k], k < min(count[i], cap).

static_assert(sizeof(fc2_bam_frag) == 8, "a fragment row is 8 bytes");

__global__ __launch_bounds__(64) void bam_frag_kernel(const uint8_t *__restrict__ bytes, uint32_t n_bytes,
                                                      const uint32_t *__restrict__ ooff, const uint16_t *__restrict__ starts,
                                                      const uint32_t *__restrict__ count,
                                                      const fc2_bam_digest *__restrict__ rows,
                                                      const uint32_t *__restrict__ first, fc2_bam_frag *__restrict__ frag_rows,
                                                      uint32_t n_blocks) {
    const uint32_t blk = blockIdx.x, lane = threadIdx.x;
    const fc2::frag::Tables T{bytes, n_bytes, ooff, starts, count, rows, first, n_blocks};
    const uint32_t cnt = min(count[blk], kWalkCap);
    const uint64_t f = first[blk];
    for (uint32_t k = lane; k < cnt; k += 64u) frag_rows[f + k] = fc2::frag::frag_row(T, blk, k);
}

}  // namespace

// C ABI (include/fc2_ingest.h): the fragment rows of the record starts listed for n_blocks blocks
extern "C" int fc2_bam_frag_launch(const uint8_t *bytes, uint32_t n_bytes, const uint32_t *ooff, const uint32_t *isize,
                                   const uint32_t *status, const uint16_t *starts, const uint32_t *count,
                                   const fc2_bam_digest *rows, const uint32_t *first, fc2_bam_frag *frag_rows,
                                   uint32_t n_blocks, void *stream) {
    (void)isize, (void)status;                  // (the digest rows have taken both into account)
    if (!n_blocks) return FC2_OK;
    if ((!bytes && n_bytes) || !ooff || !starts || !count || !rows || !first || !frag_rows)
        return fc2::fail(FC2_E_PARAM, "fc2_bam_frag_launch: null argument");
    if (n_blocks > kDigestMaxBlocks) return fc2::fail(FC2_E_PARAM, "fc2_bam_frag_launch: more than 1024 blocks");
    if (((uintptr_t)rows & 7u) || ((uintptr_t)frag_rows & 7u) || ((uintptr_t)first & 3u))
        return fc2::fail(FC2_E_PARAM, "fc2_bam_frag_launch: rows must be 8-byte and first 4-byte aligned");
    hipLaunchKernelGGL(bam_frag_kernel, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream, bytes, n_bytes, ooff, starts, count,
                       rows, first, frag_rows, n_blocks);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_bam_frag_launch: ") + hipGetErrorString(e));
}

// C ABI (include/fc2_ingest.h): the digest rows of the record starts listed for n_blocks blocks
extern "C" int fc2_bam_digest_launch(const uint8_t *bytes, uint32_t n_bytes, const uint32_t *ooff, const uint32_t *isize,
                                     const uint32_t *status, const uint16_t *starts, const uint32_t *count,
                                     fc2_bam_digest *rows, uint32_t *first, uint32_t n_blocks, void *stream) {
    if (!n_blocks) return FC2_OK;
    if ((!bytes && n_bytes) || !ooff || !isize || !starts || !count || !rows || !first)
        return fc2::fail(FC2_E_PARAM, "fc2_bam_digest_launch: null argument");
    if (n_blocks > kDigestMaxBlocks) return fc2::fail(FC2_E_PARAM, "fc2_bam_digest_launch: more than 1024 blocks");
    if (((uintptr_t)rows & 7u) || ((uintptr_t)first & 3u))
        return fc2::fail(FC2_E_PARAM, "fc2_bam_digest_launch: rows must be 8-byte and first 4-byte aligned");
    hipLaunchKernelGGL(bam_digest_kernel, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream, bytes, n_bytes, ooff, status,
                       starts, count, rows, first, n_blocks);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_bam_digest_launch: ") + hipGetErrorString(e));
}

// C ABI (include/fc2_ingest.h): the record starts of n_blocks inflated blocks
extern "C" int fc2_bam_walk_launch(const uint8_t *slots, const uint32_t *isize, const uint32_t *status, uint16_t *starts,
                                   uint32_t *count, uint32_t *exit, uint32_t n_blocks, void *stream) {
    if (!n_blocks) return FC2_OK;
    if (!slots || !isize || !starts || !count || !exit) return fc2::fail(FC2_E_PARAM, "fc2_bam_walk_launch: null argument");
    if ((uintptr_t)slots & 3u) return fc2::fail(FC2_E_PARAM, "fc2_bam_walk_launch: slots must be 4-byte aligned");
    hipLaunchKernelGGL(bam_walk_kernel, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream, slots, isize, status, starts,
                       count, exit);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_bam_walk_launch: ") + hipGetErrorString(e));
}

// C ABI (include/fc2_ingest.h): n blocks; src must be readable 8 bytes past every payload
extern "C" int fc2_bgzf_inflate_launch(const uint8_t *src, const uint32_t *off, const uint32_t *len,
                                       const uint32_t *isize, const uint32_t *crc, uint8_t *dst, uint32_t *status,
                                       uint32_t n, void *stream) {
    if (!n) return FC2_OK;
    if (!src || !off || !len || !isize || !dst || !status) return fc2::fail(FC2_E_PARAM, "fc2_bgzf_inflate_launch: null argument");
    static bool attr = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(inflate_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Lds)) == hipSuccess;
    }();
    if (!attr) return fc2::fail(FC2_E_HIP, "fc2_bgzf_inflate_launch: cannot reserve the kernel's LDS");
    hipLaunchKernelGGL(inflate_kernel, dim3(n), dim3(64), sizeof(Lds), (hipStream_t)stream, src, off, len, isize, crc,
                       dst, status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_bgzf_inflate_launch: ") + hipGetErrorString(e));
}

// ---- host side: the ingest's batches (fc2_inflate.h) -------------------------------------------
namespace fc2 {
namespace inf {

// the pinned pool: batch buffers the inflated bytes are downloaded into directly (fc2_ingest.cpp's
// batch allocator asks for them), made on first use, kept while a Gpu is open
namespace {
struct Pool {
    struct Buf {
        void *p;
        size_t size;
    };
    std::mutex mu;
    size_t cap = 0;                            // bytes of a new buffer: the largest asked of the pool
    int users = 0, max_buffers = 0;
    std::vector<Buf> idle, all;                // (a buffer keeps the size it was made with)
};
Pool &pool() {
    static Pool *p = new Pool();               // (never destroyed: outlives the static destructors)
    return *p;
}
std::atomic<bool> pool_on{false};

void pool_open(size_t cap, int max_buffers) {
    Pool &P = pool();
    std::lock_guard<std::mutex> g(P.mu);
    ++P.users;
    P.cap = std::max(P.cap, cap);
    P.max_buffers = std::max(P.max_buffers, max_buffers);
    pool_on = true;
}
void pool_drop(Pool &P, void *b) {             // (P.mu held)
    (void)hipHostFree(b);
    for (size_t k = 0; k < P.all.size(); ++k)
        if (P.all[k].p == b) {
            P.all.erase(P.all.begin() + (ptrdiff_t)k);
            break;
        }
}
void pool_close() {
    Pool &P = pool();
    std::lock_guard<std::mutex> g(P.mu);
    if (--P.users > 0) return;
    pool_on = false;
    for (const Pool::Buf &b : P.idle) pool_drop(P, b.p);
    P.idle.clear();                            // (buffers still in use are freed when given back)
    P.cap = 0;
    P.max_buffers = 0;
}
}  // namespace

void *pinned_take(size_t n) {
    if (!pool_on.load(std::memory_order_relaxed)) return nullptr;
    Pool &P = pool();
    std::lock_guard<std::mutex> g(P.mu);
    if (!P.users || n > P.cap) return nullptr;
    for (size_t k = 0; k < P.idle.size(); ++k)
        if (P.idle[k].size >= n) {
            void *b = P.idle[k].p;
            P.idle.erase(P.idle.begin() + (ptrdiff_t)k);
            return b;
        }
    if ((int)P.all.size() >= P.max_buffers) return nullptr;
    void *b = nullptr;
    if (hipHostMalloc(&b, P.cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    P.all.push_back({b, P.cap});
    return b;
}

bool pinned_owns(const void *b) {
    Pool &P = pool();
    std::lock_guard<std::mutex> g(P.mu);
    for (const Pool::Buf &x : P.all)
        if (x.p == b) return true;
    return false;
}

bool pinned_give(void *b) {
    Pool &P = pool();
    std::lock_guard<std::mutex> g(P.mu);
    for (const Pool::Buf &x : P.all)
        if (x.p == b) {
            if (P.users) P.idle.push_back(x);
            else pool_drop(P, b);
            return true;
        }
    return false;
}

// chunks of a batch in flight at once: four chunks of 256 blocks hold half the GPU's 2048 wave slots
// for this kernel (eight 20 KB workgroups a CU), so the breakpoint search's kernels find room
constexpr int kStreams = 4;

// the blocks' table by column, M entries each in one allocation: the payload's offset in the input
// and its length, ISIZE, CRC-32, the output offset in the batch, the device's status, and the output
// offset in the block's chunk (the digest kernel's)
struct Cols {
    uint32_t *off, *len, *isize, *crc, *ooff, *status, *rooff;
    static constexpr size_t kCount = 7;
    static Cols of(uint32_t *b, size_t M) { return {b, b + M, b + 2 * M, b + 3 * M, b + 4 * M, b + 5 * M, b + 6 * M}; }
};
struct WalkCols {                              // a block's listed record starts: how many, and the walk's exit
    uint32_t *count, *exit;
    static constexpr size_t kCount = 2;
    static WalkCols of(uint32_t *b, size_t M) { return {b, b + M}; }
};
// blocks [i0, i0 + c) of the batch under way: input bytes [b0, b1), output bytes [o0, o1), on stream s;
// a digested chunk's first[] lies at foff of d_first / h_first, its first row at row0 of h_rows
struct Chunk {
    uint32_t i0, c;
    size_t b0, b1;
    uint64_t o0, o1, row0;
    uint32_t foff;
    int s;
};

struct Gpu {
    int device = 0;
    uint32_t max_blocks = 0;
    size_t src_cap = 0;
    hipStream_t stream[kStreams] = {};
    hipEvent_t done[kStreams] = {};            // blocking-sync: the reader thread sleeps, not spins
    std::vector<std::pair<void *, bool>> bufs; // every buffer below and whether it is pinned (make): gpu_close frees them
    uint8_t *h_src = nullptr, *d_src = nullptr, *d_slots = nullptr, *d_out = nullptr;
    Cols h{}, d{};                             // the blocks' table, pinned and on the device
    // the blocks' record lists (bam_walk_kernel): count | exit, and a row of starts per block
    WalkCols h_walk{}, d_walk{};
    uint16_t *h_starts = nullptr, *d_starts = nullptr;
    bool walk = false;                         // this batch's blocks are listed on the device
    // the listed records' digest rows (bam_digest_kernel), made by the first batch that asks for them:
    // a chunk's rows lie dense from row i0 * kWalkCap of d_rows on, its first[] (c + 1 entries) at
    // d_first + i0 + its index among the batch's chunks; gpu_finish downloads the counted rows into h_rows
    fc2_bam_digest *d_rows = nullptr, *h_rows = nullptr;
    uint32_t *d_first = nullptr, *h_first = nullptr;
    size_t rows_cap = 0;                       // rows h_rows holds (a batch with more gets no digests)
    std::vector<Chunk> dchunks;                // the chunks that were digested
    bool digest = false, rows_ready = false;
    // the listed records' fragment rows (bam_frag_kernel), indexed like the digest rows and made by the
    // first batch that asks for them.  With group the digest kernel runs whether or not its rows are
    // downloaded (digest): the fragment kernel reads them on the device
    fc2_bam_frag *d_frags = nullptr, *h_frags = nullptr;
    bool group = false, frags_ready = false;
    bool pooled = false;
    // the batch under way (gpu_begin .. gpu_finish)
    char *dest = nullptr;
    uint32_t n = 0;                            // blocks submitted
    int chunks = 0;                            // chunks given to the device
    bool spilled = false;                      // a block over 64 KiB was met: the CPU's from there on, no digests
    bool ok = true;
    std::string err;
};

static bool fail(Gpu *g, const std::string &what) {      // the first failure is the batch's error
    if (g->ok) g->err = "GPU inflate: " + what;
    g->ok = false;
    return false;
}
static bool hip_ok(Gpu *g, hipError_t e, const char *what) {
    return e == hipSuccess || fail(g, std::string(what) + ": " + hipGetErrorString(e));
}
static bool copy(Gpu *g, void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    return hip_ok(g, hipMemcpyAsync(dst, src, bytes, kind, s), kind == hipMemcpyHostToDevice ? "upload" : "download");
}
// a device buffer, or a pinned host one, of n elements: listed in g->bufs, which gpu_close frees
template <class T>
static bool make(Gpu *g, T *&p, size_t n, bool pinned, const char *what) {
    void *v = nullptr;
    if (!hip_ok(g, pinned ? hipHostMalloc(&v, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&v, n * sizeof(T)), what))
        return false;
    g->bufs.push_back({v, pinned});
    p = static_cast<T *>(v);
    return true;
}

Gpu *gpu_open(int device, uint32_t max_blocks, size_t pool_cap, std::string &err) {
    Gpu *g = new Gpu();
    g->device = device;
    g->max_blocks = max_blocks;
    g->src_cap = (size_t)max_blocks * kOutMax + 64;      // a BGZF block is at most 64 KiB
    const size_t M = max_blocks, out = M * kOutMax;
    uint32_t *h_meta = nullptr, *d_meta = nullptr, *h_walk = nullptr, *d_walk = nullptr;
    bool ok = hip_ok(g, hipSetDevice(device), "hipSetDevice");
    for (int k = 0; k < kStreams && ok; ++k)
        ok = hip_ok(g, hipStreamCreateWithFlags(&g->stream[k], hipStreamNonBlocking), "stream") &&
             hip_ok(g, hipEventCreateWithFlags(&g->done[k], hipEventBlockingSync | hipEventDisableTiming), "event");
    ok = ok && make(g, g->h_src, g->src_cap, true, "pinned input") && make(g, h_meta, M * Cols::kCount, true, "pinned table") &&
         make(g, g->d_src, g->src_cap, false, "device input") && make(g, g->d_slots, out, false, "device slots") &&
         make(g, g->d_out, out, false, "device output") && make(g, d_meta, M * Cols::kCount, false, "device table") &&
         make(g, h_walk, M * WalkCols::kCount, true, "pinned record counts") &&
         make(g, g->h_starts, M * kWalkCap, true, "pinned record lists") &&
         make(g, d_walk, M * WalkCols::kCount, false, "device record counts") &&
         make(g, g->d_starts, M * kWalkCap, false, "device record lists");
    if (!ok) {
        err = g->err;
        gpu_close(g);
        return nullptr;
    }
    g->h = Cols::of(h_meta, M), g->d = Cols::of(d_meta, M);
    g->h_walk = WalkCols::of(h_walk, M), g->d_walk = WalkCols::of(d_walk, M);
    if (pool_cap) {              // the batches the parse blocks and the read loop's chunks still hold, and one in flight
        pool_open(pool_cap, 16);
        g->pooled = true;
        void *first[3];                        // the first few made now (pinning takes ~10 ms each)
        for (void *&b : first) b = pinned_take(pool_cap);
        for (void *b : first)
            if (b) pinned_give(b);
    }
    return g;
}

void gpu_close(Gpu *g) {
    if (!g) return;
    if (hipSetDevice(g->device) == hipSuccess) {
        for (int k = 0; k < kStreams; ++k)
            if (g->stream[k]) (void)hipStreamSynchronize(g->stream[k]);
        for (auto b = g->bufs.rbegin(); b != g->bufs.rend(); ++b) (void)(b->second ? hipHostFree(b->first) : hipFree(b->first));
        for (int k = 0; k < kStreams; ++k) {
            if (g->done[k]) (void)hipEventDestroy(g->done[k]);
            if (g->stream[k]) (void)hipStreamDestroy(g->stream[k]);
        }
    }
    if (g->pooled) pool_close();
    delete g;
}

uint32_t gpu_max_blocks(const Gpu *g) { return g->max_blocks; }

// rows a block of the pinned row buffer: 64 KiB of records of 128 bytes or more
constexpr size_t kRowsPerBlock = 512;

void gpu_begin(Gpu *g, char *dest, bool walk, bool digest, bool group) {
    g->dest = dest;
    g->walk = walk || group;
    g->digest = g->walk && digest;
    g->group = group;
    g->spilled = g->rows_ready = g->frags_ready = false;
    g->dchunks.clear();
    g->n = 0;
    g->chunks = 0;
    g->ok = hipSetDevice(g->device) == hipSuccess;
    g->err = g->ok ? "" : "GPU inflate: hipSetDevice failed";
    const size_t M = g->max_blocks;
    g->rows_cap = M * kRowsPerBlock;
    if (g->ok && (g->digest || g->group) && !g->d_rows)
        make(g, g->d_rows, M * kWalkCap, false, "device digest rows") && make(g, g->d_first, 2 * M + 1, false, "device row index") &&
            make(g, g->h_first, 2 * M + 1, true, "pinned row index");
    if (g->ok && g->digest && !g->h_rows) make(g, g->h_rows, g->rows_cap, true, "pinned digest rows");
    if (g->ok && g->group && !g->d_frags)
        make(g, g->d_frags, M * kWalkCap, false, "device fragment rows") && make(g, g->h_frags, g->rows_cap, true, "pinned fragment rows");
}

constexpr size_t kWord = sizeof(uint32_t);

// Stage 1: the chunk's columns into the pinned table and its bytes into the pinned input (at their
// offsets in the batch, 8 zero bytes behind).  false: the chunk holds a block over 64 KiB, or follows
// one -- not BGZF, and its bytes may lie past what the buffers hold: the CPU inflates (and reports) its
// blocks and those of every later chunk; the chunks before it hold in-spec sizes only
static bool stage_chunk(Gpu *g, const uint8_t *raw, const Block *blocks, const Chunk &ch) {
    const Cols &h = g->h;
    for (size_t i = ch.i0; i < ch.i0 + ch.c; ++i) {
        const Block &b = blocks[i];
        g->spilled = g->spilled || b.isize > kOutMax || b.out + b.isize > (uint64_t)g->max_blocks * kOutMax;
        h.off[i] = (uint32_t)b.payload, h.len[i] = (uint32_t)b.len, h.isize[i] = b.isize, h.crc[i] = b.crc;
        h.ooff[i] = (uint32_t)b.out, h.rooff[i] = (uint32_t)(b.out - ch.o0);
    }
    if (g->spilled) {
        std::fill(h.status + ch.i0, h.status + ch.i0 + ch.c, (uint32_t)INF_TOO_BIG);
        return false;
    }
    memcpy(g->h_src + ch.b0, raw + ch.b0, ch.b1 - ch.b0);
    memset(g->h_src + ch.b1, 0, 8);
    return true;
}

// Stage 2: the bytes and the five columns the inflate and the compaction read go up; each block is
// inflated into its slot, then moved to its place in the batch
static bool enqueue_inflate(Gpu *g, const Chunk &ch) {
    hipStream_t s = g->stream[ch.s];
    const size_t i0 = ch.i0;
    const Cols &h = g->h, &d = g->d;
    bool ok = copy(g, g->d_src + ch.b0, g->h_src + ch.b0, ch.b1 + 8 - ch.b0, hipMemcpyHostToDevice, s);
    for (uint32_t *Cols::*col : {&Cols::off, &Cols::len, &Cols::isize, &Cols::crc, &Cols::ooff})
        ok = ok && copy(g, d.*col + i0, h.*col + i0, ch.c * kWord, hipMemcpyHostToDevice, s);
    if (!ok || fc2_bgzf_inflate_launch(g->d_src, d.off + i0, d.len + i0, d.isize + i0, d.crc + i0, g->d_slots + i0 * kOutMax,
                                       d.status + i0, ch.c, s) != FC2_OK)
        return fail(g, "launch failed");
    hipLaunchKernelGGL(compact_kernel, dim3(kOutMax / 16 / 256, ch.c), dim3(256), 0, s, g->d_slots + i0 * kOutMax,
                       d.isize + i0, d.ooff + i0, d.status + i0, g->d_out);
    return hip_ok(g, hipGetLastError(), "compact");
}
// Stage 3: the blocks' record lists, from the slots the compaction leaves as they are, and their download
static bool enqueue_walk(Gpu *g, const Chunk &ch) {
    hipStream_t s = g->stream[ch.s];
    const size_t i0 = ch.i0, r0 = i0 * kWalkCap;
    const WalkCols &h = g->h_walk, &d = g->d_walk;
    if (fc2_bam_walk_launch(g->d_slots + i0 * kOutMax, g->d.isize + i0, g->d.status + i0, g->d_starts + r0, d.count + i0,
                            d.exit + i0, ch.c, s) != FC2_OK)
        return fail(g, "record list launch failed");
    return copy(g, g->h_starts + r0, g->d_starts + r0, (size_t)ch.c * kWalkCap * sizeof(uint16_t), hipMemcpyDeviceToHost, s) &&
           copy(g, h.count + i0, d.count + i0, ch.c * kWord, hipMemcpyDeviceToHost, s) &&
           copy(g, h.exit + i0, d.exit + i0, ch.c * kWord, hipMemcpyDeviceToHost, s);
}

// Stage 4: the listed records' digest rows, from the chunk's contiguous bytes (records cross blocks),
// and the download of its row index; the rows follow in gpu_finish
static bool enqueue_digest(Gpu *g, Chunk ch) {
    hipStream_t s = g->stream[ch.s];
    const size_t i0 = ch.i0, r0 = i0 * kWalkCap;
    ch.foff = (uint32_t)(i0 + g->dchunks.size());
    if (!copy(g, g->d.rooff + i0, g->h.rooff + i0, ch.c * kWord, hipMemcpyHostToDevice, s)) return false;
    if (fc2_bam_digest_launch(g->d_out + ch.o0, (uint32_t)(ch.o1 - ch.o0), g->d.rooff + i0, g->d.isize + i0, g->d.status + i0,
                              g->d_starts + r0, g->d_walk.count + i0, g->d_rows + r0, g->d_first + ch.foff, ch.c, s) != FC2_OK)
        return fail(g, "record digest launch failed");
    if (g->group &&
        fc2_bam_frag_launch(g->d_out + ch.o0, (uint32_t)(ch.o1 - ch.o0), g->d.rooff + i0, g->d.isize + i0, g->d.status + i0,
                            g->d_starts + r0, g->d_walk.count + i0, g->d_rows + r0, g->d_first + ch.foff, g->d_frags + r0, ch.c,
                            s) != FC2_OK)
        return fail(g, "fragment row launch failed");
    if (!copy(g, g->h_first + ch.foff, g->d_first + ch.foff, (ch.c + 1) * kWord, hipMemcpyDeviceToHost, s)) return false;
    g->dchunks.push_back(ch);
    return true;
}

// Stage 5: the chunk's bytes into the batch buffer, and its statuses
static bool enqueue_download(Gpu *g, const Chunk &ch) {
    hipStream_t s = g->stream[ch.s];
    return copy(g, g->dest + ch.o0, g->d_out + ch.o0, ch.o1 - ch.o0, hipMemcpyDeviceToHost, s) &&
           copy(g, g->h.status + ch.i0, g->d.status + ch.i0, ch.c * kWord, hipMemcpyDeviceToHost, s);
}

bool gpu_add(Gpu *g, const uint8_t *raw, const Block *blocks, size_t i0, size_t i1) {
    if (!g->ok) return false;
    if (i1 <= i0) return true;
    const Block &first = blocks[i0], &last = blocks[i1 - 1];
    if (i0 != g->n || i1 > g->max_blocks || last.at + last.size + 8 > g->src_cap)
        return fail(g, "chunk out of order or larger than the buffers");
    g->n = (uint32_t)i1;
    Chunk ch{(uint32_t)i0, (uint32_t)(i1 - i0), first.at, last.at + last.size, first.out, last.out + last.isize, 0, 0, 0};
    if (!stage_chunk(g, raw, blocks, ch)) return true;
    ch.s = g->chunks++ % kStreams;
    return enqueue_inflate(g, ch) && (!g->walk || enqueue_walk(g, ch)) &&
           ((!g->digest && !g->group) || ch.c > kDigestMaxBlocks || enqueue_digest(g, ch)) && enqueue_download(g, ch);
}

bool gpu_finish(Gpu *g, std::string &err) {
    for (int k = 0; k < kStreams; ++k)
        if (hip_ok(g, hipEventRecord(g->done[k], g->stream[k]), "event")) hip_ok(g, hipEventSynchronize(g->done[k]), "kernel");
    // the digest rows and the fragment rows, now that every chunk's first[] says how many there are: a
    // sized download per chunk on its stream, side by side, then the same wait again
    if (g->ok && (g->digest || g->group) && !g->spilled && !g->dchunks.empty()) {
        uint64_t total = 0;
        for (Chunk &ch : g->dchunks) {
            ch.row0 = total;
            total += std::min<uint64_t>(g->h_first[ch.foff + ch.c], (uint64_t)ch.c * kWalkCap);
        }
        if (total <= g->rows_cap) {
            bool used[kStreams] = {};
            for (const Chunk &ch : g->dchunks) {
                const uint64_t n = std::min<uint64_t>(g->h_first[ch.foff + ch.c], (uint64_t)ch.c * kWalkCap);
                const size_t r0 = (size_t)ch.i0 * kWalkCap;
                if (!n) continue;
                if (g->digest && copy(g, g->h_rows + ch.row0, g->d_rows + r0, n * sizeof(fc2_bam_digest), hipMemcpyDeviceToHost,
                                      g->stream[ch.s]))
                    used[ch.s] = true;
                if (g->group && copy(g, g->h_frags + ch.row0, g->d_frags + r0, n * sizeof(fc2_bam_frag), hipMemcpyDeviceToHost,
                                     g->stream[ch.s]))
                    used[ch.s] = true;
            }
            for (int k = 0; k < kStreams; ++k)
                if (used[k] && hip_ok(g, hipEventRecord(g->done[k], g->stream[k]), "event"))
                    hip_ok(g, hipEventSynchronize(g->done[k]), "download");
            g->rows_ready = g->ok && g->digest;
            g->frags_ready = g->ok && g->group;
        }
    }
    if (!g->ok) err = g->err;
    return g->ok;
}

uint32_t gpu_status(const Gpu *g, size_t i) { return g->h.status[i]; }

const uint16_t *gpu_walk(const Gpu *g, size_t i, uint32_t &count, uint32_t &exit) {
    count = std::min<uint32_t>(g->h_walk.count[i], kWalkCap);
    exit = g->h_walk.exit[i];
    return g->h_starts + i * kWalkCap;
}

// block i's place among the downloaded rows: its first row's index and its row count (false: it has none)
static bool block_rows(const Gpu *g, size_t i, uint64_t &row, uint32_t &count) {
    count = 0;
    for (const Chunk &ch : g->dchunks)
        if (i >= ch.i0 && i < ch.i0 + ch.c) {
            const uint32_t *f = g->h_first + ch.foff;
            const uint32_t a = f[i - ch.i0], b = f[i - ch.i0 + 1];
            if (a > b || b > f[ch.c] || (uint64_t)f[ch.c] > (uint64_t)ch.c * kWalkCap) return false;
            count = b - a;
            row = ch.row0 + a;
            return true;
        }
    return false;
}

const fc2_bam_digest *gpu_digest(const Gpu *g, size_t i, uint32_t &count) {
    uint64_t row;
    count = 0;
    return g->rows_ready && block_rows(g, i, row, count) ? g->h_rows + row : nullptr;
}

const fc2_bam_frag *gpu_frags(const Gpu *g, size_t i, uint32_t &count) {
    uint64_t row;
    count = 0;
    return g->frags_ready && block_rows(g, i, row, count) ? g->h_frags + row : nullptr;
}

}  // namespace inf
}  // namespace fc2
