// fc2_bam_frag_impl.h -- the fragment row of one listed record start (include/fc2_ingest.h fc2_bam_frag):
// the rule itself, compiled twice -- into bam_frag_kernel (fc2_inflate.hip) and into fc2_bam_frag_host
// (fc2_ingest.cpp) -- over the same tables: the chunk's bytes, the blocks' offsets, the listed record
// starts, the digest rows of those starts and the rows' index.
//
// A record is reached only through a listed start whose digest row has state 1 (frag_load): the row's
// block_size gives its end, which is checked against n_bytes again here, so every load below lies under a
// record end that was shown to be at most n_bytes whatever rows and bytes hold.  The back walk takes at
// most 5 steps (4 unmapped records and the mapped one), the forward walk at most FC2_BAM_FRAG_CAP + 1 (the
// fragment's records after the head, and the record that closes it); a step moves the (block, k) cursor
// over each block and each listed start at most once.
#pragma once
#include <stdint.h>

#include "../../include/fc2_ingest.h"

#if defined(__HIPCC__)
#define FC2_FRAG_HD __host__ __device__ inline
#else
#define FC2_FRAG_HD inline
#endif

namespace fc2 {
namespace frag {

struct Tables {
    const uint8_t *bytes;
    uint32_t n_bytes;
    const uint32_t *ooff;                      // block j's first byte in `bytes` (ascending)
    const uint16_t *starts;                    // FC2_BAM_WALK_CAP entries a block
    const uint32_t *count;
    const fc2_bam_digest *rows;                // rows[first[j] + k]: the digest of block j's k-th start
    const uint32_t *first;
    uint32_t n_blocks;
};

// a usable record: where it starts and ends, and the fields the rule reads
struct Rec {
    uint32_t j, k;                             // block, and index among its listed starts
    uint64_t at, lim;                          // [at, lim): block_size and body
    uint32_t flag, l_name;
    int32_t ref;
};

FC2_FRAG_HD uint32_t u8(const Tables &T, uint64_t o) { return T.bytes[o]; }
FC2_FRAG_HD uint32_t u16(const Tables &T, uint64_t o) { return u8(T, o) | (u8(T, o + 1) << 8); }
FC2_FRAG_HD uint32_t u32(const Tables &T, uint64_t o) { return u16(T, o) | (u16(T, o + 2) << 16); }
FC2_FRAG_HD uint32_t listed(const Tables &T, uint32_t j) {
    const uint32_t c = T.count[j];
    return c < (uint32_t)FC2_BAM_WALK_CAP ? c : (uint32_t)FC2_BAM_WALK_CAP;
}

// block j's k-th listed start (k < listed(j)): false unless its digest row has state 1 and the record the
// row describes -- 4 + block_size bytes, its name inside them -- lies below n_bytes
FC2_FRAG_HD bool frag_load(const Tables &T, uint32_t j, uint32_t k, Rec &r) {
    const fc2_bam_digest &d = T.rows[(uint64_t)T.first[j] + k];
    if (d.state != 1) return false;
    r.j = j, r.k = k;
    r.at = (uint64_t)T.ooff[j] + T.starts[(uint64_t)j * FC2_BAM_WALK_CAP + k];
    const uint64_t bs = d.block_size;
    r.lim = r.at + 4 + bs;
    if (bs < 32 || r.lim > T.n_bytes) return false;
    r.ref = (int32_t)u32(T, r.at + 4);
    r.l_name = u8(T, r.at + 12);
    r.flag = u16(T, r.at + 18);
    return r.l_name >= 1 && 32 + (uint64_t)r.l_name <= bs;
}

// std::string equality of the two query names: l_read_name and the l_read_name - 1 bytes before the NUL
FC2_FRAG_HD bool same_name(const Tables &T, const Rec &a, const Rec &b) {
    if (a.l_name != b.l_name) return false;
    for (uint32_t i = 0; i + 1 < a.l_name; ++i)
        if (u8(T, a.at + 36 + i) != u8(T, b.at + 36 + i)) return false;
    return true;
}

// the listed start before (j, k) in the order of the lists; false: there is none
FC2_FRAG_HD bool step_back(const Tables &T, uint32_t &j, uint32_t &k) {
    if (k) { --k; return true; }
    while (j) {
        const uint32_t c = listed(T, --j);
        if (c) { k = c - 1; return true; }
    }
    return false;
}

// the cursor (j, k) moved forward to byte `to` of the stream (past its own start): true if `to` is a listed
// start, which (j, k) then names
FC2_FRAG_HD bool seek(const Tables &T, uint32_t &j, uint32_t &k, uint64_t to) {
    while (j + 1 < T.n_blocks && T.ooff[j + 1] <= to) ++j, k = 0;
    const uint32_t c = listed(T, j);
    const uint16_t *S = T.starts + (uint64_t)j * FC2_BAM_WALK_CAP;
    while (k < c && (uint64_t)T.ooff[j] + S[k] < to) ++k;
    return k < c && (uint64_t)T.ooff[j] + S[k] == to;
}

// the row of block j's k-th listed start (include/fc2_ingest.h states the rule)
FC2_FRAG_HD fc2_bam_frag frag_row(const Tables &T, uint32_t j, uint32_t k) {
    fc2_bam_frag out;
    out.state = out.n_records = out.n_mates = out.n_unmapped = 0;
    out.bytes = 0;
    const fc2_bam_frag none = out;
    Rec H;
    if (!frag_load(T, j, k, H) || (H.flag & 4u)) return none;                  // 1. a usable, mapped head
    // 2. the mapped record before it has another name: at most 4 unmapped ones lie between
    {
        uint32_t bj = j, bk = k;
        uint64_t at = H.at;
        for (uint32_t step = 0;; ++step) {
            Rec P;
            if (step == 5 || !step_back(T, bj, bk) || !frag_load(T, bj, bk, P) || P.lim != at) return none;
            at = P.at;
            if (P.flag & 4u) continue;
            if (same_name(T, P, H)) return none;
            break;
        }
    }
    // 3. - 5. forward to the first mapped record with another name
    uint32_t n_records = 1, n_mates = 1, n_unmapped = 0;
    uint32_t prim_flag = H.flag;
    int32_t prim_ref = H.ref;
    uint32_t cj = j, ck = k;
    uint64_t nx = H.lim;
    for (uint32_t step = 0; step <= (uint32_t)FC2_BAM_FRAG_CAP; ++step) {
        Rec R;
        if (!seek(T, cj, ck, nx) || !frag_load(T, cj, ck, R)) return none;
        nx = R.lim;
        const bool unmapped = (R.flag & 4u) != 0;
        if (!unmapped && !same_name(T, R, H)) {                               // N: the fragment is closed
            out.state = 1;
            out.n_records = (uint8_t)n_records;
            out.n_mates = (uint8_t)n_mates;
            out.n_unmapped = (uint8_t)n_unmapped;
            out.bytes = (uint32_t)(R.at - H.at);
            return out;
        }
        if (++n_records > (uint32_t)FC2_BAM_FRAG_CAP) return none;
        if (unmapped) {
            ++n_unmapped;
        } else if ((R.flag & 0x40u) == (prim_flag & 0x40u)) {                  // a segment of the current mate
            if (R.ref == prim_ref && (R.flag & 0x10u) == (prim_flag & 0x10u)) return none;   // proper
        } else {
            if (n_mates == 2) return none;                                    // a third mate would open
            n_mates = 2;
            prim_flag = R.flag;
            prim_ref = R.ref;
        }
    }
    return none;
}

}  // namespace frag
}  // namespace fc2
