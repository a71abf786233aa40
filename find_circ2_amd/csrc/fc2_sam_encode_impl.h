// fc2_sam_encode_impl.h -- one SAM text line into the BAM record fc2::bam::encode_sam (fc2_bamout.cpp) makes
// of it (include/fc2_ingest.h fc2_sam_encode_launch): the rule itself, compiled twice -- into sam_size_kernel
// and sam_write_kernel (fc2_sam_encode.hip), where a wavefront works on a line, and into fc2_sam_encode_host
// (the same file's host side), where one "lane" does -- over the same tables: the text, the lines' offsets
// and the reference names' table.
//
// The contract is "never a wrong byte": parse() either refuses the line (a FC2_SAM_ENC_* reason) or accepts
// it, and an accepted line is one on which encode_sam succeeds and whose bytes write() reproduces.  Every
// place where encode_sam is laxer than the grammar below (strtol's leading blanks and signs, a CIGAR count
// without digits or one that wraps 32 bits, an empty QNAME, strtof) is a refusal here, not an approximation.
//
// A group G of lanes (G::width of them, this one g.lane(), g.ballot(p): bit k set where lane k's p holds)
// runs every function below with the same arguments in every lane, so all control flow is uniform in the
// group; the lanes differ only in which bytes they load for a ballot and which bytes they store.  The host's
// group is one lane wide.  Loads lie in [a, b) of the line, stores in [dst, dst + plan.size).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/fc2_ingest.h"

#if defined(__HIPCC__)
#define FC2_SAMENC_HD __host__ __device__ inline
#else
#define FC2_SAMENC_HD inline
#endif

namespace fc2 {
namespace samenc {

constexpr uint32_t kMaxLines = FC2_SAM_ENC_MAX_LINES, kMaxText = FC2_SAM_ENC_MAX_TEXT;
constexpr uint32_t kFixed = 36;                 // block_size and the 32 bytes before the name

// Bytes a line of `line` bytes becomes at most: 2 * line + 40.  An accepted line has 10 tabs or more; its
// record is 36 bytes, the name and its NUL, 4 bytes an op, ceil(l_seq / 2) + l_seq bytes of bases and
// qualities, and the tags.  Against the text: QNAME of q bytes gives q + 1 <= 2 q + 1; a CIGAR op is two
// characters or more and gives 4 bytes; SEQ of s >= 1 characters gives ceil(s / 2) + s <= 2 s (`*`: nothing);
// a tag of t >= 5 characters and the tab before it give 4 (A), at most 7 (i, t >= 6) or t - 1 (Z, H) bytes,
// each at most 2 (t + 1).  Every character is charged once, so the record is at most 36 + 1 + 2 * line.
FC2_SAMENC_HD uint64_t record_bound(uint64_t line) { return 2 * line + 40; }

// the host's group: one lane
struct One {
    static constexpr uint32_t width = 1;
    FC2_SAMENC_HD uint32_t lane() const { return 0; }
    FC2_SAMENC_HD uint64_t ballot(bool p) const { return p ? 1u : 0u; }
};

// ---- the names' table -----------------------------------------------------------------------------------
// Words: [0] the slots (a power of two, more than the names), [1] the table's bytes, then 3 words a slot --
// the name's byte offset in the table, its length (0xFFFFFFFF: an empty slot), its id -- then the names'
// bytes.  A name sits at the first free slot from hash & (slots - 1) on; a name that comes again overwrites
// the id (the last one wins, as std::unordered_map's operator[] = does in the ingest).
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
FC2_SAMENC_HD uint32_t name_hash(const uint8_t *s, uint32_t n) {          // FNV-1a
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ s[i]) * 16777619u;
    return h;
}

// the id of text[p .. e) in the table, -1 if it is not there (or the table is not one: every load is
// checked against table_bytes)
FC2_SAMENC_HD int32_t name_lookup(const uint32_t *table, uint32_t table_bytes, const uint8_t *s, uint32_t n) {
    if (table_bytes < 8) return -1;
    const uint32_t slots = table[0];
    if (!slots || (slots & (slots - 1)) || (uint64_t)slots * 12 + 8 > table_bytes) return -1;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(table);
    uint32_t k = name_hash(s, n) & (slots - 1);
    for (uint32_t step = 0; step < slots; ++step, k = (k + 1) & (slots - 1)) {
        const uint32_t at = table[2 + 3 * k], len = table[3 + 3 * k];
        if (len == kEmpty) return -1;
        if (len != n || (uint64_t)at + len > table_bytes) continue;
        uint32_t i = 0;
        while (i < n && bytes[at + i] == s[i]) ++i;
        if (i == n) return (int32_t)table[4 + 3 * k];
    }
    return -1;
}

// the table of these names (lens null: C strings); empty if it would pass 4 GiB
inline std::vector<uint32_t> build_table(const char *const *names, const uint32_t *lens, uint32_t n) {
    uint32_t slots = 2;
    while (slots <= 2 * (uint64_t)n && slots < (1u << 30)) slots <<= 1;
    uint64_t name_bytes = 0;
    for (uint32_t i = 0; i < n; ++i) name_bytes += lens ? lens[i] : strlen(names[i]);
    const uint64_t head = 8 + 12ull * slots, all = (head + name_bytes + 3) & ~3ull;
    std::vector<uint32_t> t;
    if (all > 0xFFFFFFFFull) return t;
    t.assign((size_t)(all / 4), 0);
    t[0] = slots, t[1] = (uint32_t)all;
    for (uint32_t k = 0; k < slots; ++k) t[3 + 3 * k] = kEmpty;
    uint8_t *bytes = reinterpret_cast<uint8_t *>(t.data());
    uint32_t at = (uint32_t)head;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t *s = reinterpret_cast<const uint8_t *>(names[i]);
        const uint32_t len = lens ? lens[i] : (uint32_t)strlen(names[i]);
        uint32_t k = name_hash(s, len) & (slots - 1);
        for (;; k = (k + 1) & (slots - 1)) {
            if (t[3 + 3 * k] == kEmpty) {
                t[2 + 3 * k] = at, t[3 + 3 * k] = len, t[4 + 3 * k] = i;
                if (len) memcpy(bytes + at, s, len);
                at += len;
                break;
            }
            if (t[3 + 3 * k] == len && !memcmp(bytes + t[2 + 3 * k], s, len)) {
                t[4 + 3 * k] = i;               // the name again: the last one wins
                break;
            }
        }
    }
    return t;
}

// ---- the rule's pieces --------------------------------------------------------------------------------

// SAM spec 5.3 (fc2_bamout.cpp reg2bin, the same arithmetic on the same types)
FC2_SAMENC_HD int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// fc2_bamout.cpp nt16 without its switch: `=` is 0, a letter of either case its IUPAC code from a table of
// nibbles indexed by c & 31 (A = 1 .. Z = 26), anything else 15
FC2_SAMENC_HD uint32_t nt16(uint8_t c) {
    if (c == '=') return 0;
    const uint8_t l = c | 0x20;
    if (l < 'a' || l > 'z') return 15;
    const uint32_t i = c & 31u;
    const uint64_t lo = 0xFF3FCFFB4FFD2E1Full, hi = 0xFFFFFFAF978865FFull;
    return (uint32_t)((i < 16 ? lo >> (4 * i) : hi >> (4 * (i - 16))) & 15u);
}

FC2_SAMENC_HD int cigar_op(uint8_t c) {
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
        default: return -1;
    }
}

// the first tab in [p, end), or end: the lanes look at G::width bytes a step
template <class G>
FC2_SAMENC_HD uint32_t find_tab(const G &g, const uint8_t *t, uint32_t p, uint32_t end) {
    for (; p < end; p += G::width) {
        const uint32_t i = p + g.lane();
        const uint64_t m = g.ballot(i < end && t[i] == '\t');
        if (m) return p + (uint32_t)__builtin_ctzll(m);
    }
    return end;
}

// -?[0-9]{1,max_digits} and nothing else: what strtol / strtoll give for it (no overflow at 18 digits)
FC2_SAMENC_HD bool parse_int(const uint8_t *t, uint32_t p, uint32_t e, uint32_t max_digits, int64_t &v) {
    const bool neg = p < e && t[p] == '-';
    if (neg) ++p;
    if (p == e || e - p > max_digits) return false;
    int64_t x = 0;
    for (; p < e; ++p) {
        const uint32_t d = (uint32_t)t[p] - '0';
        if (d > 9) return false;
        x = x * 10 + d;
    }
    v = neg ? -x : x;
    return true;
}

// what parse() learns of a line, enough for write() to place every byte
struct Plan {
    uint32_t status, size;                      // size: the record with its block_size; 0 when refused
    uint32_t fb[11], fe[11];                    // the 11 mandatory fields: text[fb[k] .. fe[k])
    uint32_t tags, end;                         // the first tag's first byte (end + 1: no tag), the line's end
    int32_t ref, pos, nref, npos, tlen;
    uint32_t flag, mapq, bin, n_cig, l_qname, l_seq, l_qual;
    bool cigar_star, qual_star;
};

// CIGAR text[p .. e), not `*`: ([0-9]{1,9}[MIDNSHP=X])+ with every count below 2^28 and at most 65535 ops.
// dst (write()'s call): op j's 4 bytes at dst + 4 j, stored by lane j % width.
template <class G>
FC2_SAMENC_HD bool cigar(const G &g, const uint8_t *t, uint32_t p, uint32_t e, uint32_t &n_ops, int64_t &rlen, uint8_t *dst) {
    uint32_t n = 0, digits = 0, ops = 0;
    int64_t span = 0;
    for (; p < e; ++p) {
        const uint8_t c = t[p];
        const uint32_t d = (uint32_t)c - '0';
        if (d <= 9) {
            if (++digits > 9) return false;
            n = n * 10 + d;
            continue;
        }
        const int op = cigar_op(c);
        if (op < 0 || !digits || n >= (1u << 28) || ops == 65535) return false;
        if (dst && ops % G::width == g.lane()) {
            const uint32_t w = n << 4 | (uint32_t)op;
            uint8_t *o = dst + 4 * (uint64_t)ops;
            o[0] = (uint8_t)w, o[1] = (uint8_t)(w >> 8), o[2] = (uint8_t)(w >> 16), o[3] = (uint8_t)(w >> 24);
        }
        ++ops;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += n;
        n = 0, digits = 0;
    }
    if (digits || !ops) return false;           // a trailing count, or nothing at all
    n_ops = ops, rlen = span;
    return true;
}

// The tags text[p .. end): with dst null their bytes are counted, otherwise written at dst.  False and
// `why`: a tag the rule refuses.
template <class G>
FC2_SAMENC_HD bool tags(const G &g, const uint8_t *t, uint32_t p, uint32_t end, uint32_t &bytes, uint32_t &why, uint8_t *dst) {
    uint32_t at = 0;
    const bool first = g.lane() == 0;
    for (;;) {
        const uint32_t e = find_tab(g, t, p, end);
        if (e - p < 5 || t[p + 2] != ':' || t[p + 4] != ':') { why = FC2_SAM_ENC_TAG; return false; }
        const uint8_t type = t[p + 3];
        const uint32_t v = p + 5, vlen = e - v;
        uint8_t *o = dst ? dst + at : nullptr;
        if (o && first) o[0] = t[p], o[1] = t[p + 1];
        if (type == 'A') {
            if (o && first) o[2] = 'A', o[3] = vlen ? t[v] : 0;
            at += 4;
        } else if (type == 'i') {               // the smallest integer type that holds it (encode_sam)
            int64_t x;
            if (!parse_int(t, v, e, 18, x)) { why = FC2_SAM_ENC_TAG; return false; }
            uint8_t code;
            uint32_t nb;
            if (x < 0) {
                if (x >= -128) code = 'c', nb = 1;
                else if (x >= -32768) code = 's', nb = 2;
                else code = 'i', nb = 4;
            } else {
                if (x <= 255) code = 'C', nb = 1;
                else if (x <= 65535) code = 'S', nb = 2;
                else code = 'I', nb = 4;
            }
            if (o && first) {
                o[2] = code;
                const uint32_t w = (uint32_t)(uint64_t)x;       // (the host's casts keep the low bytes)
                for (uint32_t k = 0; k < nb; ++k) o[3 + k] = (uint8_t)(w >> (8 * k));
            }
            at += 3 + nb;
        } else if (type == 'Z' || type == 'H') {
            if (o) {
                if (first) o[2] = type;
                for (uint32_t k = g.lane(); k <= vlen; k += G::width) o[3 + k] = k < vlen ? t[v + k] : 0;
            }
            at += 3 + vlen + 1;
        } else {
            why = FC2_SAM_ENC_TAG_TYPE;
            return false;
        }
        if (e == end) break;
        p = e + 1;
    }
    bytes = at;
    return true;
}

// line text[a .. b) (a <= b, inside the text) against the rule
template <class G>
FC2_SAMENC_HD Plan parse(const G &g, const uint8_t *t, uint32_t a, uint32_t b, const uint32_t *table, uint32_t table_bytes) {
    Plan P;
    P.size = 0;
    P.end = b;
    auto refuse = [&](uint32_t why) { P.status = why; P.size = 0; return P; };
    uint32_t p = a;
    for (uint32_t k = 0; k < 11; ++k) {
        const uint32_t e = find_tab(g, t, p, b);
        P.fb[k] = p, P.fe[k] = e;
        if (k < 10 && e == b) return refuse(FC2_SAM_ENC_FIELDS);
        p = e + 1;
    }
    P.tags = p;                                 // (b + 1 where field 11 ends the line)
    P.l_qname = P.fe[0] - P.fb[0];
    if (P.l_qname < 1 || P.l_qname > 254) return refuse(FC2_SAM_ENC_QNAME);
    int64_t flag, pos, mapq, npos, tlen;
    if (!parse_int(t, P.fb[1], P.fe[1], 9, flag) || !parse_int(t, P.fb[3], P.fe[3], 9, pos) ||
        !parse_int(t, P.fb[4], P.fe[4], 9, mapq) || !parse_int(t, P.fb[7], P.fe[7], 9, npos) ||
        !parse_int(t, P.fb[8], P.fe[8], 9, tlen))
        return refuse(FC2_SAM_ENC_NUMBER);
    P.flag = (uint16_t)flag;
    P.pos = (int32_t)(pos - 1);
    P.mapq = (uint8_t)mapq;
    P.npos = (int32_t)(npos - 1);
    P.tlen = (int32_t)tlen;
    auto star = [&](int k) { return P.fe[k] - P.fb[k] == 1 && t[P.fb[k]] == '*'; };
    auto tid = [&](int k) { return star(k) ? -1 : name_lookup(table, table_bytes, t + P.fb[k], P.fe[k] - P.fb[k]); };
    P.ref = tid(2);
    P.nref = (P.fe[6] - P.fb[6] == 1 && t[P.fb[6]] == '=') ? P.ref : tid(6);
    P.cigar_star = star(5);
    P.n_cig = 0;
    int64_t rlen = 0;
    if (!P.cigar_star && !cigar(g, t, P.fb[5], P.fe[5], P.n_cig, rlen, nullptr)) return refuse(FC2_SAM_ENC_CIGAR);
    const int64_t e = (!(P.flag & 4u) && P.n_cig && rlen > 0) ? P.pos + rlen : (int64_t)P.pos + 1;
    P.bin = (uint16_t)reg2bin(P.pos, e);
    P.l_seq = star(9) ? 0 : P.fe[9] - P.fb[9];
    P.qual_star = star(10);
    P.l_qual = P.fe[10] - P.fb[10];
    uint32_t tag_bytes = 0, why = 0;
    if (P.tags <= b && !tags(g, t, P.tags, b, tag_bytes, why, nullptr)) return refuse(why);
    P.size = kFixed + P.l_qname + 1 + 4 * P.n_cig + (P.l_seq + 1) / 2 + P.l_seq + tag_bytes;
    P.status = FC2_SAM_ENC_OK;
    return P;
}

// word j (0..8) of the record's first 36 bytes
FC2_SAMENC_HD uint32_t fixed_word(const Plan &P, uint32_t j) {
    switch (j) {
        case 0: return P.size - 4;
        case 1: return (uint32_t)P.ref;
        case 2: return (uint32_t)P.pos;
        case 3: return (P.l_qname + 1) | P.mapq << 8 | P.bin << 16;
        case 4: return P.n_cig | P.flag << 16;
        case 5: return P.l_seq;
        case 6: return (uint32_t)P.nref;
        case 7: return (uint32_t)P.npos;
        default: return (uint32_t)P.tlen;
    }
}

// an accepted line's record (P.status == 0) into dst[0 .. P.size): the lanes share every run of bytes
template <class G>
FC2_SAMENC_HD void write(const G &g, const uint8_t *t, const Plan &P, uint8_t *dst) {
    const uint32_t lane = g.lane();
    for (uint32_t k = lane; k < kFixed; k += G::width) dst[k] = (uint8_t)(fixed_word(P, k >> 2) >> (8 * (k & 3u)));
    uint8_t *o = dst + kFixed;
    for (uint32_t k = lane; k <= P.l_qname; k += G::width) o[k] = k < P.l_qname ? t[P.fb[0] + k] : 0;
    o += P.l_qname + 1;
    if (!P.cigar_star) {
        uint32_t n_ops;
        int64_t rlen;
        (void)cigar(g, t, P.fb[5], P.fe[5], n_ops, rlen, o);
    }
    o += 4 * (uint64_t)P.n_cig;
    const uint8_t *s = t + P.fb[9], *q = t + P.fb[10];
    const uint32_t packed = (P.l_seq + 1) / 2;
    for (uint32_t k = lane; k < packed; k += G::width)
        o[k] = (uint8_t)(nt16(s[2 * k]) << 4 | (2 * k + 1 < P.l_seq ? nt16(s[2 * k + 1]) : 0u));
    o += packed;
    for (uint32_t k = lane; k < P.l_seq; k += G::width)
        o[k] = P.qual_star || k >= P.l_qual ? (uint8_t)0xff : (uint8_t)(q[k] - 33);
    o += P.l_seq;
    if (P.tags <= P.end) {
        uint32_t bytes, why;
        (void)tags(g, t, P.tags, P.end, bytes, why, o);
    }
}

// line i's bounds from the offsets: false where they are not a line of the text
FC2_SAMENC_HD bool line_of(const uint32_t *off, uint32_t i, uint32_t text_bytes, uint32_t &a, uint32_t &b) {
    a = off[i], b = off[i + 1];
    return a <= b && b <= text_bytes;
}

// The host's form of the whole rule: status, size, out_off[0 .. n_lines], *total and the records; a record that
// would pass out_cap is not written (the entries check out_cap against FC2_SAM_ENC_BOUND, so none does)
inline void encode_batch(const uint8_t *text, uint32_t text_bytes, const uint32_t *off, uint32_t n_lines,
                         const uint32_t *table, uint32_t table_bytes, uint8_t *out, uint64_t out_cap, uint32_t *out_off,
                         uint32_t *size, uint32_t *status, uint32_t *total) {
    const One g;
    uint32_t at = 0;
    for (uint32_t i = 0; i < n_lines; ++i) {
        uint32_t a, b;
        out_off[i] = at;
        if (!line_of(off, i, text_bytes, a, b)) {
            status[i] = FC2_SAM_ENC_OFFSETS, size[i] = 0;
            continue;
        }
        const Plan P = parse(g, text, a, b, table, table_bytes);
        status[i] = P.status, size[i] = P.size;
        if (P.status == FC2_SAM_ENC_OK && (uint64_t)at + P.size <= out_cap) write(g, text, P, out + at);
        at += P.size;
    }
    out_off[n_lines] = at;
    *total = at;
}

}  // namespace samenc
}  // namespace fc2
