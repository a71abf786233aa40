// fc2_sam_frag_impl.h -- the head row and the fragment row of one line of SAM text (include/fc2_ingest.h
// fc2_sam_group_launch): the rule itself, compiled twice -- into sam_head_kernel and sam_frag_kernel
// (fc2_sam_group.hip), where a wavefront reads a line's head and a lane walks a fragment, and into
// fc2_sam_group_host (the same file's host side) -- over the same tables: the text, the lines' starts and the
// reference names' table of fc2_sam_encode_impl.h.
//
// starts[0 .. n_lines]: line k is text[starts[k] .. starts[k + 1] - 1), the byte before starts[k + 1] its `\n`;
// starts[0] = 0 and every other entry is one past a `\n` of the text, so every load below lies under
// starts[n_lines] <= n_bytes whatever the bytes hold.  The fragment rule is fc2_bam_frag_impl.h's with "record"
// read as "line": the back walk takes at most 5 steps, the forward walk at most FC2_BAM_FRAG_CAP + 1.
#pragma once
#include <stdint.h>

#include "../../include/fc2_ingest.h"
#include "fc2_sam_encode_impl.h"

namespace fc2 {
namespace samfrag {

// CIGAR bytes parse_sam_record takes: digits and cig_code's letters
FC2_SAMENC_HD bool cigar_byte(uint8_t c) { return (uint32_t)c - '0' <= 9 || samenc::cigar_op(c) >= 0; }

// The head row of line text[a .. b) (a <= b, inside the text).  A group G of lanes runs this with the same
// arguments in every lane (fc2_sam_encode_impl.h): the tabs are found G::width bytes a ballot, the fields are
// uniform in the group, and nothing is read after the 10th tab.
template <class G>
FC2_SAMENC_HD fc2_sam_head head_row(const G &g, const uint8_t *t, uint32_t a, uint32_t b, const uint32_t *table,
                                    uint32_t table_bytes) {
    fc2_sam_head row;
    row.flag = 0, row.tid = 0, row.l_name = 0, row.state = 0;
    const fc2_sam_head none = row;
    if (b > a && t[b - 1] == '\r') return none;
    uint32_t fb[10], fe[10];
    uint32_t p = a;
    for (uint32_t k = 0; k < 10; ++k) {
        const uint32_t e = samenc::find_tab(g, t, p, b);
        if (e == b) return none;                // fewer than 10 tabs (a blank line among them)
        fb[k] = p, fe[k] = e;
        p = e + 1;
    }
    const uint32_t l_name = fe[0] - fb[0];
    if (l_name < 1 || l_name > 254) return none;
    const uint32_t l_flag = fe[1] - fb[1];
    if (l_flag < 1 || l_flag > 5) return none;
    uint32_t flag = 0;
    for (uint32_t i = fb[1]; i < fe[1]; ++i) {
        const uint32_t d = (uint32_t)t[i] - '0';
        if (d > 9) return none;
        flag = flag * 10 + d;
    }
    if (flag > 65535) return none;
    if (!(fe[5] - fb[5] == 1 && t[fb[5]] == '*')) {
        // every lane looks at its own bytes of the CIGAR; one bad byte anywhere refuses the line
        for (uint32_t q = fb[5]; q < fe[5]; q += G::width) {
            const uint32_t i = q + g.lane();
            if (g.ballot(i < fe[5] && !cigar_byte(t[i]))) return none;
        }
    }
    row.flag = flag;
    row.tid = (fe[2] - fb[2] == 1 && t[fb[2]] == '*') ? -1 : samenc::name_lookup(table, table_bytes, t + fb[2], fe[2] - fb[2]);
    row.l_name = l_name;
    row.state = 1;
    return row;
}

struct Tables {
    const uint8_t *text;
    const uint32_t *starts;                     // n_lines + 1 entries
    const fc2_sam_head *rows;                   // n_lines head rows
    uint32_t n_lines;
};

// byte equality of the two QNAMEs (both lines usable: l_name bytes from the line's start lie inside it)
FC2_SAMENC_HD bool same_name(const Tables &T, uint32_t i, uint32_t j) {
    const uint32_t n = T.rows[i].l_name;
    if (n != T.rows[j].l_name) return false;
    const uint8_t *x = T.text + T.starts[i], *y = T.text + T.starts[j];
    for (uint32_t k = 0; k < n; ++k)
        if (x[k] != y[k]) return false;
    return true;
}

// the fragment row of line k (k < n_lines): include/fc2_ingest.h states the rule
FC2_SAMENC_HD fc2_bam_frag frag_row(const Tables &T, uint32_t k) {
    fc2_bam_frag out;
    out.state = out.n_records = out.n_mates = out.n_unmapped = 0;
    out.bytes = 0;
    const fc2_bam_frag none = out;
    const fc2_sam_head H = T.rows[k];
    if (H.state != 1 || (H.flag & 4u)) return none;                            // 1. a usable, mapped head
    // 2. the mapped line before it has another name: at most 4 unmapped ones lie between
    {
        uint32_t j = k;
        for (uint32_t step = 0;; ++step) {
            if (step == 5 || j == 0) return none;
            --j;
            const fc2_sam_head P = T.rows[j];
            if (P.state != 1) return none;
            if (P.flag & 4u) continue;
            if (same_name(T, j, k)) return none;
            break;
        }
    }
    // 3. - 5. forward to the first mapped line with another name
    uint32_t n_records = 1, n_mates = 1, n_unmapped = 0;
    uint32_t prim_flag = H.flag;
    int32_t prim_ref = H.tid;
    for (uint32_t step = 0; step <= (uint32_t)FC2_BAM_FRAG_CAP; ++step) {
        const uint32_t j = k + 1 + step;
        if (j >= T.n_lines) return none;                                      // the closer is not a line of this block
        const fc2_sam_head R = T.rows[j];
        if (R.state != 1) return none;
        const bool unmapped = (R.flag & 4u) != 0;
        if (!unmapped && !same_name(T, j, k)) {                               // N: the fragment is closed
            out.state = 1;
            out.n_records = (uint8_t)n_records;
            out.n_mates = (uint8_t)n_mates;
            out.n_unmapped = (uint8_t)n_unmapped;
            out.bytes = T.starts[j] - T.starts[k];
            return out;
        }
        if (++n_records > (uint32_t)FC2_BAM_FRAG_CAP) return none;
        if (unmapped) {
            ++n_unmapped;
        } else if ((R.flag & 0x40u) == (prim_flag & 0x40u)) {                  // a segment of the current mate
            if (R.tid == prim_ref && (R.flag & 0x10u) == (prim_flag & 0x10u)) return none;   // proper
        } else {
            if (n_mates == 2) return none;                                    // a third mate would open
            n_mates = 2;
            prim_flag = R.flag;
            prim_ref = R.tid;
        }
    }
    return none;
}

// The host's form of the whole rule: *n_lines always; starts[0 .. n_lines], the head rows and the fragment rows
// only where n_lines <= cap
inline void group_text(const uint8_t *text, uint32_t n_bytes, const uint32_t *table, uint32_t table_bytes, uint32_t *starts,
                       fc2_sam_head *line_rows, fc2_bam_frag *frag_rows, uint32_t *n_lines, uint32_t cap) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_bytes; ++i) n += text[i] == '\n';
    *n_lines = n;
    if (n > cap) return;
    starts[0] = 0;
    for (uint32_t i = 0, k = 0; i < n_bytes; ++i)
        if (text[i] == '\n') starts[++k] = i + 1;
    const samenc::One g;
    for (uint32_t k = 0; k < n; ++k) line_rows[k] = head_row(g, text, starts[k], starts[k + 1] - 1, table, table_bytes);
    const Tables T = {text, starts, line_rows, n};
    for (uint32_t k = 0; k < n; ++k) frag_rows[k] = frag_row(T, k);
}

}  // namespace samfrag
}  // namespace fc2
