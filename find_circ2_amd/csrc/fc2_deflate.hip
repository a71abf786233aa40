// fc2_deflate.hip -- DEFLATE compression on the GPU: the gzip members of spliced_reads.fastq.gz
// (fc2_gzpieces.h's device mode, fc2_deflate_gpu.hip), the mirror image of fc2_inflate.hip.
//
// The text is cut into tiles of at most 64 KiB; a tile never refers to bytes before its own start
// (but with a history, below: then to input bytes of its launch, never to another tile's output),
// so tiles are independent: one wavefront per tile, no waits between workgroups.  Each tile becomes
// one complete raw DEFLATE stream (RFC 1951) -- a single dynamic-Huffman block, or stored block(s)
// when that would not be smaller -- with the gzip CRC-32 of its input beside it, so the host only
// wraps it in a gzip header and trailer, and the project's own inflater can read it back.
//
// The tile is held whole in LDS.  Pass 1 (matches): 64 consecutive positions a step, one per lane;
// a hash of the next 4 bytes indexes a table of last positions (read first, then updated with an LDS
// atomicMax of the position, so the table does not depend on the order the lanes get there); the
// candidate is compared 4 bytes at a time; a match is kept if it should cost less than its bytes as
// literals (the tile's byte entropy, from a histogram taken while the tile is loaded, against the
// length and distance codes' sizes); overlaps inside the 64 positions are resolved greedily in scalar
// code over the ballot of the lanes that found one.  The tokens go to a per-tile scratch in global
// memory (4 bytes each; they do not fit in LDS beside the tile) and into the two symbol histograms.
// The Huffman codes (lengths <= 15, zlib's overflow repair; always complete: a code with fewer than
// two symbols is padded with dummy ones as zlib does) are built with the symbols ranked in parallel
// and the tree made by one lane, in the hash table's LDS, free by then.  Pass 2 (emission): 64 tokens a
// step, a prefix sum of their bit counts over the lanes, each lane ORs its bits into a staging
// buffer in LDS (atomicOr on 32-bit words) that is laid out with the destination's alignment, so it
// is flushed to HBM in whole aligned 16-byte pieces; only the first and last pieces of a stream are
// stored byte by byte, and nothing outside [slot, slot + out_len) is written.
//
// LDS: 22540 B beside the tile (hash table 16 KiB, staging 3 KiB, histograms, codes): 55324 B with a
// tile of 32 KiB -- two workgroups a CU of 160 KiB -- and 88092 B with one of 64 KiB: one a CU.
//
// Level 2 (deflate_kernel<2>, fc2_deflate_launch_level) is the same kernel with a deeper pass 1; what
// follows pass 1 is shared, and level 1's instantiation has neither the code nor the LDS below.
//   Links.  Beside the table of heads there is link[], one 16-bit entry per position, indexed by
// p & 32767: the distance from p back to the head its step read for it before the step's own positions
// were entered (1..32768), or 0 for none -- no head, or one more than 32768 back.  Every position with
// p + 4 <= n writes its entry where it enters itself into the heads; the 64 positions of a step have 64
// slots of their own, so link[], like the heads, does not depend on the order of the lanes.
//   Search.  A position p >= skip walks at most 8 candidates: the head it read, then
// c - link[c & 32767] (so every candidate lies strictly below the one before).  The walk ends before a
// candidate that is none, that is more than 32768 back, or whose link slot this very step has
// rewritten (c + 32768 < base + 64: position c + 32768 is one of the step's own).  A candidate whose
// first four bytes are p's gets its length as at level 1, at most min(n - p, 258); the longest is kept,
// the first found (the nearest) among equal ones; once the kept length reaches 32 or the cap the walk
// ends.  The kept match must pass level 1's cost rule.
//   Lazy resolution.  Going up from the lowest open position of the step: the match at step index i is
// dropped for a literal if i + 1 < 64 and index i + 1 found a longer one; else it is taken as at level
// 1.  Nothing is deferred from index 63 to the next step.
//   Bounds (link[]).  link[] has min(tile rounded up to 4, 32768) entries behind the tile's padding.  A
// store is at p & 32767 with p < n <= tile; a load at c & 32767 with c < p, since the first candidate
// is a head of an earlier step and every further one is c - back with 1 <= back <= c, checked before
// the subtraction.  Every c walked is a position that entered itself and so wrote its entry: no entry
// is read before it is written, and the slot of c cannot hold c + 32768's entry, because the walk has
// ended where c + 32768 < base + 64 and later positions have not been entered yet.  The walk is bounded
// by 8 and by the falling candidate, the extension by 258; tile bytes are read up to c + 258 + 3 <
// n + 16, as at level 1.  Level 2 adds no store to global memory.
//   LDS at level 2: 2 bytes more per position of the window: 120860 B with a tile of 32 KiB, 153372 B
// at 0xff00, 153628 B at 64 KiB -- one workgroup a CU at every tile over some 19 KiB.
//
// History (deflate_kernel<level, true>, fc2_deflate_launch_hist; tests/deflate_model_hist.py is the rule in
// Python, bit-exact).  The launch's n bytes are one DEFLATE stream cut into tiles.  Tile i covers
// src[i * tile, min(n, (i + 1) * tile)); its history is the h = min(hist, i * tile) input bytes before it --
// input, so no tile waits for another's output -- and the launch's first tile has none.  LDS holds the region:
// history and tile back to back, m = h + (the tile's bytes) <= 65536 bytes; positions are counted from the
// history's first byte, the tile starts at position h.
//   Steps.  Pass 1 steps over the whole region 64 positions at a time from position 0 (base = 0, 64, ...), so
// one step may hold the history's last positions and the tile's first.  Every position with p + 4 <= m, of
// the history or of the tile (a history position's four bytes may run into the tile), enters the heads and at
// level 2 writes its link[] entry exactly as above: read first, then atomicMax.  Pass 1 starts with skip = h
// in place of 0: the history lies "inside a match" that ends where the tile begins, and that alone keeps a
// history position from searching and from giving a token (a step wholly inside it is left after it has
// entered its positions; a step across the boundary has its history lanes covered).
//   Matches.  A tile position searches as above; its candidate is any earlier position, of the history too.
// The distance limit stays 32768, the length limit min(258, m - p): the end of the tile.  A match whose
// source starts in the history and runs into the tile is an ordinary overlapping match.
//   Not the history's: the bytes' histogram and with it the literal cost (taken over positions h .. m, divided
// by the tile's length), the CRC-32 (crc[i] is the CRC of the tile's own bytes, read at any byte offset of the
// region), the tokens, and so ISIZE.
//   Stream.  The launch's last tile is written as above, BFINAL = 1.  Every other tile writes its dynamic block
// with BFINAL = 0 and an empty stored block behind it -- bits 000, zeros to the byte boundary, 00 00 FF FF, at
// most 5 bytes -- so its stream ends on a byte boundary and the streams back to back are one stream.  The
// Huffman form is used only where its estimate with those bytes counted, ((header + data bits + 3 + 7) >> 3)
// + 4, is below the stored form's n + 5 (n + 10 at 65536); the stored form is written as non-final stored
// blocks with nothing after them.  Both stay within tile + 16.
//   link[] with a history.  The bounds argument above holds word for word with n read as m, the region's
// length: link[] has min(tile + hist rounded up to 4, 32768) entries behind the region's padding; a store is at
// p & 32767 with p < m <= tile + hist <= 65536; a load at c & 32767 with c < p; a history position enters
// itself and writes its entry like any other, so every c walked has written its entry; with m > 32768 the slot
// of c is reused by c + 32768, and the walk ends where c + 32768 < base + 64 as before.  Region bytes are read
// up to c + 258 + 3 < m + 16.  Nothing changes in the scratch (a token per tile byte at most: history
// positions give none) or in FC2_DEFLATE_TILE_BOUND.
//   Instantiations.  The history is a template parameter: <1, false> and <2, false> are the kernels above --
// the same instructions as before the history existed, one more (unread) kernel argument -- and `hist = 0`
// goes to them.  (A body shared by two kernels with the former arguments was tried: inlined there, the compiler
// orders and allocates it otherwise.)  Compiler's resource report for gfx950 (VGPRs, SGPRs, scratch; dynamic LDS
// only):
//   <1, false> 48, 72, 0    <2, false> 48, 72, 0    <1, true> 47, 74, 0    <2, true> 47, 78, 0
//   LDS with a history: 22540 B + (tile + hist rounded up to 4) + 16, and at level 2 two bytes more per
// position up to 32768.  Level 1: 8 KiB + 32 KiB 63516 B (two workgroups a CU), 32 KiB + 32 KiB 88092 B
// (one).  Level 2: 8 KiB + 32 KiB 129052 B, 32 KiB + 32 KiB 153628 B (one a CU both).
//
// Groups (deflate_kernel<level, true, true>, fc2_deflate_launch_groups; tests/deflate_model_groups.py is the rule
// in Python).  The launch's n bytes are cut into groups of `group` bytes, the last group holding the rest, and
// every group is a DEFLATE stream of its own cut into tiles: a BGZF block compressed by several wavefronts.  A
// whole group has tpg = ceil(group / tile) tiles, its last one holding the rest of the group; tiles are numbered
// densely, tile g * tpg + k is the k-th of group g, and only the last group can have fewer than tpg.  The kernel
// is the history's with three things derived from `group`: the tile's start g * group + k * tile, its history
// h = min(hist, k * tile) -- never a byte before the group's first, none for a group's first tile -- and `last`,
// true for the tile that ends its group (BFINAL = 1; every other tile in the non-final form above, with hist = 0
// too: a group is one stream whatever hist is).  Pass 1, the link[] bounds argument with m = h + n <= tile + hist,
// the Huffman and stored choice and the emission are the history's word for word.  One tile a group (tile >=
// group) is <level, false> at tile = group byte for byte; with hist > 0 a group's slots are
// fc2_deflate_launch_hist's over that group's bytes alone.
//   Scratch.  A tile's tokens lie at scratch + 4 * (its first byte's offset in src), at most one per byte of
// the tile: tiles cover disjoint bytes, so 4 * n_bytes suffice, which fc2_deflate_scratch_bytes(n_bytes, tile)
// is at least.  Slots, out_len and crc have fc2_deflate_group_tiles(n_bytes, group, tile) entries.
//   Instantiations.  <.., false> and <.., true> got one more unread kernel argument (`group`); their
// instructions are those from before the groups, compared in the compiler's output.  Resource report for
// gfx950 as above:   <1, true, true> 47, 74, 0    <2, true, true> 47, 78, 0
//   LDS by the formula above at tile 0x3fc0 with 32 KiB of history (region 49088 B): level 1 71644 B, two
// workgroups a CU; level 2 137180 B, one.
//
// Search effort (deflate_kernel<2, .., .., true>, fc2_deflate_launch_deep; tests/deflate_model_deep.py is the rule in
// Python).  Level 2's pass 1 with its two limits as kernel arguments, the same for every lane of every wavefront:
// `depth`, the candidates a position walks at most (1..128; level 2 itself: kDepth = 8), and `nice`, the kept length
// that ends the walk (4..258; level 2 itself: kNice = 32); one argument carries both, depth | nice << 16.  Nothing
// else differs: links written with the head read before the step's positions enter, the walk's ends (no candidate,
// over 32768 back, c + 32768 < base + 64), the first found among equal lengths, the cost rule, the lazy step and
// everything after pass 1 are level 2's, in all three shapes (independent tiles, history, groups).  At depth 8 and
// nice 32 the streams are level 2's byte for byte.  nice >= 258 leaves only the cap (min(258, m - p)) to end a walk
// early; nice = 4 ends it at the first candidate whose four bytes fit.
//   Bounds (link[]) for a walk of up to 128 candidates.  The argument above never used the 8.  It rests on two
// things.  The falling candidate: the first c is a head of an earlier step, c < p, and every further one is c - back
// with 1 <= back <= c checked before the subtraction, so c falls strictly, stays >= 0 and below p, and a walk ends
// after at most p steps whatever `depth` says -- the host refuses depth > 128, but no load depends on that.  The
// stale-slot stop: every c walked entered itself and wrote link[c & 32767]; that slot holds c's entry and not
// c + 32768's, because the walk ends before reading it where c + 32768 < base + 64 (the only positions entered after
// c that share its slot are >= c + 32768, and positions >= base + 64 have not been entered).  This is per candidate,
// not per walk, so it holds at the 9th and the 128th as at the 1st.  Loads of link[] are at c & 32767 < min(region
// rounded up to 4, 32768) since c < m; tile bytes are read up to c + 258 + 3 < m + 16.  The deep instantiations add
// no LDS (link[] is level 2's), no store to global memory, no scratch byte, and FC2_DEFLATE_TILE_BOUND is unchanged.
//   Divergence.  A wavefront's step takes as long as its lane with the longest walk: up to `depth` rounds of one
// LDS read of link[], two of the tile (load32u) and, where the four bytes fit, the extension.  Lanes whose walk has
// ended idle under the exec mask.  No cheaper schedule is tried here: the bytes are the model's.
//   Instantiations.  The six kernels above got one more unread kernel argument (`search`); their instructions are
// those of before, compared in the compiler's output (one symbol's name differs).  Resource report for gfx950
// as above:   <2, false, false, true> 48, 76, 0    <2, true, false, true> 47, 82, 0    <2, true, true, true> 47, 82, 0
//
// Priced passes (deflate_kernel<2, .., .., true, true>, fc2_deflate_launch_priced; tests/deflate_model_priced.py is the
// rule in Python).  The search above run 2 or 3 times over the same region, every pass after the first judging a match
// by the Huffman code the pass before it produced.  `search` carries the number too: depth | nice << 16 | passes << 28
// (depth <= 128 and nice <= 258 leave bits 25..31 free), wave-uniform like the other two.
//   Pass 1 is the search effort's pass 1, lit16 and all.  After a pass that is not the last: lfreq[256] = 1, then
// build_code(lfreq, 286, 15) and build_code(dfreq, 30, 15) exactly as they run after the last pass -- dummy symbols,
// overflow repair -- but no code-length code and no header.  If either is not ok (not expected) no further pass runs
// and the tile goes on below with the tokens it has.  Else the heads are zeroed (the code builder's workspace lay in
// them), the two histograms are zeroed, ntok = 0, extra = 0, skip = h, and the pass loop runs again from base = 0,
// writing its tokens over the scratch: the last pass's tokens are the ones emitted, nothing compares passes, and the
// stored form still bounds the tile.
//   The one difference of a pass k >= 2 is the cost rule.  With llen and dlen as the last build_code left them,
// lit(b) = llen[b], or 15 where that is 0; match(l, d) = (llen[length symbol] or 15) + the length's extra bits +
// (dlen[distance symbol] or 15) + the distance's extra bits.  The walk's kept match -- the longest, the first found among
// equals, the same three ends, `nice` and the cap -- is a found match iff the sum of lit over its `best` bytes at
// p .. p + best - 1 is strictly more than match(best, bestd); lit16 is not consulted.  A match costs at most 15 + 5 +
// 15 + 13 = 48 bits and a literal at least 1, so the sum stops once it is over 48 (at most 49 bytes, all below p + best
// <= m) without changing the answer.  Links, the lazy step, the greedy resolution and history positions that enter but
// never search are the same code as in pass 1.
//   No LDS is added: llen and dlen stay where they are until the next build_code overwrites them, which is after the
// pass that read them; lcode and dcode are written between passes and read only after the last.  No store to global
// memory is added beyond the token scratch the tile owns already (at most one token a tile byte, in every pass);
// FC2_DEFLATE_TILE_BOUND is unchanged.
//   Bounds (link[]) in a pass that runs again.  link[] is not cleared between passes and does not need to be: the
// argument above holds per pass once the heads are zero.  With empty heads a pass reads as a first candidate only a
// head an earlier step of this pass entered, and every further candidate is c - link[c & 32767] with c a position
// walked in this pass; every position of this pass that can be a head or be reached from one wrote its entry in this
// pass where it entered itself, before any later step reads it.  So every entry read was written in this pass, and an
// entry left by the pass before is either overwritten (positions enter in the same order, at the same slots, in every
// pass: the same p & 32767 for the same p) or never read.  In a region over 32768 bytes, where slots are reused inside
// one pass, the stale-slot stop is what it was: the slot of c holds c's entry of this pass unless c + 32768 has entered,
// and the walk ends before reading it where c + 32768 < base + 64.  The falling candidate (c < p, back <= c checked
// before the subtraction) bounds every load as above: link[] at c & 32767 < min(region rounded up to 4, 32768), region
// bytes up to c + 258 + 3 < m + 16.  (tests/test_gpu_deflate_priced.py runs deflate_deep_inputs.stale_chain in a region
// of 65536 bytes with two passes.)
//   Instantiations.  The nine kernels above are the same template with kPriced = false: the pass loop is a do-while
// whose condition is the template parameter, and nothing in it is instantiated for them.  Compared in the compiler's
// output against the parent's: the same instructions in each of the nine (11849 .. 12125 of them), in the same order
// but for one to three neighbouring register moves (v_mov_b32 0, s_mov_b64 0, one v_cndmask_b32) that the scheduler
// places one or two slots earlier or later in <2, false>, <2, true, true>, <2, true, true, true> and <2, false, false,
// true>; the other five are identical line for line (symbol names apart).  Same registers as reported above.  Resource
// report for gfx950 as above:
//   <2, false, false, true, true> 70, 104, 0    <2, true, false, true, true> 70, 104, 0    <2, true, true, true, true> 70, 104, 0
// (one workgroup a CU by its LDS at every tile over some 19 KiB, as level 2: the registers do not limit it).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <string>

#include "../../include/fc2_caller.h"
#include "fc2_common.h"
#include "fc2_devcrc.h"

namespace {

constexpr uint32_t kTileMax = 65536;
constexpr int kHashBits = 12;
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr uint32_t kLinks = 32768;             // level 2: link[] slots (a power of two: the window)
constexpr int kDepth = 8;                      // level 2: candidates a position walks at most
constexpr uint32_t kNice = 32;                 // level 2: a kept length that ends the walk
constexpr uint32_t kStageWords = 768;          // 3 KiB: flushed once 2 KiB are full; a step adds < 400 bytes
constexpr uint32_t kStageFlush = 2048;
constexpr uint32_t kTokMatch = 0x80000000u;    // token: a literal's byte, or this | (len - 3) << 16 | (dist - 1)
constexpr uint32_t kFailed = 0xFFFFFFFFu;      // out_len of a tile the kernel gave up on (the host compresses it)

__constant__ uint8_t kDClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Lds {
    uint32_t htab[1 << kHashBits];             // last position + 1 per hash; then the code builder's workspace
    uint32_t stage[kStageWords];
    uint32_t lfreq[288], dfreq[32], cfreq[20]; // (lfreq: the bytes' histogram first, then literal/length symbols)
    uint32_t blc[16];
    uint16_t lcode[288], dcode[32], ccode[20]; // codewords, bit-reversed: as they go into the stream
    uint16_t rle[320];                         // the code lengths' run-length form: symbol | extra << 8
    uint8_t llen[288], dlen[32], clen[20];
    uint32_t tile[1];                          // the tile's bytes and 16 bytes of zeros (dynamic)
};

// the code builder's workspace inside htab (m <= 286 symbols in use: 2 m - 1 nodes)
struct Work {
    uint32_t w[576];
    uint16_t par[576], sorted[288];
    uint8_t dep[576];
};
static_assert(sizeof(Work) <= sizeof(uint32_t) << kHashBits, "the code builder works in the hash table");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// 4 bytes at any byte offset of the tile (little-endian), from two aligned words
__device__ __forceinline__ uint32_t load32u(const uint32_t *t, uint32_t p) {
    const uint32_t k = p >> 2;
    const uint64_t v = (uint64_t)t[k] | ((uint64_t)t[k + 1] << 32);
    return (uint32_t)(v >> ((p & 3u) * 8u));
}

// 16 log2(x), x >= 1: the mantissa's top four bits stand for the fraction
__device__ __forceinline__ uint32_t log2x16(uint32_t x) {
    const uint32_t m = 31u - (uint32_t)__clz((int)x);
    return 16u * m + (((x << (31u - m)) >> 27) & 15u);
}

// length l = len - 3 (0..255): its symbol, extra-bit count and extra bits (RFC 1951 3.2.5)
__device__ __forceinline__ void len_sym(uint32_t l, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    if (l < 8u) { sym = 257u + l; eb = 0; ev = 0; return; }
    if (l == 255u) { sym = 285u; eb = 0; ev = 0; return; }
    eb = 29u - (uint32_t)__clz((int)l);
    sym = 261u + 4u * eb + ((l >> eb) & 3u);
    ev = l & ((1u << eb) - 1u);
}
// distance d = dist - 1 (0..32767)
__device__ __forceinline__ void dist_sym(uint32_t d, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    if (d < 4u) { sym = d; eb = 0; ev = 0; return; }
    const uint32_t m = 31u - (uint32_t)__clz((int)d);
    eb = m - 1u;
    sym = 2u * m + ((d >> eb) & 1u);
    ev = d & ((1u << eb) - 1u);
}

// Code lengths <= maxbits for the n symbols' frequencies (a Huffman code, repaired as zlib's
// gen_bitlen does when the tree is deeper), and the bit-reversed canonical codewords.  A code with
// fewer than two symbols in use gets dummy ones (symbols 0 / 1, frequency 1; zlib's build_tree), so
// it is always complete.  False if the lengths do not add up to a complete code (not expected).
__device__ bool build_code(uint32_t *freq, int n, int maxbits, uint8_t *lens, uint16_t *code, uint32_t *blc, Work &W,
                           int lane) {
    __syncthreads();
    uint32_t used = 0;
    for (int b = 0; b < n; b += 64) {
        const int s = b + lane;
        used += (uint32_t)__popcll(__ballot(s < n && freq[s] != 0));
    }
    if (used < 2u && lane == 0) {
        if (freq[0] == 0) { freq[0] = 1; ++used; }
        if (used < 2u) freq[1] = 1;            // (freq[1] is 0 here: otherwise two were in use)
    }
    used = used < 2u ? 2u : used;
    const int m = (int)used;
    for (int s = lane; s < n; s += 64) lens[s] = 0;
    if (lane < 16) blc[lane] = 0;
    __syncthreads();
    // the symbols in use in ascending order of (frequency, symbol): each lane ranks its own
    for (int s = lane; s < n; s += 64) {
        const uint32_t f = freq[s];
        if (!f) continue;
        uint32_t r = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t g = freq[j];
            r += (g != 0 && (g < f || (g == f && j < s))) ? 1u : 0u;
        }
        W.sorted[r] = (uint16_t)s;
        W.w[r] = f;
    }
    __syncthreads();
    bool ok = true;
    if (lane == 0) {
        // leaves 0..m-1 in order, inner nodes m..2m-2 in the order they are made (their weights rise too)
        int i = 0, j = m;
        for (int k = m; k < 2 * m - 1; ++k) {
            uint32_t sum = 0;
            for (int t = 0; t < 2; ++t) {
                int pick;
                if (i < m && (j >= k || W.w[i] <= W.w[j])) pick = i++;
                else pick = j++;
                sum += W.w[pick];
                W.par[pick] = (uint16_t)k;
            }
            W.w[k] = sum;
        }
        // depths from the root down, cut at maxbits (overflow counts the nodes cut)
        int overflow = 0;
        W.dep[2 * m - 2] = 0;
        for (int k = 2 * m - 3; k >= 0; --k) {
            int d = (int)W.dep[W.par[k]] + 1;
            if (d > maxbits) { d = maxbits; ++overflow; }
            W.dep[k] = (uint8_t)d;
            if (k < m) ++blc[d];
        }
        while (overflow > 0) {                  // move a leaf down the tree, a leaf of the last level up
            int bits = maxbits - 1;
            while (bits > 0 && blc[bits] == 0) --bits;
            if (bits == 0) break;
            --blc[bits];
            blc[bits + 1] += 2;
            --blc[maxbits];
            overflow -= 2;
        }
        uint32_t kraft = 0, total = 0;
        for (int b = 1; b <= maxbits; ++b) {
            kraft += blc[b] << (maxbits - b);
            total += blc[b];
        }
        ok = kraft == (1u << maxbits) && total == (uint32_t)m;
        if (ok) {
            int idx = 0;                        // the rarest symbols get the longest codewords
            for (int b = maxbits; b >= 1; --b)
                for (uint32_t c = 0; c < blc[b]; ++c) lens[W.sorted[idx++]] = (uint8_t)b;
            uint32_t next[16];
            uint32_t c = 0;
            next[0] = 0;
            for (int b = 1; b <= maxbits; ++b) {
                c = (c + (b > 1 ? blc[b - 1] : 0u)) << 1;
                next[b] = c;
            }
            for (int s = 0; s < n; ++s) {
                const uint32_t l = lens[s];
                code[s] = l ? (uint16_t)(__builtin_bitreverse32(next[l]++) >> (32u - l)) : (uint16_t)0;
            }
        }
    }
    ok = uni(ok ? 1u : 0u) != 0;
    __syncthreads();
    return ok;
}

// the stream's bytes as they are staged: coordinate c = the destination's low four address bits + the
// byte's index in the stream, so that staged 16-byte pieces are aligned 16-byte pieces of HBM
struct Out {
    uint8_t *base;                             // slot - a (16-byte aligned; bytes before `a` are never touched)
    uint32_t a;                                // the first coordinate
    uint32_t limit;                            // a + FC2_DEFLATE_TILE_BOUND(tile): no store at or past it
    uint32_t stage0;                           // coordinate of stage[0]'s first byte (a multiple of 16)
    uint64_t bit;                              // the next bit's position, 8 a + bits so far
    bool over;
};

// staged coordinates [stage0, upto) to HBM; bytes outside [a, min(upto, limit)) are not stored
__device__ void store_pieces(const Lds &L, Out &o, uint32_t upto, int lane) {
    const uint32_t end = upto < o.limit ? upto : o.limit;
    if (upto > o.limit) o.over = true;
    for (uint32_t c0 = o.stage0 + 16u * (uint32_t)lane; c0 < end; c0 += 1024u) {
        const uint32_t wi = (c0 - o.stage0) >> 2;
        const uint4 v = make_uint4(L.stage[wi], L.stage[wi + 1], L.stage[wi + 2], L.stage[wi + 3]);
        if (c0 >= o.a && c0 + 16u <= end) {
            *reinterpret_cast<uint4 *>(o.base + c0) = v;
        } else {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint32_t lo = c0 > o.a ? c0 : o.a, hi = c0 + 16u < end ? c0 + 16u : end;
            for (uint32_t c = lo; c < hi; ++c) o.base[c] = (uint8_t)(w[(c - c0) >> 2] >> (8u * (c & 3u)));
        }
    }
}

// whole staged 16-byte pieces to HBM once 2 KiB are full; the unfinished piece moves to the front
__device__ void flush_stage(Lds &L, Out &o, int lane) {
    const uint32_t bytes = (uint32_t)(o.bit >> 3);       // whole bytes so far, as a coordinate
    if (bytes - o.stage0 < kStageFlush) return;
    __syncthreads();
    const uint32_t upto = bytes & ~15u;
    store_pieces(L, o, upto, lane);
    const uint32_t wi = (upto - o.stage0) >> 2;
    const uint32_t keep = lane < 8 ? L.stage[wi + (uint32_t)lane] : 0u;   // (< 16 bytes and a part of one are left)
    __syncthreads();
    for (uint32_t k = (uint32_t)lane; k < kStageWords; k += 64) L.stage[k] = 0;
    __syncthreads();
    if (lane < 8) L.stage[lane] = keep;
    o.stage0 = upto;
    __syncthreads();
}

// nb <= 57 bits of v at the stream's bit position `at` (a position, not a coordinate in the stage)
__device__ __forceinline__ void or_bits(Lds &L, const Out &o, uint64_t at, uint64_t v, uint32_t nb) {
    if (!nb) return;
    const uint32_t rel = (uint32_t)(at - (uint64_t)o.stage0 * 8u);
    const uint32_t wi = rel >> 5, sh = rel & 31u;
    const uint32_t w0 = (uint32_t)(v << sh), w1 = (uint32_t)((v << sh) >> 32);
    const uint32_t w2 = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
    if (wi + 2u >= kStageWords) return;        // (cannot happen: a flush leaves a KiB free)
    if (w0) atomicOr(&L.stage[wi], w0);
    if (w1) atomicOr(&L.stage[wi + 1], w1);
    if (w2) atomicOr(&L.stage[wi + 2], w2);
}

// one lane's bit writer (the block header)
__device__ __forceinline__ void put(Lds &L, Out &o, uint32_t v, uint32_t nb) {
    or_bits(L, o, o.bit, (uint64_t)v, nb);
    o.bit += nb;
}

// kHist: the launch is one DEFLATE stream, and a tile has the `hist` bytes before it in front of it in LDS
// (the header's "History"); without it `hist` is not looked at.  kGroups (with kHist): the launch is cut into
// groups of `group` bytes, each a stream of its own whose tiles see only their group (the header's "Groups");
// without it `group` is not looked at.
// kDeep (level 2 only): the walk's two limits are kernel arguments, `search` = depth | nice << 16 (the header's
// "Search effort"); without it `search` is not looked at and the limits are kDepth and kNice.
// kPriced (with kDeep): `search` carries a number of passes too, depth | nice << 16 | passes << 28, and every pass after
// the first takes a match by its price in the code the pass before gave (the header's "Priced passes"); without it
// there is one pass and those bits are not looked at.
template <int kLevel, bool kHist, bool kGroups = false, bool kDeep = false, bool kPriced = false>
__global__ __launch_bounds__(64) void deflate_kernel(const uint8_t *__restrict__ src, uint64_t n_bytes, uint32_t tile,
                                                     uint8_t *__restrict__ dst, uint32_t stride,
                                                     uint32_t *__restrict__ out_len, uint32_t *__restrict__ crc,
                                                     uint32_t *__restrict__ scratch, uint32_t hist, uint32_t group,
                                                     uint32_t search) {
    static_assert(kHist || !kGroups, "groups are built on the history's kernel");
    static_assert(kLevel == 2 || !kDeep, "the search effort is level 2's");
    static_assert(kDeep || !kPriced, "priced passes are built on the search effort's kernel");
    extern __shared__ __align__(16) uint8_t smem[];
    Lds &L = *reinterpret_cast<Lds *>(smem);
    uint32_t *T = L.tile;
    uint16_t *link = nullptr;                  // level 2's links, behind the tile and its 16 bytes of padding (lds_bytes)
    if constexpr (kLevel == 2) {
        if constexpr (kHist) link = reinterpret_cast<uint16_t *>(smem + offsetof(Lds, tile) + ((tile + hist + 3u) & ~3u) + 16u);
        else link = reinterpret_cast<uint16_t *>(smem + offsetof(Lds, tile) + ((tile + 3u) & ~3u) + 16u);
    }
    const uint32_t blk = blockIdx.x;
    const int lane = (int)threadIdx.x;
    uint64_t start = (uint64_t)blk * tile;
    uint64_t from = 0, upto = n_bytes;          // the stream the tile belongs to: the launch, or its group
    if constexpr (kGroups) {
        const uint32_t tpg = (group - 1u) / tile + 1u;      // tiles of a whole group: tile g * tpg + k is group g's k-th
        const uint32_t g = blk / tpg, k = blk - g * tpg;
        from = (uint64_t)g * group;
        start = from + (uint64_t)k * tile;
        if (from + group < upto) upto = from + group;
    }
    if (start >= upto) return;
    const uint32_t n = (uint32_t)(upto - start < (uint64_t)tile ? upto - start : (uint64_t)tile);   // 1..65536
    // the region in LDS: h bytes of history, then the tile; m bytes, positions counted from the history's first
    uint32_t h = 0;
    if constexpr (kHist) h = (uint32_t)(start - from < (uint64_t)hist ? start - from : (uint64_t)hist);
    const uint32_t m = h + n;                   // 1..65536
    const bool last = !kHist || start + n >= upto;      // written as a stream of its own: BFINAL, nothing after it
    const uint8_t *in = src + start - h;
    uint8_t *slot = dst + (uint64_t)blk * stride;
    uint32_t *tok = scratch + start;           // n tokens at most

    // ---- the tile into LDS, its bytes' histogram and its CRC-32 ---------------------------------
    for (uint32_t k = (uint32_t)lane; k < (1u << kHashBits); k += 64) L.htab[k] = 0;
    for (uint32_t k = (uint32_t)lane; k < kStageWords; k += 64) L.stage[k] = 0;
    for (uint32_t k = (uint32_t)lane; k < 288u; k += 64) L.lfreq[k] = 0;
    if (lane < 32) L.dfreq[lane] = 0;
    if (lane < 20) L.cfreq[lane] = 0;
    const uint32_t nw = (m + 3u) >> 2;         // words holding the region; four more are zeroed
    __syncthreads();
    if (((uintptr_t)in & 15u) == 0) {
        for (uint32_t b0 = 16u * (uint32_t)lane; b0 < m; b0 += 1024u) {
            if (b0 + 16u <= m) {
                const uint4 v = *reinterpret_cast<const uint4 *>(in + b0);
                T[b0 >> 2] = v.x; T[(b0 >> 2) + 1] = v.y; T[(b0 >> 2) + 2] = v.z; T[(b0 >> 2) + 3] = v.w;
            } else {
                for (uint32_t w = 0; w < 4u; ++w) {
                    uint32_t v = 0;
                    for (uint32_t i = 0; i < 4u; ++i) {
                        const uint32_t p = b0 + 4u * w + i;
                        if (p < m) v |= (uint32_t)in[p] << (8u * i);
                    }
                    T[(b0 >> 2) + w] = v;      // (words up to nw + 3 at most: inside the 16 bytes of padding)
                }
            }
        }
    } else {
        for (uint32_t k = (uint32_t)lane; k < nw; k += 64) {
            uint32_t v = 0;
            for (uint32_t i = 0; i < 4u; ++i) {
                const uint32_t p = 4u * k + i;
                if (p < m) v |= (uint32_t)in[p] << (8u * i);
            }
            T[k] = v;
        }
    }
    __syncthreads();
    if (lane < 4) T[nw + (uint32_t)lane] = 0;
    __syncthreads();
    for (uint32_t k = (uint32_t)lane; k < nw; k += 64) {
        const uint32_t v = T[k];
        for (uint32_t i = 0; i < 4u; ++i)
            if (4u * k + i >= h && 4u * k + i < m) atomicAdd(&L.lfreq[(v >> (8u * i)) & 255u], 1u);
    }
    uint32_t R = 0;                             // raw CRC, in rows of 1024 bytes as the inflater's
    uint32_t done = 0;
    for (; done + 1024u <= n; done += 1024u) {
        uint32_t c;
        if constexpr (kHist) {                  // (the tile's own bytes: at any byte offset of the region)
            const uint32_t q = h + done + 16u * (uint32_t)lane;
            c = crc_word(crc_word(crc_word(crc_word(0u, load32u(T, q)), load32u(T, q + 4u)), load32u(T, q + 8u)), load32u(T, q + 12u));
        } else {
            const uint32_t k = (done >> 2) + 4u * (uint32_t)lane;
            c = crc_word(crc_word(crc_word(crc_word(0u, T[k]), T[k + 1]), T[k + 2]), T[k + 3]);
        }
        R = multmodp(kX2n[13], R) ^ wave_fold(c);
    }
    for (; done < n; ++done) {                  // the last, short row byte by byte, on every lane alike
        R ^= (T[(h + done) >> 2] >> (8u * ((h + done) & 3u))) & 255u;
#pragma unroll
        for (int b = 0; b < 8; ++b) R = mulx(R);
    }
    const uint32_t tile_crc = R ^ multmodp(x8n(n), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
    __syncthreads();

    // what a literal costs on average, in 1/16 bit: the bytes' entropy, at least a bit each
    uint32_t cost = 0;
    const uint32_t ln = log2x16(n);
    for (uint32_t s = (uint32_t)lane; s < 256u; s += 64) {
        const uint32_t f = L.lfreq[s];
        if (f) {
            const uint32_t c = ln - log2x16(f);
            cost += f * (c < 16u ? 16u : c);
        }
    }
    for (int s = 1; s < 64; s <<= 1) cost += (uint32_t)__shfl_xor((int)cost, s);
    const uint32_t lit16 = uni(cost) / n;       // >= 16
    __syncthreads();
    for (uint32_t k = (uint32_t)lane; k < 288u; k += 64) L.lfreq[k] = 0;
    __syncthreads();

    // ---- pass 1: matches, tokens, histograms ------------------------------------------------------
    uint32_t ntok = 0, skip = h;                // tokens so far; positions below `skip` are inside a match, or history
    uint32_t extra = 0;                         // this lane's tokens' extra bits
    uint32_t pass = 1;                          // (kPriced: the pass running, wave-uniform)
    do {
        for (uint32_t base = 0; base < m; base += 64) {
            const uint32_t p = base + (uint32_t)lane;
            const bool can = p + kMinMatch <= m;
            const uint32_t v = load32u(T, p < m ? p : 0u);
            const uint32_t h = (v * 2654435761u) >> (32 - kHashBits);
            const uint32_t cand = can ? L.htab[h] : 0u;
            __syncthreads();
            if (can) atomicMax(&L.htab[h], p + 1u);
            if constexpr (kLevel == 2) {
                if (can) link[p & (kLinks - 1u)] = (uint16_t)(cand && p + 1u - cand <= kMaxDist ? p + 1u - cand : 0u);
            }
            __syncthreads();
            if (skip >= base + 64u) continue;       // (uniform) the whole step lies inside a match
            uint32_t mlen = 0, mdist = 0;
            if constexpr (kLevel == 2) {
                if (cand && p >= skip) {
                    const uint32_t maxlen = m - p < kMaxMatch ? m - p : kMaxMatch;
                    uint32_t c = cand - 1u, best = 0, bestd = 0;
                    // (kDeep: wave-uniform limits from the kernel argument, in place of the constants)
                    for (int k = 0; k < (kDeep ? (int)(search & 0xFFFFu) : kDepth); ++k) {
                        const uint32_t d = p - c;
                        if (d > kMaxDist || c + kLinks < base + 64u) break;
                        if (load32u(T, c) == v) {
                            uint32_t l = 4;
                            while (l < maxlen) {
                                const uint32_t x = load32u(T, c + l) ^ load32u(T, p + l);
                                if (x) {
                                    l += (uint32_t)(__ffs((int)x) - 1) >> 3;
                                    break;
                                }
                                l += 4;
                            }
                            l = l < maxlen ? l : maxlen;
                            if (l > best) {
                                best = l;
                                bestd = d;
                            }
                            if (best >= (kPriced ? (search >> 16) & 0x1FFu : kDeep ? search >> 16 : kNice) || best >= maxlen) break;
                        }
                        const uint32_t back = link[c & (kLinks - 1u)];
                        if (!back || back > c) break;   // (back <= c: it points at a position of the tile)
                        c -= back;
                    }
                    bool priced = false;
                    if constexpr (kPriced) priced = pass > 1u;
                    if (priced) {
                        // the match's bits in the last pass's code against its bytes' as literals; a symbol without
                        // a codeword counts 15.  A match costs 48 bits at most and a literal one at least, so the sum
                        // stops once it is over 48: at most 49 bytes are read, all below p + best <= m.
                        if (best) {
                            uint32_t s, eb, ev;
                            len_sym(best - 3u, s, eb, ev);
                            uint32_t price = (L.llen[s] ? L.llen[s] : 15u) + eb;
                            dist_sym(bestd - 1u, s, eb, ev);
                            price += (L.dlen[s] ? L.dlen[s] : 15u) + eb;
                            uint32_t lits = 0;
                            for (uint32_t i = 0; i < best && lits <= 48u; ++i) {
                                const uint32_t b = (T[(p + i) >> 2] >> (8u * ((p + i) & 3u))) & 255u;
                                lits += L.llen[b] ? L.llen[b] : 15u;
                            }
                            if (lits > price) {
                                mlen = best;
                                mdist = bestd;
                            }
                        }
                    } else if (best) {
                        const uint32_t deb = bestd > 4u ? 30u - (uint32_t)__clz((int)(bestd - 1u)) : 0u;
                        if (best * lit16 >= 16u * (11u + deb)) {
                            mlen = best;
                            mdist = bestd;
                        }
                    }
                }
            } else if (cand && p >= skip) {
                const uint32_t c = cand - 1u;       // < p: positions of earlier steps only
                const uint32_t d = p - c;
                if (d <= kMaxDist && load32u(T, c) == v) {
                    const uint32_t maxlen = m - p < kMaxMatch ? m - p : kMaxMatch;
                    uint32_t l = 4;
                    while (l < maxlen) {
                        const uint32_t x = load32u(T, c + l) ^ load32u(T, p + l);
                        if (x) {
                            l += (uint32_t)(__ffs((int)x) - 1) >> 3;
                            break;
                        }
                        l += 4;
                    }
                    l = l < maxlen ? l : maxlen;
                    // worth it if the length and distance codes (about 11 bits and the distance's extra
                    // bits) cost less than the bytes as literals
                    const uint32_t deb = d > 4u ? 30u - (uint32_t)__clz((int)(d - 1u)) : 0u;
                    if (l >= kMinMatch && l * lit16 >= 16u * (11u + deb)) {
                        mlen = l;
                        mdist = d;
                    }
                }
            }
            const uint64_t found = __ballot(mlen != 0);
            uint64_t starts = 0;                    // lanes whose match is taken
            uint64_t cov = skip > base ? (1ull << (skip - base)) - 1ull : 0ull;   // lanes inside a match
            uint32_t cur = skip > base ? skip - base : 0u;                        // < 64
            while (cur < 64u) {
                const uint64_t mm = found & ~((1ull << cur) - 1ull);
                if (!mm) break;
                const uint32_t l = (uint32_t)__ffsll((long long)mm) - 1u;
                const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)l);
                if constexpr (kLevel == 2) {        // a longer match one position on: this one is a literal
                    if (l + 1u < 64u && ((found >> (l + 1u)) & 1ull) &&
                        (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)((l + 1u) & 63u)) > len) {
                        cur = l + 1u;
                        continue;
                    }
                }
                starts |= 1ull << l;
                const uint32_t e = l + len;         // the first position after the match
                const uint64_t upto = e >= 64u ? ~0ull : (1ull << e) - 1ull;
                cov |= upto & ~((2ull << l) - 1ull);
                cur = e;
                skip = base + e;
            }
            const bool emit = p < m && !((cov >> lane) & 1ull);
            const uint64_t em = __ballot(emit);
            if (emit) {
                const uint32_t at = ntok + (uint32_t)__popcll(em & ((1ull << lane) - 1ull));
                if ((starts >> lane) & 1ull) {
                    tok[at] = kTokMatch | ((mlen - 3u) << 16) | (mdist - 1u);
                    uint32_t s, eb, ev;
                    len_sym(mlen - 3u, s, eb, ev);
                    atomicAdd(&L.lfreq[s], 1u);
                    extra += eb;
                    dist_sym(mdist - 1u, s, eb, ev);
                    atomicAdd(&L.dfreq[s], 1u);
                    extra += eb;
                } else {
                    tok[at] = v & 255u;
                    atomicAdd(&L.lfreq[v & 255u], 1u);
                }
            }
            ntok += (uint32_t)__popcll(em);
        }
        if constexpr (kPriced) {
            // a pass that is not the last: the two codes of its histograms, built as after the last one; then the heads
            // (the code builder worked in them) and the histograms are zeroed and pass 1 runs again over the same
            // region, writing its tokens over the scratch.  llen and dlen stay until the next build_code, after the
            // pass that reads them.  A code that is not ok (not expected) ends the passes: the tile goes on below.
            if (pass >= search >> 28) break;
            if (lane == 0) L.lfreq[256] = 1;
            Work &W = *reinterpret_cast<Work *>(L.htab);
            bool again = build_code(L.lfreq, 286, 15, L.llen, L.lcode, L.blc, W, lane);
            again = build_code(L.dfreq, 30, 15, L.dlen, L.dcode, L.blc, W, lane) && again;
            if (!again) break;
            for (uint32_t k = (uint32_t)lane; k < (1u << kHashBits); k += 64) L.htab[k] = 0;
            for (uint32_t k = (uint32_t)lane; k < 288u; k += 64) L.lfreq[k] = 0;
            if (lane < 32) L.dfreq[lane] = 0;
            ntok = 0;
            skip = h;
            extra = 0;
            ++pass;
            __syncthreads();
        }
    } while (kPriced);
    for (int s = 1; s < 64; s <<= 1) extra += (uint32_t)__shfl_xor((int)extra, s);
    extra = uni(extra);
    if (lane == 0) L.lfreq[256] = 1;            // the end of the block
    __threadfence_block();                      // the tokens, visible to the lanes that read them back
    __syncthreads();

    // ---- the codes ----------------------------------------------------------------------------------
    Work &W = *reinterpret_cast<Work *>(L.htab);
    bool ok = build_code(L.lfreq, 286, 15, L.llen, L.lcode, L.blc, W, lane);
    ok = build_code(L.dfreq, 30, 15, L.dlen, L.dcode, L.blc, W, lane) && ok;
    uint32_t data_bits = lane == 0 ? extra : 0u;   // the block's symbols (dummy symbols counted: an upper bound)
    for (uint32_t s = (uint32_t)lane; s < 286u; s += 64) data_bits += L.lfreq[s] * L.llen[s];
    if (lane < 30) data_bits += L.dfreq[lane] * L.dlen[lane];
    for (int s = 1; s < 64; s <<= 1) data_bits += (uint32_t)__shfl_xor((int)data_bits, s);
    data_bits = uni(data_bits);

    // the code lengths in run-length form (symbols 16, 17, 18), by one lane
    uint32_t hlit = 286, hdist = 30, nrle = 0;
    if (lane == 0 && ok) {
        while (hlit > 257u && L.llen[hlit - 1u] == 0) --hlit;
        while (hdist > 1u && L.dlen[hdist - 1u] == 0) --hdist;
        const uint32_t total = hlit + hdist;
        uint32_t k = 0;
        while (k < total) {
            const uint32_t val = k < hlit ? L.llen[k] : L.dlen[k - hlit];
            uint32_t run = 1;
            while (k + run < total && (k + run < hlit ? L.llen[k + run] : L.dlen[k + run - hlit]) == val) ++run;
            k += run;
            if (val == 0) {
                while (run >= 11u) {
                    const uint32_t r = run < 138u ? run : 138u;
                    L.rle[nrle++] = (uint16_t)(18u | ((r - 11u) << 8));
                    ++L.cfreq[18];
                    run -= r;
                }
                if (run >= 3u) {
                    L.rle[nrle++] = (uint16_t)(17u | ((run - 3u) << 8));
                    ++L.cfreq[17];
                    run = 0;
                }
            } else {
                L.rle[nrle++] = (uint16_t)val;
                ++L.cfreq[val];
                --run;
                while (run >= 3u) {
                    const uint32_t r = run < 6u ? run : 6u;
                    L.rle[nrle++] = (uint16_t)(16u | ((r - 3u) << 8));
                    ++L.cfreq[16];
                    run -= r;
                }
            }
            for (; run; --run) {
                L.rle[nrle++] = (uint16_t)val;
                ++L.cfreq[val];
            }
        }
    }
    hlit = uni(hlit);
    hdist = uni(hdist);
    nrle = uni(nrle);
    ok = build_code(L.cfreq, 19, 7, L.clen, L.ccode, L.blc, W, lane) && ok;

    // ---- the stream ---------------------------------------------------------------------------------
    Out o;
    o.a = (uint32_t)((uintptr_t)slot & 15u);
    o.base = slot - o.a;
    o.limit = o.a + FC2_DEFLATE_TILE_BOUND(tile);
    o.stage0 = 0;
    o.bit = 8ull * o.a;
    o.over = false;
    const uint32_t stored_bytes = n + (n > 65535u ? 10u : 5u);
    if (lane == 0 && ok) {                      // the block's header
        put(L, o, (last ? 1u : 0u) | (2u << 1), 3);   // BFINAL, dynamic codes
        uint32_t hclen = 19;
        while (hclen > 4u && L.clen[kDClOrder[hclen - 1u]] == 0) --hclen;
        put(L, o, hlit - 257u, 5);
        put(L, o, hdist - 1u, 5);
        put(L, o, hclen - 4u, 4);
        for (uint32_t k = 0; k < hclen; ++k) put(L, o, L.clen[kDClOrder[k]], 3);
        for (uint32_t k = 0; k < nrle; ++k) {
            const uint32_t s = L.rle[k] & 255u, e = L.rle[k] >> 8;
            put(L, o, L.ccode[s], L.clen[s]);
            if (s >= 16u) put(L, o, e, s == 16u ? 2u : s == 17u ? 3u : 7u);
        }
    }
    o.bit = ((uint64_t)uni((uint32_t)(o.bit >> 32)) << 32) | uni((uint32_t)o.bit);
    __syncthreads();
    // (a tile that is not the last: the empty stored block behind it counted, 3 bits, the padding and 4 bytes)
    const uint32_t dyn_bytes = last ? (uint32_t)((o.bit - 8ull * o.a + data_bits + 7u) >> 3)
                                    : (uint32_t)((o.bit - 8ull * o.a + data_bits + 3u + 7u) >> 3) + 4u;
    uint32_t len;
    if (ok && dyn_bytes < stored_bytes) {
        for (uint32_t b0 = 0; b0 < ntok; b0 += 64) {
            const uint32_t k = b0 + (uint32_t)lane;
            uint64_t bits = 0;
            uint32_t nb = 0;
            if (k < ntok) {
                const uint32_t t = tok[k];
                if (t & kTokMatch) {
                    uint32_t s, eb, ev;
                    len_sym((t >> 16) & 255u, s, eb, ev);
                    bits = L.lcode[s];
                    nb = L.llen[s];
                    bits |= (uint64_t)ev << nb;
                    nb += eb;
                    dist_sym(t & 0x7FFFu, s, eb, ev);
                    bits |= (uint64_t)L.dcode[s] << nb;
                    nb += L.dlen[s];
                    bits |= (uint64_t)ev << nb;
                    nb += eb;                   // <= 15 + 5 + 15 + 13
                } else {
                    bits = L.lcode[t];
                    nb = L.llen[t];
                }
            }
            uint32_t incl = nb;                 // the bit counts' prefix sum over the lanes
            for (int s = 1; s < 64; s <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, (unsigned)s);
                if (lane >= s) incl += up;
            }
            or_bits(L, o, o.bit + (incl - nb), bits, nb);
            o.bit += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            flush_stage(L, o, lane);
        }
        if (lane == 0) or_bits(L, o, o.bit, L.lcode[256], L.llen[256]);
        o.bit += L.llen[256];
        if constexpr (kHist) {
            if (!last) {                        // bits 000, zeros to the byte boundary, 00 00 FF FF
                o.bit = (o.bit + 3u + 7u) & ~7ull;
                if (lane == 0) or_bits(L, o, o.bit, 0xFFFF0000ull, 32);
                o.bit += 32u;
            }
        }
        __syncthreads();
        const uint32_t end = (uint32_t)((o.bit + 7u) >> 3);
        store_pieces(L, o, end, lane);
        len = end - o.a;
        if (o.over || len > FC2_DEFLATE_TILE_BOUND(tile)) len = kFailed;
    } else {
        // stored: one block, or 65535 bytes and the last one (LEN is 16 bits); byte k of the stream
        for (uint32_t k = (uint32_t)lane; k < stored_bytes; k += 64) {
            const uint32_t first = n > 65535u ? 65535u : n;
            uint32_t b;
            if (k < 5u) {
                const uint32_t hd[5] = {n > 65535u || !last ? 0u : 1u, first & 255u, first >> 8, ~first & 255u, (~first >> 8) & 255u};
                b = hd[k];
            } else if (k < 5u + first) {
                b = (T[(h + k - 5u) >> 2] >> (8u * ((h + k - 5u) & 3u))) & 255u;
            } else if (k < 10u + first) {        // (only with n = 65536: the second block holds one byte)
                const uint32_t hd[5] = {last ? 1u : 0u, 1u, 0u, 0xFEu, 0xFFu};
                b = hd[k - 5u - first];
            } else {
                b = (T[(h + k - 10u) >> 2] >> (8u * ((h + k - 10u) & 3u))) & 255u;
            }
            slot[k] = (uint8_t)b;
        }
        len = stored_bytes;
    }
    if (lane == 0) {
        out_len[blk] = len;
        crc[blk] = tile_crc;
    }
}

size_t lds_bytes(uint32_t tile, int level) {     // (with a history: of tile + hist, the region's most)
    const uint32_t held = (tile + 3u) & ~3u;
    return offsetof(Lds, tile) + held + 16u + (level == 2 ? 2u * (held < kLinks ? held : kLinks) : 0u);
}

// tiles of a launch over groups: whole groups have (group - 1) / tile + 1 each, the last group those of its bytes
uint64_t group_tiles(uint64_t n_bytes, uint32_t group, uint32_t tile) {
    const uint64_t tpg = (group - 1u) / tile + 1u, rest = n_bytes % group;
    return n_bytes / group * tpg + (rest + tile - 1) / tile;
}

template <int kLevel, bool kHist, bool kGroups = false, bool kDeep = false, bool kPriced = false>
int launch(const uint8_t *src, uint64_t n_bytes, uint32_t tile, uint32_t hist, uint8_t *dst, uint32_t stride, uint32_t *out_len,
           uint32_t *crc, void *scratch, void *stream, uint32_t group = 0, uint32_t search = 0) {
    if (!tile || tile > kTileMax) return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch: tile must be 1..65536");
    if (stride < FC2_DEFLATE_TILE_BOUND(tile))
        return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch: stride below FC2_DEFLATE_TILE_BOUND(tile)");
    if (!n_bytes) return FC2_OK;
    if (!src || !dst || !out_len || !crc || !scratch) return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch: null argument");
    if (((uintptr_t)scratch & 3u) != 0) return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch: scratch must be 4-byte aligned");
    const uint64_t tiles = kGroups ? group_tiles(n_bytes, group, tile) : (n_bytes + tile - 1) / tile;
    if (tiles > 0x7FFFFFFFull) return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch: too many tiles for one launch");
    // the kernel's LDS (over the 64 KiB a kernel gets unasked, for the larger tiles): once per device and instantiation
    static std::atomic<uint64_t> reserved{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fc2::fail(FC2_E_HIP, "fc2_deflate_launch: no current device");
    const uint64_t bit = 1ull << (dev & 63);
    if (!(reserved.load() & bit)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(deflate_kernel<kLevel, kHist, kGroups, kDeep, kPriced>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kTileMax, kLevel)) != hipSuccess)
            return fc2::fail(FC2_E_HIP, "fc2_deflate_launch: cannot reserve the kernel's LDS");
        reserved |= bit;
    }
    hipLaunchKernelGGL((deflate_kernel<kLevel, kHist, kGroups, kDeep, kPriced>), dim3((uint32_t)tiles), dim3(64), lds_bytes(tile + hist, kLevel),
                       (hipStream_t)stream, src, n_bytes, tile, dst, stride, out_len, crc, static_cast<uint32_t *>(scratch),
                       hist, group, search);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FC2_OK : fc2::fail(FC2_E_HIP, std::string("fc2_deflate_launch: ") + hipGetErrorString(e));
}

}  // namespace

extern "C" uint64_t fc2_deflate_scratch_bytes(uint64_t n_bytes, uint32_t tile) {
    if (!tile || tile > kTileMax || !n_bytes) return 0;
    const uint64_t tiles = (n_bytes + tile - 1) / tile;
    return tiles * tile * sizeof(uint32_t);    // a token per input byte at most
}

extern "C" int fc2_deflate_launch(const uint8_t *src, uint64_t n_bytes, uint32_t tile, uint8_t *dst, uint32_t stride,
                                  uint32_t *out_len, uint32_t *crc, void *scratch, void *stream) {
    return launch<1, false>(src, n_bytes, tile, 0, dst, stride, out_len, crc, scratch, stream);
}

extern "C" int fc2_deflate_launch_level(const uint8_t *src, uint64_t n_bytes, uint32_t tile, uint8_t *dst, uint32_t stride,
                                        uint32_t *out_len, uint32_t *crc, void *scratch, void *stream, int level) {
    if (level == 1) return launch<1, false>(src, n_bytes, tile, 0, dst, stride, out_len, crc, scratch, stream);
    if (level == 2) return launch<2, false>(src, n_bytes, tile, 0, dst, stride, out_len, crc, scratch, stream);
    return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_level: level is 1 or 2");
}

extern "C" int fc2_deflate_launch_hist(const uint8_t *src, uint64_t n_bytes, uint32_t tile, uint32_t hist, uint8_t *dst,
                                       uint32_t stride, uint32_t *out_len, uint32_t *crc, void *scratch, void *stream,
                                       int level) {
    if (level != 1 && level != 2) return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_hist: level is 1 or 2");
    if (!tile || tile > kTileMax || hist > kMaxDist || tile + hist > kTileMax)
        return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_hist: tile must be 1..65536, hist 0..32768, tile + hist <= 65536");
    if (!hist) return fc2_deflate_launch_level(src, n_bytes, tile, dst, stride, out_len, crc, scratch, stream, level);
    if (level == 1) return launch<1, true>(src, n_bytes, tile, hist, dst, stride, out_len, crc, scratch, stream);
    return launch<2, true>(src, n_bytes, tile, hist, dst, stride, out_len, crc, scratch, stream);
}

extern "C" uint64_t fc2_deflate_group_tiles(uint64_t n_bytes, uint32_t group, uint32_t tile) {
    if (!tile || tile > kTileMax || !group) return 0;
    return group_tiles(n_bytes, group, tile);
}

extern "C" int fc2_deflate_launch_groups(const uint8_t *src, uint64_t n_bytes, uint32_t group, uint32_t tile, uint32_t hist,
                                         uint8_t *dst, uint32_t stride, uint32_t *out_len, uint32_t *crc, void *scratch,
                                         void *stream, int level) {
    if (level != 1 && level != 2) return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_groups: level is 1 or 2");
    if (!group || !tile || tile > kTileMax || hist > kMaxDist || tile + hist > kTileMax)
        return fc2::fail(FC2_E_PARAM,
                         "fc2_deflate_launch_groups: group must be >= 1, tile 1..65536, hist 0..32768, tile + hist <= 65536");
    if (level == 1) return launch<1, true, true>(src, n_bytes, tile, hist, dst, stride, out_len, crc, scratch, stream, group);
    return launch<2, true, true>(src, n_bytes, tile, hist, dst, stride, out_len, crc, scratch, stream, group);
}

extern "C" int fc2_deflate_launch_deep(const uint8_t *src, uint64_t n_bytes, uint32_t group, uint32_t tile, uint32_t hist,
                                       uint8_t *dst, uint32_t stride, uint32_t *out_len, uint32_t *crc, void *scratch,
                                       void *stream, uint32_t depth, uint32_t nice) {
    if (depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX || nice < FC2_DEFLATE_NICE_MIN ||
        nice > FC2_DEFLATE_NICE_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_deep: depth is 1..128, nice 4..258");
    if (!tile || tile > kTileMax || hist > kMaxDist || tile + hist > kTileMax)
        return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_deep: tile must be 1..65536, hist 0..32768, tile + hist <= 65536");
    const uint32_t search = depth | (nice << 16);
    if (group) return launch<2, true, true, true>(src, n_bytes, tile, hist, dst, stride, out_len, crc, scratch, stream, group, search);
    if (hist) return launch<2, true, false, true>(src, n_bytes, tile, hist, dst, stride, out_len, crc, scratch, stream, 0, search);
    return launch<2, false, false, true>(src, n_bytes, tile, 0, dst, stride, out_len, crc, scratch, stream, 0, search);
}

extern "C" int fc2_deflate_launch_priced(const uint8_t *src, uint64_t n_bytes, uint32_t group, uint32_t tile, uint32_t hist,
                                         uint8_t *dst, uint32_t stride, uint32_t *out_len, uint32_t *crc, void *scratch,
                                         void *stream, uint32_t depth, uint32_t nice, uint32_t passes) {
    if (passes < FC2_DEFLATE_PASSES_MIN || passes > FC2_DEFLATE_PASSES_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_priced: passes is 1..3");
    if (depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX || nice < FC2_DEFLATE_NICE_MIN ||
        nice > FC2_DEFLATE_NICE_MAX)
        return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_priced: depth is 1..128, nice 4..258");
    if (!tile || tile > kTileMax || hist > kMaxDist || tile + hist > kTileMax)
        return fc2::fail(FC2_E_PARAM, "fc2_deflate_launch_priced: tile must be 1..65536, hist 0..32768, tile + hist <= 65536");
    if (passes == 1)
        return fc2_deflate_launch_deep(src, n_bytes, group, tile, hist, dst, stride, out_len, crc, scratch, stream, depth, nice);
    const uint32_t search = depth | (nice << 16) | (passes << 28);
    if (group)
        return launch<2, true, true, true, true>(src, n_bytes, tile, hist, dst, stride, out_len, crc, scratch, stream, group, search);
    if (hist) return launch<2, true, false, true, true>(src, n_bytes, tile, hist, dst, stride, out_len, crc, scratch, stream, 0, search);
    return launch<2, false, false, true, true>(src, n_bytes, tile, 0, dst, stride, out_len, crc, scratch, stream, 0, search);
}
