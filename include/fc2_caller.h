/*
 * fc2_caller.h -- native find_circ read loop around the breakpoint search (libfc2.so).
 *
 * The per-fragment logic of find_circ.py 1.99 after the alignments are grouped
 * (include/fc2_ingest.h): anchor-pair formation (JunctionSpan, :821-852,
 * adjacent_segment_pairs :1058-1140, process_mate :1492-1527), the junction logic
 * of record_hits (:1276-1439), junction aggregation and naming (Hit /
 * SpliceSiteStorage, :486-730), MultiEventRecorder (:733-763), write_read
 * (:1442-1447) and the --test validator (:1148-1273), with Python-2 output
 * formatting.  find_circ2_amd/caller.py is the same logic in Python (kept as the
 * reference path: --python-caller); tests/test_native_caller.py checks both write
 * identical files.
 *
 * The breakpoint search stays outside: fc2_caller_next collects the anchor pairs
 * of up to `chunksize` fragments (the spans record_hits would evaluate) in the
 * layout fc2_pack_pairs takes; the caller evaluates them (fc2_bp_scan_launch) and
 * returns the raw per-pair results with fc2_caller_submit, which runs
 * record_hits for those fragments in input order.
 *
 * Errors the reference raises (KeyError at :927 / :193, undefined windows,
 * --stranded AttributeError, TypeError on reads without SEQ, ValueError for
 * unknown reference ids) end the run: the call returns FC2_E_FORMAT / FC2_E_KEY
 * and fc2_last_error() holds "ExceptionType: message".
 */
#ifndef FC2_CALLER_H
#define FC2_CALLER_H
#include <stdint.h>

#include "fc2_bp.h"
#include "fc2_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fc2_caller fc2_caller;

typedef struct fc2_caller_opts {     /* find_circ.py:383-413 */
    const char *name;                /* -n (tissue name) */
    const char *known_circ;          /* --known-circ BED6 path or NULL */
    const char *known_lin;           /* --known-lin BED6 path or NULL */
    int32_t min_uniq_qual, asize, margin, maxdist, short_threshold, huge_threshold;
    uint8_t noncanonical, allhits, stranded, strandpref, halfunique, report_nobridges, test, nolinear;
    uint8_t multi_events, noop, write_reads, write_multi;   /* write_*: that output file exists */
    uint32_t _pad;
    uint64_t chunksize;              /* fragments per evaluation batch */
} fc2_caller_opts;

/* Anchor pairs to evaluate (host memory, valid until the next call). pairs[i].chrom
 * is the genome chromosome index (tid_to_chrom of fc2_caller_open); pairs whose
 * chromosome is missing from the genome carry FC2_PAIR_SKIP and fail when
 * record_hits evaluates them.  Pairs whose read part is longer than FC2_MAX_READ_LEN
 * come in long_pairs instead (their read parts in the same `reads` buffer); their
 * results go back with fc2_caller_submit_long before the chunk's fc2_caller_submit. */
typedef struct fc2_caller_batch {
    uint64_t n;
    const uint8_t *reads;            /* read_part bytes (JunctionSpan.read_part, :844) */
    const uint64_t *read_off;        /* [n]; lengths are pairs[i].read_len */
    const fc2_pair *pairs;           /* [n] */
    uint64_t n_long;
    const fc2_long_pair *long_pairs; /* [n_long] */
} fc2_caller_batch;

/* path / is_bam as fc2_ingest_open.  tid_to_chrom [n_tid]: genome chromosome index
 * of each reference id of the alignment file, -1 if absent; fasta: the genome
 * FASTA (4-mers of --all-hits --non-canonical ties), NULL = dummy genome (all N).
 * *n_known_circ / *n_known_lin (may be NULL): known sites loaded. */
int  fc2_caller_open(const char *path, int is_bam, const fc2_caller_opts *opts, fc2_caller **out);
int  fc2_caller_set_genome(fc2_caller *h, const int32_t *tid_to_chrom, int32_t n_tid, const fc2_fasta *fasta,
                           uint64_t *n_known_circ, uint64_t *n_known_lin);
fc2_ingest *fc2_caller_ingest(fc2_caller *h);    /* reference names, header (NULL after the rows, below) */
/* BGZF blocks the input's GPU inflate took and left to the CPU (fc2_ingest_inflate_counts; kept
 * after the input is released). */
int fc2_caller_inflate_counts(const fc2_caller *h, uint64_t *gpu_blocks, uint64_t *cpu_blocks);
void fc2_caller_close(fc2_caller *h);

/* Read on until `chunksize` fragments carry pairs (or the input ends); *b = the pairs
 * to evaluate (n may be 0), *eof = 1 once the input is exhausted.  fc2_caller_next and
 * fc2_caller_submit may run concurrently on two threads (one caller of each): they share only
 * the chunk queue.  fc2_last_error() is per thread.  The chunk stays queued
 * (and *b valid) until fc2_caller_submit records it, so a caller may read ahead: form
 * chunk k+1 while chunk k is being searched (at most FC2_CALLER_MAX_QUEUED chunks).
 * Reading ahead changes nothing in the outputs, which submit writes in input order;
 * if next fails, the caller submits the chunks it holds first, then raises (the
 * reference reaches those fragments' record_hits before the failing one).  An input or
 * process_mate error met after some fragments of a chunk were formed ends that chunk there:
 * it is handed out as usual and the error is returned by the following call. */
#define FC2_CALLER_MAX_QUEUED 64
int fc2_caller_next(fc2_caller *h, fc2_caller_batch *b, int *eof);
/* Chunks handed out by fc2_caller_next and not yet submitted. */
int fc2_caller_queued(fc2_caller *h);
/* Results of the OLDEST queued batch, in its order: fc2_result [n] and, with --all-hits,
 * the tie mask [tw][stride] (x-major 64-bit words, '+' rows then '-' rows). */
int fc2_caller_submit(fc2_caller *h, const fc2_result *results, const uint64_t *tiemask, uint32_t tw,
                      uint64_t stride);
/* Results of the OLDEST queued batch's long pairs (fc2_bp_scan_long_launch), in their order:
 * results [n_long] and, with --all-hits, the tie words [tie words of fc2_long_geometry] (copied;
 * NULL without --all-hits).  Required before fc2_caller_submit(_compact) of a batch with long pairs. */
int fc2_caller_submit_long(fc2_caller *h, const fc2_long_result *results, uint64_t n_long, const uint64_t *ties,
                           uint64_t n_tie_words);
/* The same with the results in a compact transfer form (include/fc2_bp.h "compact results",
 * canonical mode, width 4 or 2 bytes): words [n_words] and the n_esc escapes (indices into this
 * batch), expanded here.  FC2_E_PARAM unless n_words is the oldest queued batch's pair count. */
int fc2_caller_submit_compact(fc2_caller *h, const void *words, int width, uint64_t n_words,
                              const fc2_result_escape *esc, uint64_t n_esc, const uint64_t *tiemask, uint32_t tw,
                              uint64_t stride);

/* Output text produced since the last call: 0 = spliced_reads.fastq, 1 =
 * multi_events.tsv rows, 2 = test_results.tsv rows. */
int fc2_caller_take(fc2_caller *h, int stream, const char **text, uint64_t *len);
/* Write spliced_reads.fastq.gz here instead (find_circ.py:445): the text of stream 0 is cut into
 * pieces of `piece` bytes (0: 4 MiB), each compressed at `level` as its own gzip member on
 * `threads` worker threads and written in order (one valid gzip stream); stream 0 of
 * fc2_caller_take then stays empty.  Call before the first fc2_caller_submit. */
int fc2_caller_set_reads_gz(fc2_caller *h, const char *path, int level, int threads, uint64_t piece);
/* Compress and write what is left and close the file (also done, errors ignored, by
 * fc2_caller_close); FC2_E_IO if a write failed. */
int fc2_caller_close_reads(fc2_caller *h);
/* spliced_reads.fastq.gz compressed on GPU `device` instead of the worker threads (fc2_deflate.hip): call after
 * fc2_caller_set_reads_gz and before the first fc2_caller_submit.  The level is then ignored; every tile of a
 * piece (32768 bytes; FC2_GPU_GZIP_TILE: 1..65536) is its own gzip member.  If the device fails, the CPU
 * compresses from that piece on.  A device that does not answer within FC2_GPU_GZIP_TIMEOUT_S (60) seconds
 * makes fc2_caller_close_reads fail with FC2_E_IO.  The device mode holds four pieces in flight: 64 MiB of
 * pinned host memory and 192 MiB of device memory at the default piece of 4 MiB. */
int fc2_caller_set_reads_gz_device(fc2_caller *h, int device);
/* This handle's tile (0: 32768) and longest wait for the device in seconds (0: 60), for the device mode
 * set afterwards with fc2_caller_set_reads_gz_device.  The command line passes FC2_GPU_GZIP_TILE and
 * FC2_GPU_GZIP_TIMEOUT_S here; the library itself reads no environment variable for them. */
int fc2_caller_set_reads_gz_device_tuning(fc2_caller *h, uint32_t tile, double timeout_s);
/* This handle's compression level on the device (1, the default, or 2: fc2_deflate_launch_level), for the device
 * mode set afterwards with fc2_caller_set_reads_gz_device; FC2_E_PARAM for another level or a call after it.
 * The command line passes FC2_GPU_GZIP_LEVEL here. */
int fc2_caller_set_reads_gz_device_level(fc2_caller *h, int level);
/* This handle's history on the device (bytes, 0..32768; 0, the default: none), for the device mode set afterwards
 * with fc2_caller_set_reads_gz_device: every tile of a piece but its first has the `hist` bytes before it as its
 * window (fc2_deflate_launch_hist), and a piece is one gzip member instead of one per tile.  FC2_E_PARAM for more
 * than 32768 or a call after fc2_caller_set_reads_gz_device; a tile and history of more than 65536 bytes together
 * are refused by fc2_caller_set_reads_gz_device itself (FC2_E_PARAM), which then leaves the CPU writer in place.
 * The command line passes FC2_GPU_GZIP_HISTORY here. */
int fc2_caller_set_reads_gz_device_history(fc2_caller *h, uint32_t hist);
/* This handle's search effort at level 2 on the device (fc2_deflate_launch_deep's depth 1..128 and nice 4..258; not
 * called: level 2's own 8 and 32), for the device mode set afterwards with fc2_caller_set_reads_gz_device.  Call
 * after fc2_caller_set_reads_gz_device_level(h, 2): FC2_E_PARAM while the level is 1, for a value out of range and
 * for a call after fc2_caller_set_reads_gz_device.  If the level is set back to 1 afterwards,
 * fc2_caller_set_reads_gz_device itself is refused (FC2_E_PARAM).  The command line passes FC2_GPU_GZIP_DEPTH and
 * FC2_GPU_GZIP_NICE here. */
int fc2_caller_set_reads_gz_device_search(fc2_caller *h, uint32_t depth, uint32_t nice);
/* This handle's passes at level 2 on the device (fc2_deflate_launch_priced's 1..3; not called: 1), beside whatever
 * search effort is set, for the device mode set afterwards with fc2_caller_set_reads_gz_device.  Refused exactly as
 * fc2_caller_set_reads_gz_device_search is: FC2_E_PARAM while the level is 1, for a value out of range and for a
 * call after fc2_caller_set_reads_gz_device; and fc2_caller_set_reads_gz_device itself is refused if the level is
 * set back to 1 afterwards.  The command line passes FC2_GPU_GZIP_PASSES here. */
int fc2_caller_set_reads_gz_device_passes(fc2_caller *h, uint32_t passes);
/* pieces the device compressed, and pieces of the device mode the CPU compressed, so far (0, 0 without it) */
int fc2_caller_reads_gz_counts(const fc2_caller *h, uint64_t *gpu_pieces, uint64_t *cpu_pieces);

/* ---- the DEFLATE compressor on the GPU (csrc/fc2_deflate.hip) ---- */
/* the most bytes a tile's stream takes: stored blocks (5 bytes each, two for a tile of 65536) when the
 * Huffman form would not be smaller */
#define FC2_DEFLATE_TILE_BOUND(tile) ((uint32_t)(tile) + 16u)
/* n_bytes of src (device) cut into tiles of `tile` bytes; tile i's raw DEFLATE stream goes to
 * dst + i * stride (stride >= FC2_DEFLATE_TILE_BOUND(tile)), its length to out_len[i], the gzip CRC-32 of
 * its input to crc[i]; scratch: fc2_deflate_scratch_bytes(n_bytes, tile) bytes of device memory.  Nothing
 * outside [dst + i * stride, + out_len[i]) is written.  out_len[i] = 0xFFFFFFFF: the kernel gave the tile up
 * (not expected; the caller compresses it). */
int fc2_deflate_launch(const uint8_t *src, uint64_t n_bytes, uint32_t tile, uint8_t *dst, uint32_t stride,
                       uint32_t *out_len, uint32_t *crc, void *scratch, void *stream);
/* fc2_deflate_launch at `level`: 1 is fc2_deflate_launch itself; 2 searches deeper (chains of up to 8
 * candidates per position and a lazy step, csrc/fc2_deflate.hip) for smaller streams of the same form, with the
 * same arguments, scratch and bound.  Any other level: FC2_E_PARAM, before the device is touched. */
int fc2_deflate_launch_level(const uint8_t *src, uint64_t n_bytes, uint32_t tile, uint8_t *dst, uint32_t stride,
                             uint32_t *out_len, uint32_t *crc, void *scratch, void *stream, int level);
/* fc2_deflate_launch_level with a history: the launch's n_bytes are one raw DEFLATE stream cut into tiles.  Tile i
 * may refer to the min(hist, i * tile) input bytes before it (its window: nothing of another tile's output), and
 * every tile's stream but the last ends on a byte boundary with BFINAL = 0, so the streams back to back, in
 * order, are the stream of src[0, n_bytes); crc[i] stays the CRC-32 of tile i's own bytes.  tile 1..65536, hist
 * 0..32768, tile + hist <= 65536, level 1 or 2: anything else is FC2_E_PARAM before the device is touched.
 * hist = 0 is fc2_deflate_launch_level byte for byte (every tile a stream of its own).  Same scratch and bound. */
int fc2_deflate_launch_hist(const uint8_t *src, uint64_t n_bytes, uint32_t tile, uint32_t hist, uint8_t *dst,
                            uint32_t stride, uint32_t *out_len, uint32_t *crc, void *scratch, void *stream, int level);
uint64_t fc2_deflate_scratch_bytes(uint64_t n_bytes, uint32_t tile);
/* The compressor over groups: src[0, n_bytes) is cut into groups of `group` bytes (the last holds the rest), every
 * group into tiles of `tile` bytes (a group's last tile holds its rest).  Tiles are numbered densely: tile
 * g * tpg + k is the k-th of group g, tpg = ceil(group / tile), and only the last group can have fewer than tpg;
 * fc2_deflate_group_tiles gives their number, the entries of out_len and crc and the slots at dst + i * stride.
 * Tile k of a group may refer to the min(hist, k * tile) input bytes before it, never to a byte before its group's
 * first.  Every group is one raw DEFLATE stream, whatever hist is: its last tile is written with BFINAL = 1, every
 * other tile in fc2_deflate_launch_hist's non-final form, so a group's streams back to back, in order, inflate to
 * the group's bytes.  crc[i] is the CRC-32 of tile i's own bytes; out_len[i] <= FC2_DEFLATE_TILE_BOUND(tile);
 * nothing outside [slot, slot + out_len) is written.  With hist > 0 a group's slots are fc2_deflate_launch_hist's
 * over that group's bytes alone; with one tile a group (tile >= group) the launch is fc2_deflate_launch_level at
 * tile = group byte for byte.  group >= 1, tile 1..65536, hist 0..32768, tile + hist <= 65536, level 1 or 2:
 * anything else is FC2_E_PARAM before the device is touched.  scratch: fc2_deflate_scratch_bytes(n_bytes, tile)
 * bytes of device memory (a tile's tokens lie at its input's offset, so 4 * n_bytes are what is used). */
int fc2_deflate_launch_groups(const uint8_t *src, uint64_t n_bytes, uint32_t group, uint32_t tile, uint32_t hist,
                              uint8_t *dst, uint32_t stride, uint32_t *out_len, uint32_t *crc, void *scratch,
                              void *stream, int level);
/* tiles of fc2_deflate_launch_groups over n_bytes (0 for group 0 or a tile outside 1..65536) */
uint64_t fc2_deflate_group_tiles(uint64_t n_bytes, uint32_t group, uint32_t tile);
/* Level 2 with its search effort as arguments: `depth`, the candidates a position walks at most (level 2 itself: 8),
 * and `nice`, the kept length that ends the walk (level 2 itself: 32).  Everything else of level 2 -- the links, the
 * ends of the walk, the first among equal lengths, the cost rule, the lazy step, the stream -- is unchanged, and at
 * depth 8, nice 32 every byte is the matching existing entry's at level 2.  group = 0: fc2_deflate_launch_hist's
 * shape (hist = 0: independent tiles, fc2_deflate_launch_level's); group >= 1: fc2_deflate_launch_groups' shape.
 * Same slots, scratch and bound.  depth outside 1..128 or nice outside 4..258 is FC2_E_PARAM before the device is
 * touched, as is everything the existing entries refuse.  (FC2_DEFLATE_DEPTH_MIN .. FC2_DEFLATE_NICE_MAX:
 * include/fc2_ingest.h.) */
int fc2_deflate_launch_deep(const uint8_t *src, uint64_t n_bytes, uint32_t group, uint32_t tile, uint32_t hist,
                            uint8_t *dst, uint32_t stride, uint32_t *out_len, uint32_t *crc, void *scratch,
                            void *stream, uint32_t depth, uint32_t nice);
/* the range of fc2_deflate_launch_priced's passes */
#define FC2_DEFLATE_PASSES_MIN 1u
#define FC2_DEFLATE_PASSES_MAX 3u
/* level 2's own search effort: what the passes run with where no other is set */
#define FC2_DEFLATE_LEVEL2_DEPTH 8u
#define FC2_DEFLATE_LEVEL2_NICE 32u
/* fc2_deflate_launch_deep with `passes` parses of every tile.  The first is fc2_deflate_launch_deep's; after a pass
 * that is not the last the literal/length and distance codes are built from its histograms, and the next pass runs
 * the same search from the tile's (or its history's) start with one difference: the walk's kept match is taken only
 * if its bytes, as literals in that code, cost strictly more bits than its length and distance codewords and their
 * extra bits (a symbol without a codeword counts 15).  The last pass's tokens are written; the stored form still
 * bounds a tile.  passes = 1 is fc2_deflate_launch_deep byte for byte.  Same shapes, slots, scratch and bound.
 * passes outside 1..3 is FC2_E_PARAM before the device is touched, as is everything fc2_deflate_launch_deep
 * refuses.  tests/deflate_model_priced.py is the rule in Python. */
int fc2_deflate_launch_priced(const uint8_t *src, uint64_t n_bytes, uint32_t group, uint32_t tile, uint32_t hist,
                              uint8_t *dst, uint32_t stride, uint32_t *out_len, uint32_t *crc, void *scratch,
                              void *stream, uint32_t depth, uint32_t nice, uint32_t passes);
/* one buffer through the host path of spliced_reads.fastq.gz's device mode, for tests and other hosts: gzip
 * members (one per tile) of in[0, n) into out (cap bytes); FC2_E_RANGE if they do not fit. */
int fc2_gpu_gzip(int device, const void *in, uint64_t n, uint32_t tile, void *out, uint64_t cap, uint64_t *out_n);
/* fc2_gpu_gzip with the tiles compressed at `level` (1 or 2, fc2_deflate_launch_level; else FC2_E_PARAM) */
int fc2_gpu_gzip_level(int device, const void *in, uint64_t n, uint32_t tile, int level, void *out, uint64_t cap,
                       uint64_t *out_n);
/* fc2_gpu_gzip_level with a history of `hist` bytes (fc2_deflate_launch_hist's rules): every piece of 4 MiB is one
 * gzip member, its tiles' streams back to back (csrc/fc2_gzmember_impl.h).  hist = 0: fc2_gpu_gzip_level's bytes. */
int fc2_gpu_gzip_hist(int device, const void *in, uint64_t n, uint32_t tile, uint32_t hist, int level, void *out,
                      uint64_t cap, uint64_t *out_n);
/* fc2_gpu_gzip_hist at level 2 with fc2_deflate_launch_deep's search effort (depth 1..128, nice 4..258, else
 * FC2_E_PARAM before the device is touched); depth 8, nice 32: fc2_gpu_gzip_hist's bytes at level 2.
 * fc2_gpu_gzip_bound holds. */
int fc2_gpu_gzip_deep(int device, const void *in, uint64_t n, uint32_t tile, uint32_t hist, uint32_t depth, uint32_t nice,
                      void *out, uint64_t cap, uint64_t *out_n);
/* fc2_gpu_gzip_deep with fc2_deflate_launch_priced's passes (1..3, else FC2_E_PARAM before the device is touched);
 * passes = 1: fc2_gpu_gzip_deep's bytes.  fc2_gpu_gzip_bound holds. */
int fc2_gpu_gzip_priced(int device, const void *in, uint64_t n, uint32_t tile, uint32_t hist, uint32_t depth, uint32_t nice,
                        uint32_t passes, void *out, uint64_t cap, uint64_t *out_n);
uint64_t fc2_gpu_gzip_bound(uint64_t n, uint32_t tile);

/* ---- BGZF output on the GPU (csrc/fc2_bgzf_out.hip; the rule: csrc/fc2_bgzf_frame_impl.h) ---- */
/* The slots fc2_deflate_launch filled (n_tiles tiles of `tile` input bytes, 1..0xff00, the last one holding the
 * rest of n_bytes; slots and stride multiples of 16) packed into BGZF blocks on `stream`: block i -- the 18
 * header bytes with BSIZE - 1, tile i's out_len[i] stream bytes, crc[i], ISIZE -- at out + off[i], off[i] =
 * the sum over j < i of 26 + out_len[j]; off[n_tiles] = *total.  out holds n_tiles * (26 +
 * FC2_DEFLATE_TILE_BOUND(tile)) bytes; nothing outside [out, out + *total) is written.  A tile whose out_len is
 * 0xFFFFFFFF, 0 or above the bound makes the piece unwritten: *total = 0, every offset 0.  FC2_E_PARAM (nothing
 * launched) for a tile outside 1..0xff00, more than 65535 tiles, or n_bytes that does not end in the last tile.
 * All pointers are device memory. */
int fc2_bgzf_frame_launch(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                          uint32_t n_tiles, uint64_t n_bytes, uint32_t tile, uint8_t *out, uint32_t *off,
                          uint32_t *total, void *stream);
/* the same rule on host memory (slots at any alignment); *total = 0 also when the arguments are refused */
int fc2_bgzf_frame_host(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                        uint32_t n_tiles, uint64_t n_bytes, uint32_t tile, uint8_t *out, uint32_t *off,
                        uint32_t *total);
/* one buffer through the device writer of spliced_alignments.bam (csrc/fc2_bgzf_gpu.h), for tests and other
 * hosts: in[0, n) as BGZF blocks of `block` (1..0xff00) input bytes, in pieces of piece_blocks (0: 64; at most
 * 1024) blocks, four in flight, into out (cap bytes); no EOF block, and nothing for n = 0.  FC2_E_RANGE if the
 * blocks do not fit, FC2_E_PARAM for a block outside 1..0xff00. */
int fc2_gpu_bgzf(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, void *out,
                 uint64_t cap, uint64_t *out_n);
/* fc2_gpu_bgzf with the blocks compressed at `level` (1 or 2, fc2_deflate_launch_level; else FC2_E_PARAM) */
int fc2_gpu_bgzf_level(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, int level,
                       void *out, uint64_t cap, uint64_t *out_n);
/* fc2_gpu_bgzf_level with every block cut into tiles of `tile` bytes that have up to `hist` bytes of their block
 * before them as history (fc2_deflate_launch_groups, fc2_bgzf_frame_groups_launch): at most 16 tiles a block, hist
 * 0..32768, tile + hist <= 65536, else FC2_E_PARAM.  tile = 0 or tile >= block: fc2_gpu_bgzf_level's bytes. */
int fc2_gpu_bgzf_tiles(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, uint32_t tile,
                       uint32_t hist, int level, void *out, uint64_t cap, uint64_t *out_n);
/* fc2_gpu_bgzf_tiles at level 2 with fc2_deflate_launch_deep's search effort (depth 1..128, nice 4..258, else
 * FC2_E_PARAM before the device is touched); depth 8, nice 32: fc2_gpu_bgzf_tiles' bytes at level 2.  The ISIZE
 * values do not depend on the search; fc2_gpu_bgzf_tiles_bound holds. */
int fc2_gpu_bgzf_deep(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, uint32_t tile,
                      uint32_t hist, uint32_t depth, uint32_t nice, void *out, uint64_t cap, uint64_t *out_n);
/* fc2_gpu_bgzf_deep with fc2_deflate_launch_priced's passes (1..3, else FC2_E_PARAM before the device is touched);
 * passes = 1: fc2_gpu_bgzf_deep's bytes.  The ISIZE values do not depend on it; fc2_gpu_bgzf_tiles_bound holds. */
int fc2_gpu_bgzf_priced(int device, const void *in, uint64_t n, uint32_t block, uint32_t piece_blocks, uint32_t tile,
                        uint32_t hist, uint32_t depth, uint32_t nice, uint32_t passes, void *out, uint64_t cap,
                        uint64_t *out_n);
/* the bytes fc2_gpu_bgzf_tiles needs at most: fc2_gpu_bgzf_bound's with every tile's stream at its worst */
uint64_t fc2_gpu_bgzf_tiles_bound(uint64_t n, uint32_t block, uint32_t tile);
uint64_t fc2_gpu_bgzf_bound(uint64_t n, uint32_t block);
/* fc2_bgzf_frame_launch for blocks of several tiles, the slots fc2_deflate_launch_groups filled (n_tiles =
 * fc2_deflate_group_tiles(n_bytes, group, tile)): block g -- the 18 header bytes, the streams of group g's tiles
 * back to back in order, the group's CRC-32 combined from the tiles' CRCs and lengths (the input is not read),
 * ISIZE = the group's input bytes -- at out + off[g]; off has one entry per group and the end, *total =
 * off[n_groups].  out holds min(65536, 26 + tpg * FC2_DEFLATE_TILE_BOUND(tile)) bytes a group.  A tile whose
 * out_len is 0xFFFFFFFF, 0 or above the bound, or a block of more than 65536 bytes, makes the piece unwritten:
 * *total = 0, every offset 0, no byte of out touched.  FC2_E_PARAM (nothing launched) unless group is 1..0xff00,
 * tile 1..65536 with at most 16 tiles a group, there are at most 65535 groups and n_tiles is their tiles' number.
 * One tile a group: fc2_bgzf_frame_launch's bytes.  All pointers are device memory; two kernels on `stream`. */
int fc2_bgzf_frame_groups_launch(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                                 uint32_t n_tiles, uint64_t n_bytes, uint32_t group, uint32_t tile, uint8_t *out,
                                 uint32_t *off, uint32_t *total, void *stream);
/* the same rule on host memory (slots at any alignment); *total = 0 also when the arguments are refused */
int fc2_bgzf_frame_groups_host(const uint8_t *slots, uint32_t stride, const uint32_t *out_len, const uint32_t *crc,
                               uint32_t n_tiles, uint64_t n_bytes, uint32_t group, uint32_t tile, uint8_t *out,
                               uint32_t *off, uint32_t *total);

/* The BED rows (no header) of 0 = circ_splice_sites.bed, 1 = lin_splice_sites.bed
 * (call once, at the end).  Once the input was read to its end and every chunk submitted, the first
 * call releases the read side -- the input (so finish -B output with fc2_ingest_close_bam_out
 * before), its parse blocks, the chunk buffers -- on a thread of its own: fc2_caller_ingest returns
 * NULL from then on, fc2_caller_next reports the end, the counters keep their final values. */
int fc2_caller_rows(fc2_caller *h, int kind, const char **text, uint64_t *len);
/* The same rows written to the file descriptor fd at its current offset (the CLI's BED files; the
 * ranges are formatted on the workers and written in order as each is done, never joined in memory);
 * *len (may be NULL) = bytes written.  FC2_E_IO if a write failed.  Call once per kind, instead of
 * fc2_caller_rows. */
int fc2_caller_write_rows(fc2_caller *h, int kind, int fd, uint64_t *len);
/* The reference's N[...] counters in sorted key order: i-th name and value;
 * FC2_E_RANGE past the end. */
int fc2_caller_counter(fc2_caller *h, int i, const char **name, double *value);
/* fragments read (n_reads) and anchor pairs evaluated so far, as of the last fc2_caller_next to
 * return (safe to call from a thread other than the one calling fc2_caller_next). */
int fc2_caller_stats(fc2_caller *h, uint64_t *n_reads, uint64_t *n_pairs);

#ifdef __cplusplus
}
#endif
#endif /* FC2_CALLER_H */
