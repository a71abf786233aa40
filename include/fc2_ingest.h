/*
 * fc2_ingest.h -- native SAM/BAM ingest for the find_circ2 caller (libfc2.so).
 *
 * Replaces the per-record Python work of find_circ.py's read loop
 * (pysam iteration find_circ.py:461-469, collected_bwa_mem_segments
 * :1450-1486, MateSegments :976-1140, process_mate :1492-1527) for the records
 * that never reach the breakpoint search: every record is parsed and grouped
 * into fragments (mate pairs / single reads) here, adjacent segment pairs are
 * formed with the reference's rules, and only fragments that carry at least
 * one anchor pair are handed back (as SAM text) for the per-fragment logic.
 * Counters the reference keeps for the others are accumulated here.
 *
 * Reads a path or "-" (stdin).  The format is detected from the bytes, never
 * from the file name, as htslib's hts_open does for the reference's
 * pysam.Samfile(path | '-', 'r' | 'rb') (find_circ.py:461-469): the byte source
 * is plain, BGZF (parallel block inflate) or any other gzip stream, and what it
 * holds is BAM ("BAM\1") or SAM text.  CRAM is rejected (FC2_E_FORMAT).
 */
#ifndef FC2_INGEST_H
#define FC2_INGEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fc2_ingest fc2_ingest;

typedef struct fc2_ingest_params {
    int32_t asize;      /* -a: minimal segment length of an anchor (find_circ.py:1125) */
    uint8_t nolinear;   /* --no-linear: fragments without backsplice spans are skipped (:1568-1569) */
    uint8_t noop;       /* --noop: count reads only (:1554-1558) */
    uint8_t _pad[2];
} fc2_ingest_params;

typedef struct fc2_ingest_counts {  /* cumulative since open (the reference's N[...] keys) */
    uint64_t n_reads;               /* fragments yielded (n_reads, :1536) */
    uint64_t total_mates;           /* N['total_mates'] (:978) */
    uint64_t unmapped_reads;        /* N['unmapped_reads'] (:1467) */
    uint64_t unspliced_mates;       /* N['unspliced_mates'] of skipped fragments (:1494) */
    uint64_t seg_too_short_skip;    /* N['seg_too_short_skip'] of skipped fragments (:1127) */
    uint64_t records;               /* alignment records read */
    uint64_t handed_back;           /* fragments returned to the caller */
} fc2_ingest_counts;

/* path "-" reads stdin.  is_bam is the reference's mode hint ('rb' unless the name ends in
 * "sam", find_circ.py:463-466) and, as in htslib, does not decide anything: a BAM named x.sam,
 * SAM named x.bam, bgzip'ed or gzip'ed SAM and BAM on stdin are all read by what they are. */
int  fc2_ingest_open(const char *path, int is_bam, fc2_ingest **out);

/* What fc2_ingest_open found: FC2_INGEST_SAM or FC2_INGEST_BAM (-1 for a null handle);
 * *compression (optional) = FC2_INGEST_PLAIN / _BGZF / _GZIP. */
enum { FC2_INGEST_SAM = 0, FC2_INGEST_BAM = 1 };
enum { FC2_INGEST_PLAIN = 0, FC2_INGEST_BGZF = 1, FC2_INGEST_GZIP = 2 };
int  fc2_ingest_format(const fc2_ingest *h, int *compression);
void fc2_ingest_close(fc2_ingest *h);
int  fc2_ingest_n_refs(const fc2_ingest *h);
const char *fc2_ingest_ref_name(const fc2_ingest *h, int tid);
/* SAM header text (one line per @ record). */
const char *fc2_ingest_header(const fc2_ingest *h);

/* Process up to max_frags fragments.  *text / *text_len: SAM lines of the
 * returned fragments, each fragment's records consecutive and followed by an
 * empty line; valid until the next call.  *n_handed: fragments in *text.
 * *eof = 1 when the input is exhausted.  Returns FC2_OK or a negative status
 * (FC2_E_FORMAT for malformed input; the reference's UnboundLocalError on
 * single-record input is FC2_E_FORMAT with that message).  An error met after some fragments
 * of the call were formed is returned by the following call, after those fragments. */
int fc2_ingest_next(fc2_ingest *h, const fc2_ingest_params *p, uint64_t max_frags, fc2_ingest_counts *counts,
                    const char **text, uint64_t *text_len, uint64_t *n_handed, int *eof);

/* Counters so far (also returned by fc2_ingest_next). */
int fc2_ingest_counts_get(const fc2_ingest *h, fc2_ingest_counts *counts);

/* -B/--bam (replaces pysam.Samfile(spliced_alignments.bam, 'wb', template=sam_input) and
 * bam_out.write(seg) in adjacent_segment_pairs, find_circ.py:479-483, 1134-1140): every
 * processed mate's anchor alignments go to a BGZF BAM with the input's header, in the
 * reference's order.  BAM input records are copied byte for byte; SAM lines are encoded as
 * htslib's sam_parse1 does.  Call once, before the first fc2_ingest_next; the file is
 * finished (EOF block) by fc2_ingest_close_bam_out or fc2_ingest_close. */
int fc2_ingest_set_bam_out(fc2_ingest *h, const char *path);
int fc2_ingest_close_bam_out(fc2_ingest *h);
/* The records of spliced_alignments.bam compressed on a GPU instead of by zlib on the calling thread: call
 * after fc2_ingest_set_bam_out and before the first fc2_ingest_next.  mode 0: off (the default); 1: GPU
 * `device` (fc2_deflate_launch at tile = block, then fc2_bgzf_frame_launch, include/fc2_caller.h); 2: the
 * host model of the device -- every tile raw-deflated by zlib level 1 and framed by fc2_bgzf_frame_host,
 * through the same writer code otherwise (a test setting).  The header block(s) stay zlib's.  The record bytes
 * are cut every `block` bytes (0: 0xff00, where the zlib writer cuts them; at most 0xff00), so the file's
 * ISIZE values are those of mode 0 and only the compressed payloads differ.  piece_blocks (0: 64; at most
 * 1024) blocks make a piece; piece p uses slot p % 4, and a slot's piece is waited for and written before the
 * slot is reused: pieces are written in order, by the calling thread.  fc2_ingest_close_bam_out sends the rest
 * as a last piece, writes every piece in flight and the EOF block.  If the device fails or hands a piece back,
 * zlib compresses that piece and every later one.  A device that does not answer within timeout_s (0: 60)
 * seconds fails the call that waited, and fc2_ingest_close_bam_out, with FC2_E_IO; it is not touched again.
 * At the defaults the four slots hold 31.9 MiB of pinned host and 111.6 MiB of device memory. */
int fc2_ingest_set_bam_out_device(fc2_ingest *h, int mode, int device, uint32_t block, uint32_t piece_blocks,
                                  double timeout_s);
/* The level mode 1 compresses at (1, the default, or 2: fc2_deflate_launch_level, include/fc2_caller.h), for the
 * device mode set afterwards with fc2_ingest_set_bam_out_device; mode 2 ignores it.  FC2_E_PARAM for another
 * level or a call after reading has begun.  The command line passes FC2_GPU_BAM_LEVEL here. */
int fc2_ingest_set_bam_out_device_level(fc2_ingest *h, int level);
/* the ranges of level 2's search effort on the device (fc2_deflate_launch_deep, include/fc2_caller.h): the candidates
 * a position walks at most, and the kept match length that ends the walk */
#define FC2_DEFLATE_DEPTH_MIN 1u
#define FC2_DEFLATE_DEPTH_MAX 128u
#define FC2_DEFLATE_NICE_MIN 4u
#define FC2_DEFLATE_NICE_MAX 258u
/* The search effort mode 1 compresses with at level 2 (not called: level 2's own depth 8 and nice 32), for the device
 * mode set afterwards with fc2_ingest_set_bam_out_device; mode 2 ignores it as it ignores the level.  Call where
 * fc2_ingest_set_bam_out_device_level is called, after it has set level 2: FC2_E_PARAM while the level is 1, for a
 * value out of range, and for a call before fc2_ingest_set_bam_out, after fc2_ingest_set_bam_out_device or after
 * reading has begun.  If the level is set back to 1 afterwards, fc2_ingest_set_bam_out_device itself is refused
 * (FC2_E_PARAM).  The command line passes FC2_GPU_BAM_DEPTH and FC2_GPU_BAM_NICE here. */
int fc2_ingest_set_bam_out_device_search(fc2_ingest *h, uint32_t depth, uint32_t nice);
/* The passes mode 1 compresses with at level 2 (fc2_deflate_launch_priced, include/fc2_caller.h: 1..3,
 * FC2_DEFLATE_PASSES_MIN .. _MAX there; not called: 1), beside whatever search effort is set; mode 2 ignores it.
 * Called and refused exactly as fc2_ingest_set_bam_out_device_search is.  The command line passes
 * FC2_GPU_BAM_PASSES here. */
int fc2_ingest_set_bam_out_device_passes(fc2_ingest *h, uint32_t passes);
/* Tiles inside a block, for the device mode set afterwards with fc2_ingest_set_bam_out_device: every block of the
 * record bytes is cut into tiles of `tile` bytes, each compressed by a wavefront of its own with the min(hist,
 * its offset in the block) bytes of its block before it as history, and the block's streams, combined CRC-32 and
 * ISIZE are put together on the device (fc2_deflate_launch_groups, fc2_bgzf_frame_groups_launch,
 * include/fc2_caller.h).  tile = 0 (the default) or tile >= block: a block is one tile, and hist is not used.
 * Mode 2 flushes zlib at the tiles' ends and frames with fc2_bgzf_frame_groups_host.  FC2_E_PARAM for hist over
 * 32768 and for a call after fc2_ingest_set_bam_out_device or after reading has begun; more than 16 tiles a block
 * and tile + hist over 65536 are refused by fc2_ingest_set_bam_out_device itself (FC2_E_PARAM), which then leaves
 * the CPU writer in place.  The command line passes FC2_GPU_BAM_TILE and FC2_GPU_BAM_HISTORY here. */
int fc2_ingest_set_bam_out_device_tiles(fc2_ingest *h, uint32_t tile, uint32_t hist);
/* pieces the device (mode 2: its host model) compressed, and pieces of the device mode zlib compressed, so
 * far; final after fc2_ingest_close_bam_out (0, 0 without the device mode) */
int fc2_ingest_bam_out_counts(const fc2_ingest *h, uint64_t *gpu_pieces, uint64_t *cpu_pieces);

/* ``samtools view -b`` for SAM text (any compression): every record encoded as htslib's
 * sam_parse1 does (the -B encoder above), BGZF blocks (zlib level 1, as samtools view -1) + EOF block.  Used to make BAM inputs for
 * tests and the bench's stdin-BAM CLI run. */
int fc2_sam_to_bam(const char *sam_path, const char *bam_path);
/* The BAM input's BGZF blocks inflated on GPU `device` (fc2_inflate.hip) instead of the CPU from the
 * next batch on; call before reading (FC2_GPU_INFLATE=1 or 2 makes the CLI's read loop call this, on
 * its first device; by default it calls fc2_ingest_set_gpu_inflate_from below).  The device's
 * buffers are made now (wait != 0) or meanwhile, the batches inflated on the CPU until they are ready.
 * Batches grow to 1024 blocks (FC2_BGZF_BATCH still sets them); every block's CRC-32 and ISIZE are
 * checked (on the device), and the CPU inflates any block the GPU refused, and every block from then
 * on if the device fails.  device < 0, a non-BGZF input or FC2_GPU_INFLATE=0: the CPU inflates. */
int fc2_ingest_set_gpu_inflate(fc2_ingest *h, int device, int wait);
/* The same, with nothing made on the device until after_bytes of the input were read (0: as
 * fc2_ingest_set_gpu_inflate(h, device, 0)): smaller inputs never touch the device, and their batches
 * keep the ingest's size.  The CLI's default, with 256 MiB (DESIGN.md §5 "The BAM input inflated on the
 * GPU").  FC2_GPU_INFLATE=0 turns it off, 1 or 2 start it at once. */
int fc2_ingest_set_gpu_inflate_from(fc2_ingest *h, int device, uint64_t after_bytes);
/* Blocks of the batches the GPU inflated: those it took, and those it left to the CPU. */
int fc2_ingest_inflate_counts(const fc2_ingest *h, uint64_t *gpu_blocks, uint64_t *cpu_blocks);
/* BGZF blocks inflated on the GPU (fc2_inflate.hip; the BAM input's inflate, which pysam/htslib does for
 * the reference, find_circ.py:461-469): n blocks, block i = len[i] bytes of raw DEFLATE at src + off[i]
 * (device memory, readable 8 bytes past every payload: a BGZF block's trailer) holding isize[i] <= 65536
 * bytes, inflated into dst + i * 65536 and, when crc is not NULL, checked against crc[i] (the gzip
 * CRC-32); status[i] = 0, or why the block was refused (the host then inflates it on the CPU). */
int fc2_bgzf_inflate_launch(const uint8_t *src, const uint32_t *off, const uint32_t *len, const uint32_t *isize,
                            const uint32_t *crc, uint8_t *dst, uint32_t *status, uint32_t n, void *stream);

/* The BAM record starts of inflated BGZF blocks, listed on the GPU (fc2_inflate.hip bam_walk_kernel) for the
 * ingest's splitter: per block, the record starts a walk visits when it begins at the block's first
 * plausible record -- one followed by another plausible record or by the block's end -- and goes from
 * block_size to block_size, and where that walk leaves the block.  A row of `starts` holds
 * FC2_BAM_WALK_CAP entries: a step advances at least 4 + 32 bytes and the last start is at most
 * 65536 - 4, so a block has at most (65536 - 4) / 36 + 1 = 1821 of them (1824: rows of whole 16 bytes). */
#define FC2_BAM_WALK_CAP 1824
#define FC2_BAM_WALK_NO_EXIT 0xFFFFFFFFu
/* n_blocks blocks, block i = isize[i] <= 65536 bytes at slots + i * 65536 (device memory, 4-byte aligned:
 * the slots fc2_bgzf_inflate_launch fills), on `stream`.  count[i] = its record starts, starts[i *
 * FC2_BAM_WALK_CAP + k] = the k-th one (ascending offsets into the block), exit[i] = the offset the walk
 * leaves the block at (it may lie far past the block's end), FC2_BAM_WALK_NO_EXIT if it met a block_size
 * below 32 or found no start.  A block whose status[i] != 0 is not read: count 0, no exit (status NULL:
 * every block is read). */
int fc2_bam_walk_launch(const uint8_t *slots, const uint32_t *isize, const uint32_t *status, uint16_t *starts,
                        uint32_t *count, uint32_t *exit, uint32_t n_blocks, void *stream);
/* The same for one block of n <= 65536 bytes in host memory, on the CPU: the ingest's own walk (what it
 * runs for the blocks the CPU inflates), in the kernel's output form; starts holds FC2_BAM_WALK_CAP entries. */
int fc2_bam_walk_host(const uint8_t *block, uint32_t n, uint16_t *starts, uint32_t *count, uint32_t *exit);
/* Whether the blocks the GPU inflates take their record lists from the device as well (on != 0, the
 * default) or are walked by host threads (0).  Holds from the next batch on; without a GPU inflate it
 * changes nothing. */
int fc2_ingest_set_gpu_walk(fc2_ingest *h, int on);
/* Blocks of the batches the GPU inflated whose record lists came from the device, and those walked on the
 * host (the blocks the device refused, or every block with the device lists off). */
int fc2_ingest_walk_counts(const fc2_ingest *h, uint64_t *device_blocks, uint64_t *cpu_blocks);

/* The record digest: the fields the ingest's BAM parser derives from a record's CIGAR, aux tags and first
 * QUAL byte, computed on the GPU (fc2_inflate.hip bam_digest_kernel) for the record starts the walk
 * listed, one row per listed start.  The fixed fields (flag, tid, pos, l_read_name, l_seq) are not here:
 * the host reads them from the record's first cache line, which it touches for the query name anyway.
 * A row with state 0 holds block_size (0 if its four bytes are not all in the byte range) and zeros. */
typedef struct fc2_bam_digest {
    uint8_t  state;      /* 1: the fields below are the host parser's; 0: the host parses this record */
    uint8_t  as_type;    /* 0: no AS tag; else its BAM type char (c C s S i I f A Z H B) */
    uint8_t  xs_type;    /* the same for XS */
    uint8_t  has_qual;   /* !(l_seq == 0 || qual[0] == 0xFF) */
    uint32_t block_size; /* the record's own block_size, for the host to match against the bytes it reads */
    int32_t  astart;     /* leading clips up to the first M (aligned_start_from_cigar) */
    int32_t  qlen;       /* len(query) with Python's slice semantics (-1 when l_seq == 0) */
    uint32_t as_bits;    /* the value's bytes, zero- or sign-extended as its type says; 0 for A Z H B */
    uint32_t xs_bits;
    int64_t  aend;       /* -1 if flag & 4 or n_cigar == 0, else pos + ref_span */
} fc2_bam_digest;
/* Blocks of one launch at most (the ingest's largest batch). */
#define FC2_BAM_DIGEST_MAX_BLOCKS 1024
/* n_blocks blocks of one contiguous stream of n_bytes at `bytes` (device memory, any alignment): block i
 * is isize[i] bytes at bytes + ooff[i], ooff ascending; starts / count are fc2_bam_walk_launch's rows
 * (offsets into each block).  first[i] = the sum of min(count[j], FC2_BAM_WALK_CAP) over j < i, first[n_blocks]
 * the number of rows; rows[first[i] + k] digests the record at ooff[i] + starts[i * FC2_BAM_WALK_CAP + k],
 * which may run on into the following blocks.  State 0 (the host parses the record as ever, and raises
 * what it raises): the record's 4 + block_size bytes are not all below n_bytes; it touches a block whose
 * status is not 0 (status NULL: none); block_size < 32 or >= 2^28; its fields exceed the block, its name
 * is empty or not NUL-terminated; its aux data is corrupt or ends inside a tag; AS or XS occurs more than
 * once; a CIGAR sum (reference span, aligned start, leading or trailing soft clips) is 2^31 or more.
 * Nothing outside [bytes, bytes + n_bytes) is read whatever the bytes say, and nothing but first[0 ..
 * n_blocks] and rows[0 .. first[n_blocks]) written.  More than FC2_BAM_DIGEST_MAX_BLOCKS blocks: FC2_E_PARAM. */
int fc2_bam_digest_launch(const uint8_t *bytes, uint32_t n_bytes, const uint32_t *ooff, const uint32_t *isize,
                          const uint32_t *status, const uint16_t *starts, const uint32_t *count,
                          fc2_bam_digest *rows, uint32_t *first, uint32_t n_blocks, void *stream);
/* The same row for the record start at byte `at` of n_bytes bytes in host memory, from the ingest's own
 * parser (the tests' oracle; it knows no block status).  at > n_bytes: FC2_E_RANGE. */
int fc2_bam_digest_host(const uint8_t *bytes, uint32_t n_bytes, uint32_t at, fc2_bam_digest *row);
/* Whether the parse threads take those fields from device rows for the records of the blocks the GPU
 * inflated and listed (on != 0) or parse every record themselves (0, the default).  Needs the device
 * lists (fc2_ingest_set_gpu_walk); holds from the next batch on. */
int fc2_ingest_set_gpu_digest(fc2_ingest *h, int on);
/* Records of the batches the GPU inflated whose fields came from device rows, and those the host parsed. */
int fc2_ingest_digest_counts(const fc2_ingest *h, uint64_t *device_records, uint64_t *host_records);

/* The fragment row: whether the record at a listed start opens a fragment that is never handed to the
 * search whatever the options are -- each mate has fewer than two proper segments, so the fragment changes
 * four counters and nothing else -- and where the next fragment begins, found on the GPU (fc2_inflate.hip
 * bam_frag_kernel) from the bytes the walk and the digest read.  One row per listed start, indexed like
 * the digest rows.  The ingest's parse threads step over such a fragment without building its records. */
typedef struct fc2_bam_frag {
    uint8_t  state;       /* 1: this record opens a fragment the device closed; 0: nothing is claimed */
    uint8_t  n_records;   /* records of the fragment, this one and unmapped ones included */
    uint8_t  n_mates;     /* 1 or 2 */
    uint8_t  n_unmapped;  /* records among them with flag & 4 */
    uint32_t bytes;       /* from this record's offset to the offset of the record that opens the next fragment */
} fc2_bam_frag;
/* Records of a fragment the device closes, at most. */
#define FC2_BAM_FRAG_CAP 16
/* The tables of fc2_bam_digest_launch, the digest rows it made of them (rows, first: device memory, the
 * launch before this one on `stream`), and frag_rows[first[i] + k] for block i's k-th listed start.
 * isize and status are taken to keep that launch's argument list and are not read: a block's status acts
 * here only through the digest rows, where a record that touches a refused block has state 0.
 * A record is *usable* if its digest row has state 1.  A step from a record forward reaches the record at
 * its end (offset + 4 + block_size), which must be a listed start and usable; a step back reaches the
 * listed start before it in the order of the lists, which must be usable and end where this one starts.
 * Two names are equal when l_read_name and the l_read_name - 1 bytes before the NUL are.  Record H gets
 * state 1 only if (otherwise the row is all zeros)
 *   1. H is usable and mapped (flag & 4 == 0);
 *   2. stepping back over at most 4 unmapped records reaches a mapped record, whose name differs from H's;
 *   3. stepping forward reaches a mapped record N whose name differs from H's, after at most
 *      FC2_BAM_FRAG_CAP records (H, and every record before N: the fragment);
 *   4. the fragment's mapped records form one or two mates: H opens mate 1, a record whose flag & 0x40 is
 *      the current mate's first record's is a segment of it, the first one that differs opens mate 2, and
 *      a further change ends the attempt;
 *   5. no segment is proper (the refID and the flag & 0x10 of its mate's first record).
 * Then the fragment is n_reads += 1, records += n_records, total_mates += n_mates, unmapped_reads +=
 * n_unmapped and (unless noop) unspliced_mates += n_mates to the ingest, and nothing else.
 * Nothing outside [bytes, bytes + n_bytes) is read and nothing but frag_rows[0 .. first[n_blocks]) written. */
int fc2_bam_frag_launch(const uint8_t *bytes, uint32_t n_bytes, const uint32_t *ooff, const uint32_t *isize,
                        const uint32_t *status, const uint16_t *starts, const uint32_t *count,
                        const fc2_bam_digest *rows, const uint32_t *first, fc2_bam_frag *frag_rows,
                        uint32_t n_blocks, void *stream);
/* The same rows from the same tables in host memory (the tests' oracle): `usable` is decided by
 * fc2_bam_digest_host and the blocks' status, as fc2_bam_digest_launch decides it.  first: n_blocks + 1
 * entries, written; frag_rows: first[n_blocks] rows (at most the sum of min(count[i], FC2_BAM_WALK_CAP)). */
int fc2_bam_frag_host(const uint8_t *bytes, uint32_t n_bytes, const uint32_t *ooff, const uint32_t *isize,
                      const uint32_t *status, const uint16_t *starts, const uint32_t *count,
                      fc2_bam_frag *frag_rows, uint32_t *first, uint32_t n_blocks);
/* Whether the parse threads step over the fragments the device closed (on = 1; needs the device lists,
 * fc2_ingest_set_gpu_walk) or group every record themselves (0, the default).  Only where fragments are
 * grouped on the parse threads: never with a -B writer or fc2_ingest_next's SAM text.  Holds from the
 * next batch on.  on = 2 is a test setting for machines without a GPU: the rows of the batches the CPU
 * inflates are filled on the host with fc2_bam_frag_host, so the same parse-thread logic runs. */
int fc2_ingest_set_gpu_group(fc2_ingest *h, int on);
/* Fragments the parse threads stepped over on the device's word, and every other fragment.  The pair is
 * meant to be read once the input is exhausted: the first figure is counted by the parse threads, which
 * run ahead of the reader, the second is the reader's n_reads less the first (0 while that is negative),
 * so before the end the two need not add up to the fragments read so far. */
int fc2_ingest_group_counts(const fc2_ingest *h, uint64_t *device_fragments, uint64_t *host_fragments);

/* ---- -B's BAM records from SAM text on the GPU (csrc/fc2_sam_encode_impl.h, fc2_sam_encode.hip) ----
 * A batch of SAM lines (back to back, no newlines; line i is text[off[i] .. off[i + 1])) becomes the BAM
 * record bytes the -B encoder above (fc2::bam::encode_sam) makes of them.  The contract is "never a wrong
 * byte": for every line either status[i] != 0 (one of the reasons below) and size[i] == 0, or the record's
 * bytes, its 4-byte block_size included, are encode_sam's and encode_sam succeeds on the line.  What the rule
 * does not reproduce exactly it refuses; the caller encodes such lines on the host. */
#define FC2_SAM_ENC_OK        0u
#define FC2_SAM_ENC_FIELDS    1u  /* fewer than 11 fields */
#define FC2_SAM_ENC_NUMBER    2u  /* FLAG, POS, MAPQ, PNEXT or TLEN is not -?[0-9]{1,9} */
#define FC2_SAM_ENC_CIGAR     3u  /* not `*` or ([0-9]{1,9}[MIDNSHP=X])+, a count of 2^28 or more, over 65535 ops */
#define FC2_SAM_ENC_QNAME     4u  /* QNAME is empty or longer than 254 bytes */
#define FC2_SAM_ENC_TAG       5u  /* a tag that is not TG:T:VALUE, an `i` value that is not -?[0-9]{1,18} */
#define FC2_SAM_ENC_TAG_TYPE  6u  /* a tag of type f or B (left to the host), or of no known type */
#define FC2_SAM_ENC_OFFSETS   7u  /* off[i] > off[i + 1], or off[i + 1] > text_bytes */
#define FC2_SAM_ENC_LONG      8u  /* fc2_gpu_sam_encode only: a line longer than a batch's text */
/* a batch: at most this many lines and this many bytes of text */
#define FC2_SAM_ENC_MAX_LINES 16384u
#define FC2_SAM_ENC_MAX_TEXT  (4u << 20)
/* Bytes the records of n_lines lines in text_bytes bytes of text take at most: 2 * text_bytes + 40 * n_lines
 * (proved beside fc2::samenc::record_bound in csrc/fc2_sam_encode_impl.h). */
#define FC2_SAM_ENC_BOUND(text_bytes, n_lines) (2ull * (text_bytes) + 40ull * (n_lines))
/* The table RNAME and RNEXT are looked up in, made of the header's reference names in their order: a name's
 * id is its index, and of a name that occurs twice the last index counts (as in the ingest's own map).  lens
 * may be null (the names are C strings).  table null or cap below the need: only *need (bytes, a multiple of
 * 4) is set and FC2_E_RANGE returned if table was given.  The table is position independent: copy it to the
 * device as it is. */
int fc2_sam_names_table(const char *const *names, const uint32_t *lens, uint32_t n_names, uint32_t *table,
                        uint64_t cap, uint64_t *need);
/* One batch on the device (all pointers device memory; n_lines 1..FC2_SAM_ENC_MAX_LINES, text_bytes at most
 * FC2_SAM_ENC_MAX_TEXT, out_cap at least FC2_SAM_ENC_BOUND(text_bytes, n_lines)): a sizing pass (status[i],
 * size[i]), an exclusive scan (out_off[0 .. n_lines], *total = out_off[n_lines]) and a writing pass that puts
 * the accepted records back to back in line order, record i at out + out_off[i].  A wavefront a line.  No
 * byte of out at or past *total is written; nothing outside the line is read. */
int fc2_sam_encode_launch(const uint8_t *text, uint32_t text_bytes, const uint32_t *off, uint32_t n_lines,
                          const uint32_t *names_table, uint32_t table_bytes, uint8_t *out, uint64_t out_cap,
                          uint32_t *out_off, uint32_t *size, uint32_t *status, uint32_t *total, void *stream);
/* The same rule on host memory (the tests' oracle for the kernels, and the writer's stand-in mode). */
int fc2_sam_encode_host(const uint8_t *text, uint32_t text_bytes, const uint32_t *off, uint32_t n_lines,
                        const uint32_t *names_table, uint32_t table_bytes, uint8_t *out, uint64_t out_cap,
                        uint32_t *out_off, uint32_t *size, uint32_t *status, uint32_t *total);
/* Any number of lines through the writer's slot pipeline on GPU `device` (four slots, each with its stream:
 * upload, the three kernels, download of the total, the statuses and exactly the total's bytes), in batches of
 * batch_lines lines (0: FC2_SAM_ENC_MAX_LINES) and at most FC2_SAM_ENC_MAX_TEXT bytes: status[i] for every
 * line, the accepted records back to back in line order in out (cap at least fc2_gpu_sam_encode_bound), their
 * bytes in *out_n.  names: n_names C strings. */
int fc2_gpu_sam_encode(int device, const void *text, const uint32_t *off, uint64_t n_lines, const char *const *names,
                       uint32_t n_names, uint32_t batch_lines, void *out, uint64_t cap, uint64_t *out_n, uint32_t *status);
uint64_t fc2_gpu_sam_encode_bound(uint64_t text_bytes, uint64_t n_lines);
/* The yardstick: one line through the -B encoder itself (fc2::bam::encode_sam, whose body this does not
 * change).  FC2_E_FORMAT and encode_sam's message (fc2_last_error) where it fails; FC2_E_RANGE if cap is
 * below the record's bytes (*out_n is set all the same). */
int fc2_sam_encode_line(const char *line, uint64_t n, const char *const *names, uint32_t n_names, void *out,
                        uint64_t cap, uint64_t *out_n);
/* -B with SAM input: the written records encoded in batches by the rule above instead of line by line on the
 * reading thread.  Call after fc2_ingest_set_bam_out and before reading.  mode 0: off (the default); 1: GPU
 * `device`; 2: fc2_sam_encode_host in the device's place, through the same batching, ordering, refusal and
 * error code (a test setting).  Lines fill a batch; a full batch goes to one of four slots; batches are
 * collected strictly in order.  A batch with no refusal is written as it came back; a batch with one is
 * encoded again on the host, line by line, so the file's bytes and order are those of mode 0 always.  A line
 * the -B encoder fails on ends the run with the code and message of mode 0, at a later fc2_ingest_next or at
 * fc2_ingest_close_bam_out: the records before it are in the file, none after it.  A device that fails moves
 * that batch and every later one to the host; one that does not answer within the timeout ends the run with
 * FC2_E_IO.  BAM input takes the call and does nothing (its records are copied).  Works with either writer
 * (fc2_ingest_set_bam_out_device or zlib). */
int fc2_ingest_set_bam_out_encode(fc2_ingest *h, int mode, int device);
/* A batch's caps (0: FC2_SAM_ENC_MAX_LINES, FC2_SAM_ENC_MAX_TEXT; never more) and the seconds a wait for the
 * device may take (0: 60), for the stage set afterwards with fc2_ingest_set_bam_out_encode.  The command line
 * passes FC2_GPU_BAM_TIMEOUT_S here. */
int fc2_ingest_set_bam_out_encode_caps(fc2_ingest *h, uint32_t max_lines, uint32_t max_text, double timeout_s);
/* batches written as the device (mode 2: the host rule) returned them, and batches encoded line by line on
 * the host; final after fc2_ingest_close_bam_out (0, 0 while the stage is off) */
int fc2_ingest_bam_encode_counts(const fc2_ingest *h, uint64_t *gpu_batches, uint64_t *host_batches);

/* ---- unspliced fragments of SAM text closed on the GPU (csrc/fc2_sam_frag_impl.h, fc2_sam_group.hip) ----
 * A block is n_bytes of text as the ingest's splitter cuts it: whole lines.  A *line* is the bytes from the
 * block's start, or from the byte after a `\n`, up to the next `\n`; a tail with no `\n` is not listed.
 * starts[0 .. n_lines]: line k is text[starts[k] .. starts[k + 1] - 1) (without its `\n`), starts[0] = 0.
 * A line is *usable* (its head row has state 1) only if it does not end in `\r`, has at least 10 tabs, a QNAME
 * of 1..254 bytes, a FLAG that is [0-9]{1,5} and at most 65535, and a CIGAR that is `*` or made only of bytes
 * in [0-9MIDNSHP=X].  A usable line is one the ingest's parse_sam_record accepts, with the flag, the name and
 * the refID the row gives: what strtoll would be asked about (a sign, a blank, 0x) is not usable.  A blank
 * line is not usable.  tid is RNAME through the names' table (fc2_sam_names_table): `*` and unknown names -1. */
typedef struct fc2_sam_head {
    uint32_t flag;        /* FLAG */
    int32_t  tid;         /* RNAME's index in the header, -1 for `*` or a name it does not hold */
    uint32_t l_name;      /* QNAME's bytes: the line's first l_name */
    uint32_t state;       /* 1: usable, the fields above are the host parser's; 0: not, and the row is all zeros */
} fc2_sam_head;
/* The text of one launch at most, the bytes of a listing segment, and the words of scratch a launch needs. */
#define FC2_SAM_GROUP_MAX_TEXT (16u << 20)
#define FC2_SAM_GROUP_SEG      1024u
#define FC2_SAM_GROUP_SCRATCH(n_bytes) (((uint64_t)(n_bytes) + FC2_SAM_GROUP_SEG - 1) / FC2_SAM_GROUP_SEG + 1)
/* One block on the device (all pointers device memory, text of any alignment; n_bytes at most
 * FC2_SAM_GROUP_MAX_TEXT; scratch: FC2_SAM_GROUP_SCRATCH(n_bytes) words), five launches on `stream`: the `\n`
 * of every FC2_SAM_GROUP_SEG-byte segment counted, the counts scanned (*n_lines_out), starts[0 .. n_lines]
 * written, the head rows (a wavefront a line), the fragment rows (a lane a line).  frag_rows[k] is
 * fc2_bam_frag's row for line k under fc2_bam_frag's five conditions, with "record" read as "line", "the record
 * at its end" as line k + 1, "the listed start before" as line k - 1, and name equality as byte equality of the
 * QNAMEs: at most 4 unmapped lines on the way back, at most FC2_BAM_FRAG_CAP lines forward; the block's first
 * head, a fragment whose closer is not a listed line of this block and any unusable line on the way give state
 * 0; bytes = starts[N] - starts[H].  When n_lines > cap only *n_lines_out is written: the block is the host's.
 * Nothing outside [text, text + n_bytes) is read whatever the bytes hold; nothing but *n_lines_out,
 * starts[0 .. min(n_lines, cap)], line_rows and frag_rows[0 .. n_lines) and the scratch is written. */
int fc2_sam_group_launch(const uint8_t *text, uint32_t n_bytes, const uint32_t *names_table, uint32_t table_bytes,
                         uint32_t *starts, fc2_sam_head *line_rows, fc2_bam_frag *frag_rows, uint32_t *n_lines_out,
                         uint32_t cap, uint32_t *scratch, void *stream);
/* The same rows from host memory by the same rule (the tests' oracle, and the ingest's stand-in at setting 2). */
int fc2_sam_group_host(const uint8_t *text, uint32_t n_bytes, const uint32_t *names_table, uint32_t table_bytes,
                       uint32_t *starts, fc2_sam_head *line_rows, fc2_bam_frag *frag_rows, uint32_t *n_lines_out,
                       uint32_t cap);
/* SAM text input: whether the parse threads step over the fragments those rows close (on = 1: the splitter
 * reads every block into a slot's pinned text and queues the upload, the launches and the download of starts
 * and frag_rows on the slot's stream on GPU `device`; the parse thread that takes the block waits for them, at
 * most 60 seconds) or group every line themselves (0, the default).  on = 2 is a
 * test setting for machines without a GPU: fc2_sam_group_host fills the slot's rows, through the same slots and
 * the same parse-thread logic.  Call before reading.  A BAM input refuses it (FC2_E_PARAM).  Only where
 * fragments are grouped on the parse threads: never with a -B writer or fc2_ingest_next's SAM text.  A device
 * failure, no free slot, a block over a slot's text, or more lines than a slot's rows leave that block to the
 * host as ever; a device that does not answer in time ends the run with FC2_E_IO and the block's number. */
int fc2_ingest_set_gpu_sam_group(fc2_ingest *h, int on, int device);
/* As fc2_ingest_group_counts, for the stage above: to be read once the input is exhausted. */
int fc2_ingest_sam_group_counts(const fc2_ingest *h, uint64_t *device_fragments, uint64_t *host_fragments);
#ifdef __cplusplus
}
#endif
#endif /* FC2_INGEST_H */
