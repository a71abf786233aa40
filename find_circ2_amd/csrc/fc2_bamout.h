// BAM writer for -B/--bam (spliced_alignments.bam, find_circ.py:479-483, 1134-1140):
// BGZF blocks (SAM/BAM spec 4.1) of up to 0xff00 input bytes, raw-deflated with zlib, the
// empty EOF block at close.  Records come either as BAM bytes copied from a BAM input or
// as SAM text lines encoded the way htslib's sam_parse1 does (what pysam writes for a
// record read from SAM).
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

namespace fc2 {
namespace bam {

struct Writer;

// header: the input's header text and its reference names / lengths (pysam template=); level: zlib
// level of the BGZF blocks (htslib's default is 6)
Writer *open_writer(const std::string &path, const std::string &text, const std::vector<std::string> &names,
                    const std::vector<int64_t> &lens, std::string &err, int level = 6);
// one BAM record: block_size (4 B) + body, as found in a BAM stream
bool write_raw(Writer *w, const uint8_t *rec, size_t n);
// one SAM text line (no newline); tid_of maps RNAME/RNEXT to reference ids
bool write_sam(Writer *w, const char *line, const char *end, const std::unordered_map<std::string, int> &tid_of,
               std::string &err);
// one SAM text line encoded as write_sam does, appended to rec (block_size + body)
bool encode_sam(const char *line, const char *end, const std::unordered_map<std::string, int> &tid_of,
                std::string &rec, std::string &err);
// record bytes in bulk (BAM records, back to back): the full blocks they complete are deflated on
// `threads` threads and written in order; the blocks are cut where the record-by-record calls would
// cut them, so the file is byte for byte what those calls write
bool write_bulk(Writer *w, const char *p, size_t n, int threads);
// The device mode (fc2_ingest_set_bam_out_device): call after open_writer and before the first record.  The
// record bytes are cut every `block` (1..0xff00) bytes, as the calls above cut them at 0xff00, but go out in
// pieces of piece_blocks (1..1024) blocks: mode 1 compresses and frames a piece on GPU `device`
// (fc2_bgzf_gpu.h), mode 2 on the host with zlib level 1 and fc2_bgzf_frame_host, through the same code
// otherwise (a test setting); mode 0 leaves the writer as it is.  Piece p uses slot p % 4, and a slot's piece
// is waited for and written before the slot is reused: the pieces reach the file in order, from the calling
// thread.  A piece the device fails on or hands back, and every later one, is compressed by zlib as above.  A
// device that does not answer within timeout_s seconds fails the call that waited and close_writer.
// tile (0 or >= block: none) cuts every block into tiles of that many bytes, each with up to `hist` bytes of its
// block before it as history (fc2_deflate_launch_groups, fc2_bgzf_frame_groups_launch; mode 2: zlib flushed
// at the tiles' ends and fc2_bgzf_frame_groups_host); more than 16 tiles a block, hist over 32768 or tile + hist
// over 65536 are refused.  depth, nice (0, 0: the level's own): level 2's search effort on the device
// (bgz::gpu_open); passes (0: one): level 2's passes on the device, 1..3; mode 2 ignores them as it ignores the level.
bool set_device(Writer *w, int mode, int device, uint32_t block, uint32_t piece_blocks, double timeout_s, int level,
                uint32_t tile, uint32_t hist, std::string &err, uint32_t depth = 0, uint32_t nice = 0, uint32_t passes = 0);
bool device_set(const Writer *w);              // set_device has put the writer into mode 1 or 2
// pieces written from the device (or the host model), and pieces of the device mode zlib compressed, so far
void device_counts(const Writer *w, uint64_t &gpu_pieces, uint64_t &cpu_pieces);
// The encode stage (fc2_ingest_set_bam_out_encode; fc2_bamout_sam.cpp makes one and attaches it): with a stage
// attached write_sam hands every line to it (Writer::add_sam) instead of encoding it in place, and the stage
// gives the records back through write_raw, in the lines' order, whenever it has a batch of them.  The writer
// owns the stage: close_writer finishes it (the rest of the lines, every batch in flight) before its own flush
// and deletes it.  An interface, so that this file links against nothing of the stage's.
struct SamStage {
    virtual ~SamStage() {}
    // one line; false and err: a line encode_sam fails on (its message), the device timed out, or an I/O error
    // (err left empty) -- now or for a line taken earlier
    virtual bool add(const char *line, const char *end, std::string &err) = 0;
    virtual bool finish(std::string &err) = 0;
    // batches written as the device (or its stand-in) returned them, and batches encoded line by line
    virtual void counts(uint64_t &gpu_batches, uint64_t &host_batches) const = 0;
};
void attach_sam_stage(Writer *w, SamStage *stage);
bool sam_stage_set(const Writer *w);
void sam_stage_counts(const Writer *w, uint64_t &gpu_batches, uint64_t &host_batches);
// mode 1: the lines encoded on GPU `device` (fc2_sam_enc_gpu.h); 2: by fc2_sam_encode_host in its place; batches
// of max_lines lines and max_text bytes (0: 16384, 4 MiB), a wait for the device at most timeout_s seconds (0:
// 60).  names: the header's reference names in order; tid_of: the map encode_sam is given, which must outlive
// the writer.  Call after open_writer (and set_device, if that is called) and before the first record
bool set_encode(Writer *w, int mode, int device, const std::vector<std::string> &names,
                const std::unordered_map<std::string, int> *tid_of, uint32_t max_lines, uint32_t max_text, double timeout_s,
                std::string &err);
// flush (the encode stage finished first; the device mode: the rest as a last piece, then every piece in flight,
// in order), EOF block, close; false on an I/O error, a device that timed out or a line the stage still had that
// encode_sam fails on (err: its message); gpu_pieces, cpu_pieces (may be null): device_counts at the end;
// enc_gpu, enc_host (may be null): sam_stage_counts at the end
bool close_writer(Writer *w, std::string &err, uint64_t *gpu_pieces = nullptr, uint64_t *cpu_pieces = nullptr,
                  uint64_t *enc_gpu = nullptr, uint64_t *enc_host = nullptr);

}  // namespace bam
}  // namespace fc2
