// fc2_bamout.cpp -- BGZF/BAM writer for -B/--bam (see fc2_bamout.h).
#include "fc2_bamout.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <thread>

#include "../../include/fc2_caller.h"
#include "fc2_bgzf_gpu.h"

namespace fc2 {
namespace bam {

namespace {
constexpr size_t kBlockIn = 0xff00;        // htslib's BGZF_BLOCK_SIZE: input bytes per block
constexpr size_t kBlockMax = 0x10000;      // a block (header + deflate + trailer) is at most 64 KiB

// SAM spec 5.3 (and htslib hts_reg2bin with min_shift 14, 5 levels)
int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

int nt16(char c) {                         // htslib seq_nt16_table (case-insensitive, else N)
    switch (c) {
        case '=': return 0; case 'A': case 'a': return 1; case 'C': case 'c': return 2;
        case 'M': case 'm': return 3; case 'G': case 'g': return 4; case 'R': case 'r': return 5;
        case 'S': case 's': return 6; case 'V': case 'v': return 7; case 'T': case 't': return 8;
        case 'U': case 'u': return 8; case 'W': case 'w': return 9; case 'Y': case 'y': return 10;
        case 'H': case 'h': return 11; case 'K': case 'k': return 12; case 'D': case 'd': return 13;
        case 'B': case 'b': return 14; default: return 15;
    }
}

int cigar_op(char c) {
    const char *ops = "MIDNSHP=X";
    const char *p = strchr(ops, c);
    return (c && p) ? (int)(p - ops) : -1;
}

template <class T> void put(std::string &s, T v) { s.append((const char *)&v, sizeof v); }
}  // namespace

// one BGZF block of n (<= kBlockIn) input bytes into out (kBlockMax bytes); its size, 0 on failure
size_t deflate_block(z_stream &zs, const char *in, size_t n, uint8_t *out) {
    deflateReset(&zs);
    zs.next_in = (Bytef *)in;
    zs.avail_in = (uInt)n;
    zs.next_out = out + 18;
    zs.avail_out = (uInt)(kBlockMax - 18 - 8);
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) return 0;
    const size_t clen = kBlockMax - 18 - 8 - zs.avail_out;
    const size_t bsize = 18 + clen + 8;
    static const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    memcpy(out, hdr, 16);
    out[16] = (uint8_t)((bsize - 1) & 0xff);
    out[17] = (uint8_t)((bsize - 1) >> 8);
    const uint32_t crc = (uint32_t)crc32(0L, (const Bytef *)in, (uInt)n);
    const uint32_t isize = (uint32_t)n;
    memcpy(out + 18 + clen, &crc, 4);
    memcpy(out + 18 + clen + 4, &isize, 4);
    return bsize;
}

struct Writer {
    FILE *fp = nullptr;
    std::string buf;                       // uncompressed bytes of the current block
    z_stream zs{};
    int level = 6;
    bool ok = true;
    std::vector<uint8_t> out;

    // the device mode (set_device): pieces [head, next) are in flight, piece p in slot p % kSlots
    static constexpr int kSlots = bgz::kSlots;
    static constexpr uint64_t kNever = ~0ull;
    int mode = 0;
    uint32_t block = 0, stride = 0;
    uint32_t tile = 0, hist = 0;           // tile > 0: a block is cut into tiles (set_device), the slots are the tiles'
    size_t piece_bytes = 0;
    bgz::Gpu *gpu = nullptr;
    bool timed_out = false;
    std::string dev_err;
    std::string pend;                      // the bytes of the piece being filled
    std::string in[kSlots];                // the bytes of the piece in slot k, for zlib if the device hands it back
    uint64_t head = 0, next = 0;
    uint64_t off_from = kNever;            // zlib compresses every piece from this one on
    uint64_t gpu_pieces = 0, cpu_pieces = 0;
    // mode 2, the host model of a slot: the tiles' streams at `stride`, their tables, the framed piece
    struct Model {
        std::vector<uint8_t> slots, framed;
        std::vector<uint32_t> len, crc, off;
        uint32_t total = 0;
    } model[kSlots];

    // what the device does with a piece, on the host: every tile raw-deflated by zlib level 1 into its slot
    // (0xFFFFFFFF: it does not fit the slot), then fc2_bgzf_frame_host
    bool model_submit(int k) {
        if (tile) return model_submit_tiles(k);
        Model &m = model[k];
        const std::string &src = in[k];
        const uint32_t tiles = (uint32_t)((src.size() + block - 1) / block);
        m.slots.assign((size_t)tiles * stride, 0);
        m.len.assign(tiles, 0);
        m.crc.assign(tiles, 0);
        m.off.assign(tiles + 1, 0);
        m.framed.assign((size_t)tiles * (26 + FC2_DEFLATE_TILE_BOUND(block)), 0);
        z_stream z1{};
        if (deflateInit2(&z1, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        for (uint32_t i = 0; i < tiles; ++i) {
            const size_t at = (size_t)i * block, n = std::min<size_t>(block, src.size() - at);
            deflateReset(&z1);
            z1.next_in = (Bytef *)(src.data() + at);
            z1.avail_in = (uInt)n;
            z1.next_out = m.slots.data() + (size_t)i * stride;
            z1.avail_out = stride;
            m.len[i] = deflate(&z1, Z_FINISH) == Z_STREAM_END ? stride - z1.avail_out : 0xFFFFFFFFu;
            m.crc[i] = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)(src.data() + at), (uInt)n);
        }
        deflateEnd(&z1);
        return fc2_bgzf_frame_host(m.slots.data(), stride, m.len.data(), m.crc.data(), tiles, src.size(), block,
                                   m.framed.data(), m.off.data(), &m.total) == FC2_OK;
    }

    // the same for blocks cut into tiles (fc2_deflate_launch_groups, fc2_bgzf_frame_groups_host): a block is one
    // raw stream from zlib level 1, flushed to a byte boundary (Z_SYNC_FLUSH: the empty stored block the device
    // writes too) at every tile's end but the block's last, which finishes it; each tile's part into its slot.
    // zlib's window reaches back 32 KiB inside the block whatever `hist` is: the model stands for the stream
    // form, the tables and the framing, not for the device's bytes
    bool model_submit_tiles(int k) {
        Model &m = model[k];
        const std::string &src = in[k];
        const uint32_t tpg = (block - 1) / tile + 1, blocks = (uint32_t)((src.size() + block - 1) / block);
        const uint32_t tiles = (uint32_t)fc2_deflate_group_tiles(src.size(), block, tile);
        m.slots.assign((size_t)tiles * stride, 0);
        m.len.assign(tiles, 0);
        m.crc.assign(tiles, 0);
        m.off.assign(blocks + 1, 0);
        m.framed.assign((size_t)blocks * kBlockMax, 0);
        z_stream z1{};
        if (deflateInit2(&z1, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        for (uint32_t g = 0; g < blocks; ++g) {
            const size_t g0 = (size_t)g * block, gn = std::min<size_t>(block, src.size() - g0);
            deflateReset(&z1);
            bool fits = true;
            for (size_t t0 = 0; t0 < gn; t0 += tile) {
                const size_t n = std::min<size_t>(tile, gn - t0), i = (size_t)g * tpg + t0 / tile;
                const bool last = t0 + n == gn;
                z1.next_in = (Bytef *)(src.data() + g0 + t0);
                z1.avail_in = (uInt)n;
                z1.next_out = m.slots.data() + i * stride;
                z1.avail_out = stride;
                if (fits) {
                    const int rc = deflate(&z1, last ? Z_FINISH : Z_SYNC_FLUSH);
                    fits = last ? rc == Z_STREAM_END : (rc == Z_OK && z1.avail_out != 0);
                }
                m.len[i] = fits ? stride - z1.avail_out : 0xFFFFFFFFu;      // (0xFFFFFFFF: it does not fit the slot)
                m.crc[i] = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)(src.data() + g0 + t0), (uInt)n);
            }
        }
        deflateEnd(&z1);
        return fc2_bgzf_frame_groups_host(m.slots.data(), stride, m.len.data(), m.crc.data(), tiles, src.size(), block, tile,
                                          m.framed.data(), m.off.data(), &m.total) == FC2_OK;
    }

    // the piece in pend into the next slot (a slot in use: its piece written first)
    bool send_piece() {
        if (next - head == (uint64_t)kSlots && !retire()) return false;
        const uint64_t p = next++;
        const int k = (int)(p % kSlots);
        in[k].swap(pend);
        pend.clear();
        if (p >= off_from) return ok;
        std::string err;
        if (!(mode == 1 ? bgz::gpu_submit(gpu, k, in[k].data(), in[k].size(), err) : model_submit(k))) {
            off_from = p;
            if (mode == 1 && bgz::gpu_hung(gpu)) return fail_timeout(err);
        }
        return ok;
    }

    bool fail_timeout(const std::string &err) {
        timed_out = true;
        dev_err = err;
        return ok = false;
    }

    // the oldest piece in flight to the file: the device's blocks, or zlib's from off_from on
    bool retire() {
        const uint64_t p = head++;
        const int k = (int)(p % kSlots);
        const uint8_t *bytes = nullptr;
        size_t total = 0;
        if (p < off_from) {
            if (mode == 1) {
                std::string err;
                const bgz::Wait wt = bgz::gpu_collect(gpu, k, bytes, total, err);
                if (wt == bgz::TIMED_OUT) return fail_timeout(err);
                if (wt != bgz::DONE) total = 0;
            } else {
                bytes = model[k].framed.data();
                total = model[k].total;
            }
            if (!total) off_from = p;           // the device failed or gave a tile up
        }
        if (p < off_from) {
            if (fwrite(bytes, 1, total, fp) != total) ok = false;
            ++gpu_pieces;
        } else {
            out.resize(kBlockMax);
            for (size_t at = 0; at < in[k].size() && ok; at += block) {
                const size_t bsize = deflate_block(zs, in[k].data() + at, std::min<size_t>(block, in[k].size() - at), out.data());
                if (!bsize || fwrite(out.data(), 1, bsize, fp) != bsize) ok = false;
            }
            ++cpu_pieces;
        }
        in[k].clear();
        return ok;
    }

    bool add_piece(const char *p, size_t n) {
        while (n && ok) {
            const size_t k = std::min(n, piece_bytes - pend.size());
            pend.append(p, k);
            p += k;
            n -= k;
            if (pend.size() == piece_bytes && !send_piece()) return false;
        }
        return ok;
    }

    // the rest as a last piece (its last block short), then every piece in flight, in order
    bool drain() {
        if (!pend.empty() && ok) send_piece();
        while (head < next && ok) retire();
        return ok;
    }

    bool flush_block() {
        if (buf.empty()) return ok;
        out.resize(kBlockMax);
        const size_t bsize = deflate_block(zs, buf.data(), buf.size(), out.data());
        if (!bsize) return ok = false;
        if (fwrite(out.data(), 1, bsize, fp) != bsize) ok = false;
        buf.clear();
        return ok;
    }
    // the encode stage (attach_sam_stage): SAM lines go to it, and come back as records through add
    SamStage *sam = nullptr;
    bool add_sam(const char *line, const char *end, std::string &err) { return sam->add(line, end, err); }

    bool add(const char *p, size_t n) {
        if (mode) return add_piece(p, n);
        while (n) {
            const size_t k = std::min(n, kBlockIn - buf.size());
            buf.append(p, k);
            p += k;
            n -= k;
            if (buf.size() == kBlockIn && !flush_block()) return false;
        }
        return ok;
    }
};

Writer *open_writer(const std::string &path, const std::string &text, const std::vector<std::string> &names,
                    const std::vector<int64_t> &lens, std::string &err, int level) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) {
        err = "IOError: cannot open '" + path + "': " + strerror(errno);
        return nullptr;
    }
    Writer *w = new Writer();
    w->fp = fp;
    w->level = level;
    if (deflateInit2(&w->zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) {
        fclose(fp);
        delete w;
        err = "zlib init failed";
        return nullptr;
    }
    std::string h("BAM\1", 4);
    put<int32_t>(h, (int32_t)text.size());
    h += text;
    put<int32_t>(h, (int32_t)names.size());
    for (size_t i = 0; i < names.size(); ++i) {
        put<int32_t>(h, (int32_t)names[i].size() + 1);
        h += names[i];
        h += '\0';
        put<int32_t>(h, (int32_t)(i < lens.size() ? lens[i] : 0));
    }
    w->add(h.data(), h.size());
    w->flush_block();                      // htslib writes the header in block(s) of its own
    return w;
}

bool write_raw(Writer *w, const uint8_t *rec, size_t n) { return w->add((const char *)rec, n); }

bool write_bulk(Writer *w, const char *p, size_t n, int threads) {
    if (!w->ok) return false;
    if (w->mode) return w->add(p, n);          // (the device mode cuts its own pieces)
    // the current block first (the bytes complete it or stay in it)
    const size_t head = std::min(n, kBlockIn - w->buf.size());
    w->buf.append(p, head);
    p += head;
    n -= head;
    if (w->buf.size() < kBlockIn) return true;
    if (!w->flush_block()) return false;
    const size_t nb = n / kBlockIn;           // whole blocks; the rest starts the next current block
    if (nb) {
        const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), nb));
        std::vector<uint8_t> outb(nb * kBlockMax);
        std::vector<size_t> sz(nb, 0);
        std::atomic<size_t> next{0};
        auto work = [&] {
            z_stream zs{};
            if (deflateInit2(&zs, w->level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return;
            for (size_t b; (b = next.fetch_add(1)) < nb;)
                sz[b] = deflate_block(zs, p + b * kBlockIn, kBlockIn, outb.data() + b * kBlockMax);
            deflateEnd(&zs);
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back(work);
        work();
        for (auto &th : pool) th.join();
        for (size_t b = 0; b < nb && w->ok; ++b)
            if (!sz[b] || fwrite(outb.data() + b * kBlockMax, 1, sz[b], w->fp) != sz[b]) w->ok = false;
        p += nb * kBlockIn;
        n -= nb * kBlockIn;
    }
    w->buf.assign(p, n);
    return w->ok;
}

bool write_sam(Writer *w, const char *line, const char *end, const std::unordered_map<std::string, int> &tid_of,
               std::string &err) {
    if (w->sam) return w->add_sam(line, end, err);
    std::string rec;
    return encode_sam(line, end, tid_of, rec, err) && w->add(rec.data(), rec.size());
}

void attach_sam_stage(Writer *w, SamStage *stage) { w->sam = stage; }
bool sam_stage_set(const Writer *w) { return w && w->sam != nullptr; }
void sam_stage_counts(const Writer *w, uint64_t &gpu_batches, uint64_t &host_batches) {
    gpu_batches = host_batches = 0;
    if (w && w->sam) w->sam->counts(gpu_batches, host_batches);
}

bool encode_sam(const char *line, const char *end, const std::unordered_map<std::string, int> &tid_of,
                std::string &rec, std::string &err) {
    std::vector<std::pair<const char *, const char *>> f;
    for (const char *p = line;;) {
        const char *t = (const char *)memchr(p, '\t', (size_t)(end - p));
        f.emplace_back(p, t ? t : end);
        if (!t) break;
        p = t + 1;
    }
    if (f.size() < 11) {
        err = "ValueError: SAM line with fewer than 11 fields";
        return false;
    }
    auto str = [&](int k) { return std::string(f[k].first, f[k].second); };
    auto tid = [&](const std::string &s) {
        if (s == "*") return -1;
        auto it = tid_of.find(s);
        return it == tid_of.end() ? -1 : it->second;
    };
    const std::string qname = str(0);
    const uint16_t flag = (uint16_t)strtol(str(1).c_str(), nullptr, 10);
    const int32_t ref = tid(str(2));
    const int32_t pos = (int32_t)(strtol(str(3).c_str(), nullptr, 10) - 1);
    const uint8_t mapq = (uint8_t)strtol(str(4).c_str(), nullptr, 10);
    std::vector<uint32_t> cig;
    int64_t rlen = 0;
    const std::string cs = str(5);
    if (cs != "*") {
        uint32_t n = 0;
        for (char c : cs) {
            if (c >= '0' && c <= '9') { n = n * 10 + (uint32_t)(c - '0'); continue; }
            const int op = cigar_op(c);
            if (op < 0) { err = "ValueError: bad CIGAR " + cs; return false; }
            cig.push_back(n << 4 | (uint32_t)op);
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += n;
            n = 0;
        }
    }
    const std::string rn = str(6);
    const int32_t nref = rn == "=" ? ref : tid(rn);
    const int32_t npos = (int32_t)(strtol(str(7).c_str(), nullptr, 10) - 1);
    const int32_t tlen = (int32_t)strtol(str(8).c_str(), nullptr, 10);
    const std::string seq = str(9) == "*" ? std::string() : str(9);
    const std::string qual = str(10);
    const int64_t e = (!(flag & 4) && !cig.empty() && rlen > 0) ? pos + rlen : pos + 1;
    std::string b;
    put<int32_t>(b, ref);
    put<int32_t>(b, pos);
    put<uint8_t>(b, (uint8_t)(qname.size() + 1));
    put<uint8_t>(b, mapq);
    put<uint16_t>(b, (uint16_t)reg2bin(pos, e));
    put<uint16_t>(b, (uint16_t)cig.size());
    put<uint16_t>(b, flag);
    put<int32_t>(b, (int32_t)seq.size());
    put<int32_t>(b, nref);
    put<int32_t>(b, npos);
    put<int32_t>(b, tlen);
    b += qname;
    b += '\0';
    for (uint32_t c : cig) put<uint32_t>(b, c);
    for (size_t k = 0; k < seq.size(); k += 2)
        put<uint8_t>(b, (uint8_t)(nt16(seq[k]) << 4 | (k + 1 < seq.size() ? nt16(seq[k + 1]) : 0)));
    if (qual == "*") b.append(seq.size(), '\xff');
    else for (size_t k = 0; k < seq.size(); ++k) put<uint8_t>(b, (uint8_t)(k < qual.size() ? qual[k] - 33 : 0xff));
    for (size_t k = 11; k < f.size(); ++k) {   // optional fields TG:T:VALUE
        const char *t = f[k].first, *te = f[k].second;
        if (te - t < 5 || t[2] != ':' || t[4] != ':') { err = "ValueError: bad SAM tag"; return false; }
        b.append(t, 2);
        const std::string v(t + 5, te);
        switch (t[3]) {
            case 'A': b += 'A'; b += v.empty() ? '\0' : v[0]; break;
            case 'i': {                        // the smallest integer type that holds it (sam_parse1)
                const long long x = strtoll(v.c_str(), nullptr, 10);
                if (x < 0) {
                    if (x >= INT8_MIN) { b += 'c'; put<int8_t>(b, (int8_t)x); }
                    else if (x >= INT16_MIN) { b += 's'; put<int16_t>(b, (int16_t)x); }
                    else { b += 'i'; put<int32_t>(b, (int32_t)x); }
                } else {
                    if (x <= UINT8_MAX) { b += 'C'; put<uint8_t>(b, (uint8_t)x); }
                    else if (x <= UINT16_MAX) { b += 'S'; put<uint16_t>(b, (uint16_t)x); }
                    else { b += 'I'; put<uint32_t>(b, (uint32_t)x); }
                }
                break;
            }
            case 'f': b += 'f'; put<float>(b, strtof(v.c_str(), nullptr)); break;
            case 'Z': case 'H': b += t[3]; b += v; b += '\0'; break;
            case 'B': {
                if (v.empty()) { err = "ValueError: bad B tag"; return false; }
                const char sub = v[0];
                std::vector<std::string> xs;
                for (size_t p = 1; p < v.size();) {
                    if (v[p] == ',') ++p;
                    size_t q = v.find(',', p);
                    if (q == std::string::npos) q = v.size();
                    xs.push_back(v.substr(p, q - p));
                    p = q;
                }
                b += 'B';
                b += sub;
                put<int32_t>(b, (int32_t)xs.size());
                for (const std::string &x : xs) {
                    switch (sub) {
                        case 'c': put<int8_t>(b, (int8_t)strtol(x.c_str(), nullptr, 10)); break;
                        case 'C': put<uint8_t>(b, (uint8_t)strtoul(x.c_str(), nullptr, 10)); break;
                        case 's': put<int16_t>(b, (int16_t)strtol(x.c_str(), nullptr, 10)); break;
                        case 'S': put<uint16_t>(b, (uint16_t)strtoul(x.c_str(), nullptr, 10)); break;
                        case 'i': put<int32_t>(b, (int32_t)strtol(x.c_str(), nullptr, 10)); break;
                        case 'I': put<uint32_t>(b, (uint32_t)strtoul(x.c_str(), nullptr, 10)); break;
                        case 'f': put<float>(b, strtof(x.c_str(), nullptr)); break;
                        default: err = "ValueError: bad B tag subtype"; return false;
                    }
                }
                break;
            }
            default: err = "ValueError: bad SAM tag type"; return false;
        }
    }
    put<int32_t>(rec, (int32_t)b.size());
    rec += b;
    return true;
}

bool device_set(const Writer *w) { return w && w->mode != 0; }

bool set_device(Writer *w, int mode, int device, uint32_t block, uint32_t piece_blocks, double timeout_s, int level,
                uint32_t tile, uint32_t hist, std::string &err, uint32_t depth, uint32_t nice, uint32_t passes) {
    if (!block) block = bgz::kDefaultBlock;
    if (!piece_blocks) piece_blocks = bgz::kDefaultPieceBlocks;
    if (!w || mode < 0 || mode > 2 || block > kBlockIn || piece_blocks > bgz::kMaxPieceBlocks || timeout_s < 0 ||
        (mode == 1 && device < 0)) {
        err = "mode is 0, 1 or 2, block at most 0xff00, piece_blocks at most 1024";
        return false;
    }
    if (w->mode || !w->buf.empty()) {
        err = "call once, before the first record";
        return false;
    }
    if (!mode) return true;
    if ((depth || nice) && (level != 2 || depth < FC2_DEFLATE_DEPTH_MIN || depth > FC2_DEFLATE_DEPTH_MAX ||
                            nice < FC2_DEFLATE_NICE_MIN || nice > FC2_DEFLATE_NICE_MAX)) {
        err = "the search effort needs level 2, depth 1..128 and nice 4..258";
        return false;
    }
    if (passes && (level != 2 || passes < FC2_DEFLATE_PASSES_MIN || passes > FC2_DEFLATE_PASSES_MAX)) {
        err = "the passes need level 2 and are 1..3";
        return false;
    }
    if (tile >= block) tile = 0;                // (a block is one tile)
    if (tile && (hist > 32768u || tile + hist > 65536u || (block - 1) / tile + 1 > 16)) {
        err = "at most 16 tiles a block, a history of at most 32768 bytes, tile and history at most 65536 together";
        return false;
    }
    if (mode == 1 && !(w->gpu = bgz::gpu_open(device, block, piece_blocks, timeout_s, level == 2 && (depth || passes > 1) ? bgz::level_with_search(depth, nice, passes) : level,
                                              tile, hist, err)))
        return false;
    w->mode = mode;
    w->block = block;
    w->tile = tile;
    w->hist = tile ? hist : 0;
    w->stride = (FC2_DEFLATE_TILE_BOUND(tile ? tile : block) + 15u) & ~15u;
    w->piece_bytes = (size_t)block * piece_blocks;
    return true;
}

void device_counts(const Writer *w, uint64_t &gpu_pieces, uint64_t &cpu_pieces) {
    gpu_pieces = w ? w->gpu_pieces : 0;
    cpu_pieces = w ? w->cpu_pieces : 0;
}

bool close_writer(Writer *w, std::string &err, uint64_t *gpu_pieces, uint64_t *cpu_pieces, uint64_t *enc_gpu,
                  uint64_t *enc_host) {
    if (!w) return true;
    std::string sam_err;
    bool sam_ok = true;
    if (w->sam) {                              // the lines it still holds become records before the last flush
        sam_ok = w->sam->finish(sam_err);
        uint64_t g = 0, c = 0;
        w->sam->counts(g, c);
        if (enc_gpu) *enc_gpu = g;
        if (enc_host) *enc_host = c;
        delete w->sam;
        w->sam = nullptr;
    }
    bool ok = w->mode ? w->drain() : w->flush_block();
    ok = ok && sam_ok;
    if (gpu_pieces) *gpu_pieces = w->gpu_pieces;
    if (cpu_pieces) *cpu_pieces = w->cpu_pieces;
    if (w->gpu) bgz::gpu_close(w->gpu);        // (a device that timed out is left alone)
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0,
                                    3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (fwrite(eof, 1, sizeof eof, w->fp) != sizeof eof) ok = false;
    if (fclose(w->fp) != 0) ok = false;
    deflateEnd(&w->zs);
    if (!sam_ok && !sam_err.empty()) err = sam_err;
    else if (!ok) err = w->timed_out ? "IOError: writing spliced_alignments.bam failed: " + w->dev_err : "IOError: writing spliced_alignments.bam failed";
    delete w;
    return ok;
}

}  // namespace bam
}  // namespace fc2
