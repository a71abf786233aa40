"""Python handle of the native SAM/BAM ingest (include/fc2_ingest.h)."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Tuple

from . import _native as N
from .samio import AlignedSegment, parse_sam_line


class NativeIngest:
    """Streams fragments that carry anchor pairs; counts the rest natively."""

    def __init__(self, path: str, is_bam: bool):
        self.h = ctypes.c_void_p()
        from .native_caller import _check          # the reference's exception types (ValueError, IOError)
        _check(N.lib().fc2_ingest_open(path.encode(), int(is_bam), ctypes.byref(self.h)))
        L = N.lib()
        self.references = [L.fc2_ingest_ref_name(self.h, i).decode("latin-1")
                           for i in range(L.fc2_ingest_n_refs(self.h))]
        self.tid_of: Dict[str, int] = {n: i for i, n in enumerate(self.references)}
        self.counts = N.IngestCounts()
        self.eof = False

    def format(self) -> Tuple[str, str]:
        """(``"sam"`` | ``"bam"``, ``"plain"`` | ``"bgzf"`` | ``"gzip"``), detected from the bytes."""
        comp = ctypes.c_int()
        fmt = N.lib().fc2_ingest_format(self.h, ctypes.byref(comp))
        return ("sam", "bam")[fmt], ("plain", "bgzf", "gzip")[comp.value]

    def getrname(self, tid: int) -> str:
        return self.references[tid]

    def next_chunk(self, asize: int, nolinear: bool, noop: bool, max_frags: int) -> List[List[AlignedSegment]]:
        """Records of the next handed-back fragments (up to max_frags fragments read)."""
        p = N.IngestParams(int(asize), int(bool(nolinear)), int(bool(noop)))
        text = ctypes.c_void_p()
        ln, nh = ctypes.c_uint64(), ctypes.c_uint64()
        eof = ctypes.c_int()
        N.check(N.lib().fc2_ingest_next(self.h, ctypes.byref(p), max_frags, ctypes.byref(self.counts),
                                        ctypes.byref(text), ctypes.byref(ln), ctypes.byref(nh), ctypes.byref(eof)))
        self.eof = bool(eof.value)
        if not ln.value:
            return []
        raw = ctypes.string_at(text, ln.value).decode("latin-1")
        frags = []
        for block in raw.split("\n\n"):
            if block:
                frags.append([parse_sam_line(l, self.tid_of) for l in block.split("\n") if l])
        return frags

    def set_bam_out(self, path: str, bam_device=None, bam_encode=None):
        """-B/--bam: anchor alignments to ``path`` (include/fc2_ingest.h).  bam_device: None, or the
        arguments of fc2_ingest_set_bam_out_device as a dict -- mode (1: the records compressed on GPU
        ``device``; 2: by the host model of it, a test setting), device, block, piece_blocks, timeout_s
        (each 0 or absent: the default), level (the GPU compressor's, 1 or 2; absent: 1), tile and hist
        (fc2_ingest_set_bam_out_device_tiles; absent or 0: a block is one tile).  bam_encode: None, or the
        arguments of fc2_ingest_set_bam_out_encode as a dict -- mode (1: a SAM input's written records encoded
        on GPU ``device``; 2: by the host rule in its place, a test setting), device, and max_lines, max_text,
        timeout_s (fc2_ingest_set_bam_out_encode_caps; each 0 or absent: the default)."""
        N.check(N.lib().fc2_ingest_set_bam_out(self.h, path.encode()))
        if bam_device:
            set_bam_out_device(self.h, bam_device)
        if bam_encode:
            set_bam_out_encode(self.h, bam_encode)

    def bam_encode_counts(self) -> Tuple[int, int]:
        """(batches of SAM lines written as the device encoded them, batches encoded line by line on the
        host); final after close_bam_out, (0, 0) without bam_encode."""
        return bam_encode_counts(self.h)

    def bam_out_counts(self) -> Tuple[int, int]:
        """(pieces of spliced_alignments.bam the device compressed, pieces of the device mode zlib
        compressed); final after close_bam_out, (0, 0) without bam_device."""
        return bam_out_counts(self.h)

    def set_gpu_inflate(self, device: int, wait: bool = True):
        """A BGZF input's blocks inflated on GPU ``device`` from the next batch on (include/fc2_ingest.h);
        wait: the device's buffers made now (else meanwhile, the CPU inflating until they are)."""
        N.check(N.lib().fc2_ingest_set_gpu_inflate(self.h, int(device), int(bool(wait))))

    def set_gpu_inflate_from(self, device: int, after_bytes: int):
        """As set_gpu_inflate, with nothing made on the device until ``after_bytes`` of the input were
        read (fc2_ingest_set_gpu_inflate_from; the CLI's default)."""
        N.check(N.lib().fc2_ingest_set_gpu_inflate_from(self.h, int(device), int(after_bytes)))

    def inflate_counts(self) -> Tuple[int, int]:
        """(blocks inflated on the GPU, on the CPU) since set_gpu_inflate."""
        g, c = ctypes.c_uint64(), ctypes.c_uint64()
        N.check(N.lib().fc2_ingest_inflate_counts(self.h, ctypes.byref(g), ctypes.byref(c)))
        return int(g.value), int(c.value)

    def set_gpu_walk(self, on: bool):
        """Whether the blocks the GPU inflates take their record lists from the device too (the default)
        or from host threads (fc2_ingest_set_gpu_walk); holds from the next batch on."""
        N.check(N.lib().fc2_ingest_set_gpu_walk(self.h, int(bool(on))))

    def walk_counts(self) -> Tuple[int, int]:
        """(blocks whose record lists came from the device, blocks walked on the host) of the batches
        the GPU inflated."""
        d, c = ctypes.c_uint64(), ctypes.c_uint64()
        N.check(N.lib().fc2_ingest_walk_counts(self.h, ctypes.byref(d), ctypes.byref(c)))
        return int(d.value), int(c.value)

    def set_gpu_digest(self, on: bool):
        """Whether the parse threads take the derived fields (CIGAR sums, AS / XS, has-QUAL) of the records
        the GPU inflated and listed from the device's digest rows (fc2_ingest_set_gpu_digest) or parse every
        record themselves (the default); needs the device lists, holds from the next batch on."""
        N.check(N.lib().fc2_ingest_set_gpu_digest(self.h, int(bool(on))))

    def digest_counts(self) -> Tuple[int, int]:
        """(records whose fields came from device rows, records the host parsed) of the batches the GPU
        inflated."""
        d, c = ctypes.c_uint64(), ctypes.c_uint64()
        N.check(N.lib().fc2_ingest_digest_counts(self.h, ctypes.byref(d), ctypes.byref(c)))
        return int(d.value), int(c.value)

    def set_gpu_group(self, on: int):
        """Whether the parse threads step over the fragments the device closed -- those whose mates each have
        fewer than two proper segments, found by the GPU that inflated and listed their records
        (fc2_ingest_set_gpu_group) -- or group every record themselves (0, the default).  2 is a test
        setting: the rows are made on the host for the batches the CPU inflates."""
        N.check(N.lib().fc2_ingest_set_gpu_group(self.h, int(on)))

    def group_counts(self) -> Tuple[int, int]:
        """(fragments the parse threads stepped over on the device's word, every other fragment); read it
        once the input is exhausted (the parse threads count ahead of the reader)."""
        d, c = ctypes.c_uint64(), ctypes.c_uint64()
        N.check(N.lib().fc2_ingest_group_counts(self.h, ctypes.byref(d), ctypes.byref(c)))
        return int(d.value), int(c.value)

    def set_gpu_sam_group(self, on: int, device: int = 0):
        """SAM text input: whether the parse threads step over the unspliced fragments that GPU `device` closed
        in the blocks of text the splitter sent it (fc2_ingest_set_gpu_sam_group; 1), or group every line
        themselves (0, the default).  2 is a test setting: the host twin fills the slots' rows.  Before
        reading; a BAM input refuses it."""
        N.check(N.lib().fc2_ingest_set_gpu_sam_group(self.h, int(on), int(device)))

    def sam_group_counts(self) -> Tuple[int, int]:
        """group_counts for set_gpu_sam_group."""
        d, c = ctypes.c_uint64(), ctypes.c_uint64()
        N.check(N.lib().fc2_ingest_sam_group_counts(self.h, ctypes.byref(d), ctypes.byref(c)))
        return int(d.value), int(c.value)

    def close_bam_out(self):
        N.check(N.lib().fc2_ingest_close_bam_out(self.h))

    def close(self):
        if self.h:
            N.lib().fc2_ingest_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _u32(v, default: int) -> int:
    """``v`` (None: ``default``) as the library takes a uint32_t: anything outside it becomes 0xFFFFFFFF, which
    every range check refuses, instead of wrapping into the range."""
    v = default if v is None else int(v)
    return v if 0 <= v <= 0xFFFFFFFF else 0xFFFFFFFF


def set_bam_out_device(h, bam_device) -> None:
    """fc2_ingest_set_bam_out_device on the ingest handle ``h`` (NativeIngest.set_bam_out's bam_device)."""
    d = dict(bam_device)
    if int(d.get("level", 1)) != 1:
        N.check(N.lib().fc2_ingest_set_bam_out_device_level(h, int(d["level"])))
    if d.get("depth") is not None or d.get("nice") is not None:     # level 2's search effort (else its own 8 and 32)
        N.check(N.lib().fc2_ingest_set_bam_out_device_search(h, _u32(d.get("depth"), 8), _u32(d.get("nice"), 32)))
    if d.get("passes") is not None:                                 # level 2's passes (else one)
        N.check(N.lib().fc2_ingest_set_bam_out_device_passes(h, _u32(d["passes"], 1)))
    if int(d.get("tile", 0)) or int(d.get("hist", 0)):
        N.check(N.lib().fc2_ingest_set_bam_out_device_tiles(h, int(d.get("tile", 0)), int(d.get("hist", 0))))
    N.check(N.lib().fc2_ingest_set_bam_out_device(h, int(d.get("mode", 1)), int(d.get("device", 0)), int(d.get("block", 0)),
                                                  int(d.get("piece_blocks", 0)), float(d.get("timeout_s", 0.0))))


def set_bam_out_encode(h, bam_encode) -> None:
    """fc2_ingest_set_bam_out_encode on the ingest handle ``h`` (NativeIngest.set_bam_out's bam_encode)."""
    d = dict(bam_encode)
    if d.get("max_lines") or d.get("max_text") or d.get("timeout_s"):
        N.check(N.lib().fc2_ingest_set_bam_out_encode_caps(h, _u32(d.get("max_lines"), 0), _u32(d.get("max_text"), 0),
                                                           float(d.get("timeout_s") or 0.0)))
    N.check(N.lib().fc2_ingest_set_bam_out_encode(h, int(d.get("mode", 1)), int(d.get("device", 0))))


def bam_encode_counts(h) -> Tuple[int, int]:
    g, c = ctypes.c_uint64(), ctypes.c_uint64()
    N.check(N.lib().fc2_ingest_bam_encode_counts(h, ctypes.byref(g), ctypes.byref(c)))
    return int(g.value), int(c.value)


def bam_out_counts(h) -> Tuple[int, int]:
    g, c = ctypes.c_uint64(), ctypes.c_uint64()
    N.check(N.lib().fc2_ingest_bam_out_counts(h, ctypes.byref(g), ctypes.byref(c)))
    return int(g.value), int(c.value)


def sam_to_bam(sam_path: str, bam_path: str) -> None:
    """BGZF BAM of a SAM file, records encoded as htslib's sam_parse1 does (include/fc2_ingest.h)."""
    N.check(N.lib().fc2_sam_to_bam(sam_path.encode(), bam_path.encode()))
