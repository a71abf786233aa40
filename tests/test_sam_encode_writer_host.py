"""The -B writer's encode stage (fc2_ingest_set_bam_out_encode) in its stand-in mode, 2: fc2_sam_encode_host in the
device's place, the batching, the slots' rotation, the order of the writes, the refusals and the errors exactly
the device mode's code.  spliced_alignments.bam is the default writer's file byte for byte at batch caps of 1, 2,
63, 64 and 65 lines (more batches than slots), with the zlib writer and with the BGZF device writer's own
stand-in; its records are among fc2_sam_to_bam's; a line with an `f` tag sends its batch to the host encoder
and changes no byte; a line encode_sam fails on ends the run with the default writer's code and message and
leaves the default writer's file; BAM input takes the setter and does nothing."""
import ctypes
import struct

import pytest

from bgzf_helpers import read_bam
from find_circ2_amd import _native as N
from find_circ2_amd.ingest import NativeIngest
from sam_encode_helpers import E_IO, E_PARAM
from samgen import sam_to_bam
from test_native_caller import _rich_sam


def write_bam(inp, is_bam, path, bam_encode=None, bam_device=None):
    """The anchors of inp to path: ((batches as the stage's device returned them, batches the host encoded), None),
    or (the counts, (code, message)) where the run ends with an error."""
    ing = NativeIngest(inp, is_bam)
    ing.set_bam_out(path, bam_device=bam_device, bam_encode=bam_encode)
    err = None
    try:
        while not ing.eof:
            ing.next_chunk(15, False, False, 500)
        ing.close_bam_out()
    except N.Fc2Error as e:
        err = (e.code, str(e).split(": ", 1)[1])
    counts = ing.bam_encode_counts()
    ing.close()
    return counts, err


def records(path):
    _, data, o = read_bam(path)
    out = []
    while o < len(data):
        n, = struct.unpack_from("<i", data, o)
        out.append(data[o:o + 4 + n])
        o += 4 + n
    return out


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    d = tmp_path_factory.mktemp("samenc")
    sam = str(d / "rich.sam")
    _rich_sam(sam, 1500, seed=31)
    mode0 = str(d / "mode0.bam")
    assert write_bam(sam, False, mode0) == ((0, 0), None)
    return d, sam, mode0


@pytest.mark.parametrize("cap", [1, 2, 63, 64, 65])
def test_stand_in_mode_writes_the_default_writers_file(rich, tmp_path, cap):
    _, sam, mode0 = rich
    out = str(tmp_path / "o.bam")
    (g, h), err = write_bam(sam, False, out, dict(mode=2, max_lines=cap))
    assert err is None
    assert open(out, "rb").read() == open(mode0, "rb").read()
    n = len(records(mode0))
    assert n > 2000 and (g, h) == (-(-n // cap), 0) and g > 4          # every batch but the last holds `cap` lines


def test_text_cap_cuts_batches_and_a_line_over_it_goes_to_the_host(rich, tmp_path):
    _, sam, mode0 = rich
    out = str(tmp_path / "o.bam")
    (g, h), err = write_bam(sam, False, out, dict(mode=2, max_lines=64, max_text=1000))
    assert err is None and open(out, "rb").read() == open(mode0, "rb").read()
    assert g > len(records(mode0)) // 8 and h == 0                      # a few lines a batch
    (g, h), err = write_bam(sam, False, out, dict(mode=2, max_lines=64, max_text=150))
    assert err is None and open(out, "rb").read() == open(mode0, "rb").read()
    assert h > 1000                                                     # no batch holds a line of 200 bytes or more


def test_stand_in_mode_in_front_of_the_device_writers_stand_in(rich, tmp_path):
    _, sam, _ = rich
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    dev = dict(mode=2, block=4096, piece_blocks=3)
    assert write_bam(sam, False, a, None, dev) == ((0, 0), None)
    (g, h), err = write_bam(sam, False, b, dict(mode=2, max_lines=100), dev)
    assert err is None and g > 4 and h == 0
    assert open(a, "rb").read() == open(b, "rb").read()


def test_records_are_sam_to_bams(rich, tmp_path):
    d, sam, mode0 = rich
    whole = str(tmp_path / "whole.bam")
    sam_to_bam_native(sam, whole)
    every = records(whole)
    out = str(tmp_path / "o.bam")
    assert write_bam(sam, False, out, dict(mode=2, max_lines=64))[1] is None
    pool = set(every)
    written = records(out)
    assert all(r in pool for r in written)       # (-B writes a mate's anchors by position, not in the input's order)
    assert 2000 < len(written) < len(every)


def sam_to_bam_native(sam, path):
    N.check(N.lib().fc2_sam_to_bam(sam.encode(), path.encode()))


def _tagged(rich, tmp_path, tag):
    """The rich SAM with `tag` appended to the lines of the read whose record is the middle one written."""
    _, sam, mode0 = rich
    recs = records(mode0)
    mid = recs[len(recs) // 2]
    qname = mid[36:36 + mid[12] - 1]
    lines = open(sam, "rb").read().split(b"\n")
    hit = [i for i, l in enumerate(lines) if l.split(b"\t")[0] == qname]
    assert hit
    for i in hit:
        lines[i] += b"\t" + tag
    path = str(tmp_path / "tagged.sam")
    open(path, "wb").write(b"\n".join(lines))
    return path


def test_an_f_tag_in_the_middle_goes_to_the_host_and_changes_no_byte(rich, tmp_path):
    sam = _tagged(rich, tmp_path, b"XF:f:0.5")
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    assert write_bam(sam, False, a) == ((0, 0), None)
    assert any(b"XFf" in r for r in records(a))                         # (the line is one of those written)
    (g, h), err = write_bam(sam, False, b, dict(mode=2, max_lines=64))
    assert err is None and h >= 1 and g > 4
    assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.parametrize("cap", [1, 64, 16384])
def test_a_line_the_encoder_rejects_ends_the_run_as_the_default_writer_does(rich, tmp_path, cap):
    sam = _tagged(rich, tmp_path, b"XQ:q:1")
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    _, err0 = write_bam(sam, False, a)
    assert err0 is not None and err0[0] == E_IO and err0[1] == "ValueError: bad SAM tag type"
    _, err = write_bam(sam, False, b, dict(mode=2, max_lines=cap))      # (cap 16384: the error surfaces at the close)
    assert err == err0
    assert open(a, "rb").read() == open(b, "rb").read()                 # the records before the line, none after it
    assert 100 < len(records(a)) < len(records(rich[2]))


def test_bam_input_takes_the_setter_and_does_nothing(rich, tmp_path):
    d, sam, _ = rich
    bam = str(tmp_path / "rich.bam")
    sam_to_bam(open(sam).read(), bam)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    assert write_bam(bam, True, a) == ((0, 0), None)
    assert write_bam(bam, True, b, dict(mode=2, max_lines=64)) == ((0, 0), None)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_setters_refusals(rich, tmp_path):
    _, sam, _ = rich
    L = N.lib()
    ing = NativeIngest(sam, False)
    assert L.fc2_ingest_set_bam_out_encode(ing.h, 2, 0) == E_PARAM              # before fc2_ingest_set_bam_out
    assert L.fc2_ingest_set_bam_out_encode_caps(ing.h, 0, 0, 0.0) == E_PARAM
    ing.set_bam_out(str(tmp_path / "a.bam"))
    for args in [(3, 0), (-1, 0), (1, -1)]:
        assert L.fc2_ingest_set_bam_out_encode(ing.h, *args) == E_PARAM, args
    for args in [(16385, 0, 0.0), (0, (4 << 20) + 1, 0.0), (0, 0, -1.0)]:
        assert L.fc2_ingest_set_bam_out_encode_caps(ing.h, *args) == E_PARAM, args
    assert L.fc2_ingest_set_bam_out_encode(None, 2, 0) == E_PARAM
    assert L.fc2_ingest_set_bam_out_encode_caps(None, 0, 0, 0.0) == E_PARAM
    assert L.fc2_ingest_set_bam_out_encode(ing.h, 0, 0) == 0                    # off: nothing is set
    assert L.fc2_ingest_set_bam_out_encode_caps(ing.h, 7, 4096, 0.0) == 0
    assert L.fc2_ingest_set_bam_out_encode(ing.h, 2, 0) == 0
    assert L.fc2_ingest_set_bam_out_encode(ing.h, 2, 0) == E_PARAM              # once
    assert L.fc2_ingest_set_bam_out_encode_caps(ing.h, 7, 4096, 0.0) == E_PARAM     # before the stage is set
    g, h = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.fc2_ingest_bam_encode_counts(ing.h, ctypes.byref(g), ctypes.byref(h)) == 0 and (g.value, h.value) == (0, 0)
    assert L.fc2_ingest_bam_encode_counts(None, ctypes.byref(g), ctypes.byref(h)) == E_PARAM
    while not ing.eof:
        ing.next_chunk(15, False, False, 500)
    ing.close_bam_out()
    g, h = ing.bam_encode_counts()                                              # (they outlive the close)
    assert g > 100 and h == 0
    ing.close()
    # after the first record the setters are refused
    ing = NativeIngest(sam, False)
    ing.set_bam_out(str(tmp_path / "b.bam"))
    ing.next_chunk(15, False, False, 50)
    assert L.fc2_ingest_set_bam_out_encode(ing.h, 2, 0) == E_PARAM
    assert L.fc2_ingest_set_bam_out_encode_caps(ing.h, 0, 0, 0.0) == E_PARAM
    ing.close()
