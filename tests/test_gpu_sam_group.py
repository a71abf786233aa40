"""sam_nl_count_kernel, sam_nl_scan_kernel, sam_nl_fill_kernel, sam_head_kernel and sam_frag_kernel
(fc2_sam_group_launch, csrc/fc2_sam_group.hip) against fc2_sam_group_host, the same rule compiled for the host: the
line count, the starts, the head rows and the fragment rows, row for row, on the hand-built shapes, generator-shaped
lines with a third damaged, blocks of 0 bytes, 1 byte and 1 line, lines of 63, 64, 65 and 70,000 bytes, a `\\n` and a
tab on either side of segment boundaries, no trailing `\\n`, n_lines at cap and one past it; the text sits between
guard bytes that hold newlines and tabs (a read outside it would change the rows), and the rows are followed by guard
rows that must stay as they were."""
import ctypes

import numpy as np
import pytest

import sam_group_helpers as H
from find_circ2_amd import _native as N
from sam_encode_helpers import E_PARAM

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PAD = 67                                                # guard bytes on either side: the text starts at an odd address


def launch(text, cap):
    """fc2_sam_group_launch on a block of text: (rc, n_lines, starts, head rows, fragment rows) as the device left
    them, guard rows included."""
    dev = torch.device("cuda:0")
    guard = (b"\n\tq\t4\t" * PAD)[:PAD]
    d_text = torch.tensor(np.frombuffer(guard + text + guard, np.uint8).copy(), device=dev)
    t = H.table()
    d_table = torch.tensor(t.view(np.int32), device=dev)
    starts, heads, frags = H.outputs(cap)
    d_starts = torch.tensor(starts.view(np.int32), device=dev)
    d_heads = torch.tensor(heads.view(np.uint8), device=dev)
    d_frags = torch.tensor(frags.view(np.uint8), device=dev)
    d_n = torch.full((1,), -7, dtype=torch.int32, device=dev)
    d_scratch = torch.zeros(len(text) // H.SEG + 2, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = N.lib().fc2_sam_group_launch(d_text.data_ptr() + PAD, len(text), d_table.data_ptr(), t.nbytes, d_starts.data_ptr(),
                                      d_heads.data_ptr(), d_frags.data_ptr(), d_n.data_ptr(), cap, d_scratch.data_ptr(),
                                      ctypes.c_void_p(stream))
    torch.cuda.synchronize(dev)
    assert d_text.cpu().numpy().tobytes() == guard + text + guard
    return (rc, int(d_n.cpu().numpy().view(np.uint32)[0]), d_starts.cpu().numpy().view(np.uint32),
            d_heads.cpu().numpy().view(H.HEAD), d_frags.cpu().numpy().view(H.FRAG))


def same_as_host(text, cap=None):
    """The device's rows against the host twin's; returns the twin's."""
    want = H.group_host(text, cap)
    n = want[0]
    cap = n if cap is None else cap
    rc, got_n, starts, heads, frags = launch(text, cap)
    assert rc == 0, N.lib().fc2_last_error()
    assert got_n == n
    H.check_guards(n, cap, starts, heads, frags)
    if n <= cap:
        assert np.array_equal(starts[:n + 1], want[1]), "starts"
        assert np.array_equal(heads[:n], want[2]), "head rows"
        assert np.array_equal(frags[:n], want[3]), "fragment rows"
    return want


def test_hand_built_shapes():
    _, _, heads, frags = same_as_host(H.all_shapes_text())
    assert int(frags["state"].sum()) > 30 and int((heads["state"] == 0).sum()) > 30
    for _, frag, _ in H.shapes()[:24:3]:
        same_as_host(H.shape_text(frag))


def test_generator_shaped_lines_a_third_damaged():
    n, _, heads, frags = same_as_host(H.reads_text(1800, 31, damage=0.33))
    assert n > 3000 and 0.2 * n < int((heads["state"] == 0).sum()) < 0.5 * n and int(frags["state"].sum()) > 50
    n, _, heads, frags = same_as_host(H.reads_text(1800, 32))
    assert heads["state"].all() and int(frags["state"].sum()) > 800


@pytest.mark.parametrize("text", [b"", b"\n", b"x", b"\t", H.ln(b"a"), H.ln(b"a") + b"\n", b"\n" * 5, H.ln(b"a") + b"\n" + H.ln(b"b")],
                         ids=["0 bytes", "a newline", "1 byte", "a tab", "no newline", "1 line", "blank lines", "no trailing newline"])
def test_smallest_blocks(text):
    same_as_host(text)


@pytest.mark.parametrize("size", [63, 64, 65, 127, 128, 129, 70000])
def test_line_lengths(size):
    """Lines of exactly `size` bytes: the tabs of the 11 fields spread so that the 10th lies in the line's last
    ballot, between short lines; and one whose QNAME ends at byte 62, 63 or 64."""
    base = H.ln(b"long")
    fill = size - len(base)
    lines = [H.ln(b"a")]
    if fill >= 0:
        lines.append(H.ln(b"long", seq=b"ACGTACGTAC" + b"A" * fill))                # SEQ grows: the 10th tab moves to the end
        lines.append(H.ln(b"long", 2048, b"chr2", tags=[b"XZ:Z:" + b"z" * max(0, fill - 6 - 1)]))
    for q in (62, 63, 64, 65):
        lines.append(H.ln(b"n" * q))
    lines.append(H.ln(b"b"))
    assert fill < 0 or len(lines[1]) == size
    n, _, heads, frags = same_as_host(H.text_of(lines))
    assert heads["state"].all() and int(frags["state"].sum()) >= 4


def padded(base, size):
    """The line grown to `size` bytes by a Z tag."""
    assert size >= len(base) + 6
    return base + b"\tXZ:Z:" + b"z" * (size - len(base) - 6)


def test_a_newline_on_either_side_of_every_segment_boundary():
    """Over 40 segments: a line's `\\n` on the last byte of a segment or on the first byte of the next, in turn; every
    fourth time on both, a blank line between them."""
    lines, at = [], 0
    for s in range(1, 41):
        edge = s * H.SEG
        lines.append(H.ln(b"r%d" % s, 65))
        at += len(lines[-1]) + 1
        lines.append(padded(H.ln(b"r%d" % s, 129), (edge - 1 if s % 2 else edge) - at))
        at += len(lines[-1]) + 1
        if s % 4 == 1:
            lines.append(b"")
            at += 1
    text = H.text_of(lines)
    for s in range(1, 41):
        assert text[s * H.SEG - 1 if s % 2 else s * H.SEG] == 10
        assert s % 4 != 1 or text[s * H.SEG] == 10
    _, _, _, frags = same_as_host(text)
    assert int(frags["state"].sum()) >= 10               # (a blank line keeps the fragments on either side of it open)


def test_tabs_at_segment_boundaries():
    """Lines of 254-byte names and short ones placed so that the first, second and tenth tab of a line lie on the
    last byte of a segment and on the first byte of the next."""
    tabs_of = lambda l: [i for i, c in enumerate(l) if c == 9]
    hits = 0
    for which in (0, 1, 9):
        for edge in (H.SEG - 1, H.SEG, 2 * H.SEG - 1, 2 * H.SEG):
            probe = H.ln(b"probe")
            lead = edge - tabs_of(probe)[which]         # the probe line starts here
            filler, room = [], lead
            while room > 0:                             # lines that fill exactly `room` bytes, newline included
                base = H.ln(b"f%d" % len(filler))
                n = min(room, 400)
                if room - n and room - n < len(base) + 8:
                    n = room - len(base) - 8
                line = base + b"\tXZ:Z:" + b"z" * (n - 1 - len(base) - 6)
                assert len(line) + 1 == n
                filler.append(line)
                room -= n
            text = H.text_of(filler + [probe, H.ln(b"end")])
            assert text[edge] == 9
            hits += 1
            same_as_host(text)
    assert hits == 12


def test_rows_at_cap_and_one_past_it():
    text = H.reads_text(300, 33)
    n = text.count(b"\n")
    full = same_as_host(text, cap=n)
    assert int(full[3]["state"].sum()) > 100
    assert same_as_host(text, cap=n - 1)[0] == n        # one line past the rows: the count, and no row
    assert same_as_host(text, cap=1)[0] == n
    assert same_as_host(b"one line\n", cap=1)[0] == 1
    assert same_as_host(b"one line\ntwo\n", cap=1)[0] == 2


def test_many_segments_and_a_grid_that_strides():
    """3 MB: 3,000 segments (three counts a scan thread), 17,000 lines (more than the head grid's 16,384 waves)."""
    text = H.reads_text(9000, 34, damage=0.1)
    n, _, _, frags = same_as_host(text)
    assert n > 16500 and len(text) > 2500 * H.SEG and int(frags["state"].sum()) > 2000


def test_text_over_the_limit_is_refused_before_any_launch():
    starts, heads, frags = H.outputs(4)
    dev = torch.device("cuda:0")
    d = [torch.tensor(a.view(np.uint8), device=dev) for a in (starts, heads, frags)]
    t = H.table()
    d_table = torch.tensor(t.view(np.int32), device=dev)
    d_n = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = N.lib().fc2_sam_group_launch(d_table.data_ptr(), (16 << 20) + 1, d_table.data_ptr(), t.nbytes, d[0].data_ptr(), d[1].data_ptr(),
                                      d[2].data_ptr(), d_n.data_ptr(), 4, d_table.data_ptr(), None)
    torch.cuda.synchronize(dev)
    assert rc == E_PARAM and int(d_n.cpu()[0]) == -7
    assert all(H.untouched(x.cpu().numpy(), 0) for x in d)
