"""The head rows and the fragment rows of SAM text on the host (csrc/fc2_sam_frag_impl.h through fc2_sam_group_host)
against the rule restated in Python (sam_group_helpers.py), row for row, on hand-built text: every shape the rule
tells apart -- one and two mates, a proper segment, 0 to 5 unmapped lines before the head, 16 and 17 lines in a
fragment, a third mate -- every cause of an unusable line on the way back, forward and as the closer, RNAME `*`,
unknown and listed twice, a last line without `\\n`, the block's first head, a closer past the block, and the row
limits: nothing is written past the lines, and nothing at all when they pass `cap`."""
import ctypes

import numpy as np
import pytest

import sam_group_helpers as H
from find_circ2_amd import _native as N
from sam_encode_helpers import E_PARAM

SHAPES = H.shapes()


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_every_shape_the_rule_tells_apart(k):
    what, frag, closed = SHAPES[k]
    n, starts, heads, frags = H.same_as_rule(H.shape_text(frag))
    assert n == len(frag) + 2
    at = H.head_index(frag)
    assert int(frags[at]["state"]) == (1 if closed else 0), what
    if closed:
        assert int(frags[at]["bytes"]) == int(starts[n - 1]) - int(starts[at])
        assert int(frags[at]["n_records"]) == n - 1 - at
    assert int(frags[0]["state"]) == 0 and int(frags[n - 1]["state"]) == 0      # the first head; no closer


def test_all_shapes_in_one_block():
    n, _, heads, frags = H.same_as_rule(H.all_shapes_text())
    assert int(frags["state"].sum()) > 30 and int((heads["state"] == 0).sum()) >= 3 * len(H.bad_lines())


def test_unusable_lines_are_unusable():
    for what, bad in H.bad_lines():
        _, _, heads, _ = H.same_as_rule(H.text_of([bad]))
        assert heads[0].tobytes() == bytes(16), what
    _, _, heads, _ = H.same_as_rule(H.text_of([H.ln(b"a", 0, b"dup"), H.ln(b"a", 0, b"*"), H.ln(b"a", 0, b"nowhere"), H.ln(b"a", 0, b"chr2")]))
    assert list(heads["tid"]) == [5, -1, -1, 1] and list(heads["state"]) == [1] * 4


def test_block_edges():
    a, b, c = H.ln(b"a"), H.ln(b"b"), H.ln(b"c")
    _, _, _, frags = H.same_as_rule(H.text_of([a, b, c]))
    assert list(frags["state"]) == [0, 1, 0]            # the block's first head; closed by c; its closer is past the block
    n, starts, _, frags = H.same_as_rule(H.text_of([a, b, c], newline=False))
    assert n == 2 and list(starts) == [0, len(a) + 1, len(a) + len(b) + 2]
    assert list(frags["state"]) == [0, 0]               # c has no `\n`: it is not a line of this block
    for text in (b"", b"\n", b"x", b"\n\n\n", a, a + b"\n"):
        H.same_as_rule(text)
    n, _, _, frags = H.same_as_rule(H.text_of([a, H.un(), H.un(), b, H.un(), c]))
    assert [int(x) for x in frags[3]] == [1, 2, 1, 1, len(b) + 1 + len(H.un()) + 1]


def test_generator_shaped_lines_a_third_damaged():
    n, _, heads, frags = H.same_as_rule(H.reads_text(700, 3, damage=0.33))
    assert 0.2 * n < int((heads["state"] == 0).sum()) < 0.5 * n and int(frags["state"].sum()) > 20
    n, _, heads, frags = H.same_as_rule(H.reads_text(700, 4))
    assert heads["state"].all() and int(frags["state"].sum()) > 300


def test_rows_past_cap_are_not_written():
    text = H.reads_text(50, 5)
    n = text.count(b"\n")
    full = H.group_host(text)
    at = H.group_host(text, cap=n)                      # (group_host checks the guard rows)
    assert all(np.array_equal(x, y) for x, y in zip(full[1:], at[1:]))
    assert H.group_host(text, cap=n - 1)[0] == n        # the count, and no row
    assert H.group_host(text, cap=0)[0] == n
    assert H.group_host(b"no newline", cap=0)[0] == 0


def test_arguments():
    L, t = N.lib(), H.table()
    starts, heads, frags = H.outputs(4)
    n = ctypes.c_uint32()
    buf = np.frombuffer(b"a\n", np.uint8).copy()
    call = lambda text, nb, tab, tb, s=starts.ctypes.data: L.fc2_sam_group_host(text, nb, tab, tb, s, heads.ctypes.data,
                                                                               frags.ctypes.data, ctypes.addressof(n), 4)
    assert call(buf.ctypes.data, 2, t.ctypes.data, t.nbytes) == 0
    assert call(None, 0, t.ctypes.data, t.nbytes) == 0 and n.value == 0
    assert call(None, 2, t.ctypes.data, t.nbytes) == E_PARAM
    assert call(buf.ctypes.data, 2, None, t.nbytes) == E_PARAM
    assert call(buf.ctypes.data, 2, t.ctypes.data, t.nbytes - 4) == E_PARAM
    assert call(buf.ctypes.data, (16 << 20) + 1, t.ctypes.data, t.nbytes) == E_PARAM
    assert call(buf.ctypes.data, 2, t.ctypes.data, t.nbytes, None) == E_PARAM
