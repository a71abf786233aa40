"""The record starts of inflated BGZF blocks listed on the GPU (fc2_bam_walk_launch, csrc/fc2_inflate.hip
bam_walk_kernel) against the CPU's walk (fc2_bam_walk_host), row for row: the hand-built blocks of
test_bam_walk_host.py, a seeded fuzz of cuts of a real record stream (a third of them damaged), and
blocks with a non-zero status, which are not read.  Every launch has guard rows and guard slots around
its arrays; the kernel writes inside a block's own row, and of that only what it counts."""
import ctypes

import numpy as np
import pytest

from find_circ2_amd import _native as N
from test_bam_walk_host import CAP, NO_EXIT, host_walk, shapes

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SLOT = 65536
FILL16, FILL32 = 0x5AA5, 0x5AA5C33C


def walk_launch(blocks, status=None):
    """fc2_bam_walk_launch over blocks (block i in slot i, the rest of its slot and a guard slot either
    side holding a byte pattern a walk could stumble over): [(count, exit, starts[:count])], after
    checking that nothing but each row's counted entries and the blocks' count/exit words was written."""
    n = len(blocks)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(n)
    slots = rng.integers(0, 256, (n + 2) * SLOT, dtype=np.uint8)
    for i, b in enumerate(blocks):
        slots[(i + 1) * SLOT:(i + 1) * SLOT + len(b)] = np.frombuffer(b, np.uint8)
    d_slots = torch.tensor(slots, device=dev)
    d_isize = torch.tensor(np.array([len(b) for b in blocks], np.uint32).view(np.int32), device=dev)
    d_status = None if status is None else torch.tensor(np.array(status, np.uint32).view(np.int32), device=dev)
    d_starts = torch.tensor(np.full((n + 2) * CAP, FILL16, np.uint16).view(np.int16), device=dev)
    d_count = torch.tensor(np.full(n + 2, FILL32, np.uint32).view(np.int32), device=dev)
    d_exit = torch.tensor(np.full(n + 2, FILL32, np.uint32).view(np.int32), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().fc2_bam_walk_launch(d_slots.data_ptr() + SLOT, d_isize.data_ptr(),
                                        None if d_status is None else d_status.data_ptr(),
                                        d_starts.data_ptr() + 2 * CAP, d_count.data_ptr() + 4, d_exit.data_ptr() + 4,
                                        n, ctypes.c_void_p(stream)))
    torch.cuda.synchronize(dev)
    starts = d_starts.cpu().numpy().view(np.uint16).reshape(n + 2, CAP)
    count = d_count.cpu().numpy().view(np.uint32)
    ex = d_exit.cpu().numpy().view(np.uint32)
    assert (d_slots.cpu().numpy() == slots).all(), "a slot was written"
    for g in (0, n + 1):
        assert (starts[g] == FILL16).all() and count[g] == FILL32 and ex[g] == FILL32, "a guard row was written"
    out = []
    for i in range(n):
        c = int(count[i + 1])
        assert c <= CAP, (i, c)
        assert (starts[i + 1, c:] == FILL16).all(), "block %d wrote past its %d starts" % (i, c)
        out.append((c, int(ex[i + 1]), [int(x) for x in starts[i + 1, :c]]))
    return out


def test_hand_built_blocks_in_one_launch():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    S = shapes()
    got = walk_launch([b for _, b, _ in S])
    for (label, blk, want), g in zip(S, got):
        assert g == host_walk(blk), label
        assert g == (want[0], want[1], list(want[2])), label


@pytest.fixture(scope="module")
def fuzz_blocks(tmp_path_factory):
    """~2,000 cuts (1..65536 bytes, at random offsets) of the record stream of a bwa-mem-like BAM, a third
    with a few bytes overwritten, and the CPU's lists for them."""
    from samgen import sam_to_bam
    from test_native_caller import _rich_sam
    tmp = tmp_path_factory.mktemp("walk_fuzz")
    sam, raw = str(tmp / "rich.sam"), str(tmp / "raw.bam")
    _rich_sam(sam, 4000, seed=7)
    sam_to_bam(open(sam).read(), raw, compress="none")
    data = open(raw, "rb").read()
    assert len(data) > 4 * SLOT
    rng = np.random.default_rng(2024)
    blocks = []
    for k in range(2000):
        # lengths: every size class, the short ones and the full slot included
        ln = int(rng.integers(1, SLOT + 1)) if k % 4 else int(rng.choice([1, 35, 36, 37, 63, 64, 65, 100, 4096, SLOT]))
        a = int(rng.integers(0, len(data) - ln + 1))
        b = bytearray(data[a:a + ln])
        if k % 3 == 0:
            for _ in range(int(rng.integers(1, 6))):
                b[int(rng.integers(0, ln))] = int(rng.integers(0, 256))
        blocks.append(bytes(b))
    return blocks, [host_walk(b) for b in blocks]


def test_fuzz_equals_the_host_walk(fuzz_blocks):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    blocks, want = fuzz_blocks
    got = walk_launch(blocks)
    bad = [i for i in range(len(blocks)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:5], [(got[i][:2], want[i][:2], len(blocks[i])) for i in bad[:5]])
    assert sum(c > 0 for c, _, _ in want) > 1200 and sum(e == NO_EXIT for _, e, _ in want) > 10
    assert {s % 4 for _, _, st in want for s in st} == {0, 1, 2, 3}


def test_blocks_with_a_status_are_not_read(fuzz_blocks):
    """A block the inflater refused (status != 0): count 0, no exit, whatever its slot holds; the
    others as without a status array."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    blocks, want = fuzz_blocks
    blocks, want = blocks[:200], want[:200]
    rng = np.random.default_rng(5)
    status = [int(rng.integers(1, 17)) if rng.random() < 0.3 else 0 for _ in blocks]
    status[0], status[1], status[-1] = 7, 0, 16
    got = walk_launch(blocks, status)
    for i, s in enumerate(status):
        assert got[i] == ((0, NO_EXIT, []) if s else want[i]), (i, s)
    assert sum(1 for s, w in zip(status, want) if s and w[0]) > 10


def test_launch_arguments():
    L = N.lib()
    assert L.fc2_bam_walk_launch(None, None, None, None, None, None, 0, None) == 0
    assert L.fc2_bam_walk_launch(None, None, None, None, None, None, 3, None) == N.FC2_E_PARAM
    assert L.fc2_bam_walk_launch(ctypes.c_void_p(4098), ctypes.c_void_p(8), None, ctypes.c_void_p(8), ctypes.c_void_p(8),
                                 ctypes.c_void_p(8), 3, None) == N.FC2_E_PARAM
