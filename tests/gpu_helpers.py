"""Helpers that put GPU results and oracle results side by side as numpy arrays."""
import numpy as np

import oracle
from find_circ2_amd import first_tie_arrays
from find_circ2_amd import _native as N

_RC = str.maketrans("ACGTN", "TGCAN")


def _gtag_strings(g12: np.ndarray) -> np.ndarray:
    codes = np.frombuffer(b"ACGTN???", np.uint8)
    g12 = g12.astype(np.int64)
    chars = np.stack([codes[(g12 >> (3 * k)) & 7] for k in range(4)], axis=1)
    return chars.copy().view("S4").ravel()


def gpu_arrays(options, host_pairs, res):
    a = first_tie_arrays(options, host_pairs, res)
    g = _gtag_strings(a["gtag12"])
    # the Splice signal of a '-' hit is rev_comp(gtag) (find_circ.py:949, 954)
    sig = np.array([s.decode()[::-1].translate(_RC) if m else s.decode() for s, m in zip(g, a["minus"])],
                   dtype=object)
    n_t = np.where(a["hit"], a["n_ties"], 0)
    return dict(n_ties=n_t, x=np.where(a["hit"], a["x"], -1), start=a["start"], end=a["end"],
                strand=np.where(a["minus"], "-", "+"), dist=a["dist"], ov=a["ov"], sig=sig,
                err_key=a["err_key"], err_win=a["err_win"], done=a["done"])


def oracle_arrays(r: oracle.OracleResult):
    f = r.first
    hit = r.n_ties > 0
    return dict(n_ties=np.where(hit, r.n_ties, 0), x=np.where(hit, f["x"], -1), start=f["start"], end=f["end"],
                strand=np.array([s.decode() for s in f["strand"]], dtype=object), dist=f["dist"], ov=f["ov"],
                sig=np.array([s.decode() for s in f["gtag"]], dtype=object),
                err_key=r.n_ties == -oracle.ORC_ERR_KEY, err_shape=r.n_ties == -oracle.ORC_ERR_SHAPE)


def assert_same(gpu, orc, mask=None, label=""):
    n = len(gpu["n_ties"])
    m = np.ones(n, bool) if mask is None else mask
    keyerr = orc["err_key"] & m
    assert np.array_equal(gpu["err_key"][m], orc["err_key"][m]), label + " KeyError flags differ"
    shape = orc.get("err_shape", np.zeros(n, bool)) & m
    assert np.array_equal(gpu["err_win"][m], shape[m]), label + " window/shape error flags differ"
    ok = m & ~keyerr & ~shape
    assert np.array_equal(gpu["n_ties"][ok], orc["n_ties"][ok]), _first_diff(gpu, orc, ok, "n_ties", label)
    hit = ok & (orc["n_ties"] > 0)
    for k in ("x", "start", "end", "dist", "ov"):
        assert np.array_equal(np.asarray(gpu[k])[hit], np.asarray(orc[k])[hit]), _first_diff(gpu, orc, hit, k, label)
    for k in ("strand", "sig"):
        a = np.asarray(gpu[k])[hit].astype(str)
        b = np.asarray(orc[k])[hit].astype(str)
        assert np.array_equal(a, b), _first_diff(gpu, orc, hit, k, label)
    return int(hit.sum())


def _first_diff(gpu, orc, m, k, label):
    idx = np.nonzero(m)[0]
    a = np.asarray(gpu[k])[idx]
    b = np.asarray(orc[k])[idx]
    bad = idx[np.nonzero(a.astype(str) != b.astype(str))[0]]
    if len(bad) == 0:
        return label + " " + k
    i = int(bad[0])
    return "%s field %s differs at pair %d: gpu=%s oracle=%s (gpu n_ties=%s x=%s; oracle n_ties=%s x=%s)" % (
        label, k, i, gpu[k][i], orc[k][i], gpu["n_ties"][i], gpu["x"][i], orc["n_ties"][i], orc["x"][i])


# ---- the GPU inflater (csrc/fc2_inflate.hip) through its C entry point -----------------------------
SLOT = 65536                                     # a block's output slot (the BGZF ISIZE limit)


def _inflate_pattern(n):
    """What the output buffer holds before a launch (byte i of the allocation)."""
    return ((np.arange(n, dtype=np.int64) * 197 + 91) & 255).astype(np.uint8)


def inflate_launch(payloads, sizes, crcs=None):
    """fc2_bgzf_inflate_launch over payloads (raw DEFLATE, packed back to back at every byte
    alignment, so that a block's last word holds its neighbour's bytes) claimed to hold sizes bytes
    (with CRC-32s crcs, if given).  The output buffer is pre-filled with _inflate_pattern and has one
    guard slot before the first block's slot and one after the last: (the whole buffer, status)."""
    import ctypes
    import torch
    n = len(payloads)
    off, buf = [], bytearray()
    rng = np.random.default_rng(len(payloads))
    for p in payloads:
        buf += bytes(int(rng.integers(0, 4)))          # payloads at every byte alignment
        off.append(len(buf))
        buf += p
    buf += bytes(64)                                    # readable past every payload
    dev = torch.device("cuda:0")
    src = torch.tensor(np.frombuffer(bytes(buf), np.uint8), device=dev)
    o = torch.tensor(np.array(off, np.uint32).view(np.int32), device=dev)
    ln = torch.tensor(np.array([len(p) for p in payloads], np.uint32).view(np.int32), device=dev)
    sz = torch.tensor(np.array(sizes, np.uint32).view(np.int32), device=dev)
    cr = None if crcs is None else torch.tensor(np.array(crcs, np.uint32).view(np.int32), device=dev)
    dst = torch.tensor(_inflate_pattern((max(1, n) + 2) * SLOT), device=dev)
    st = torch.full((max(1, n),), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().fc2_bgzf_inflate_launch(src.data_ptr(), o.data_ptr(), ln.data_ptr(), sz.data_ptr(),
                                            None if cr is None else cr.data_ptr(), dst.data_ptr() + SLOT, st.data_ptr(),
                                            n, ctypes.c_void_p(stream)))
    torch.cuda.synchronize(dev)
    return dst.cpu().numpy(), st.cpu().numpy()[:n]


def inflate_run(payloads, sizes, crcs=None, contained=False):
    """The kernel over payloads claimed to hold sizes bytes (with CRC-32s crcs, if given): (outputs,
    status).  With `contained`, also asserted: every block, inflated or refused, wrote only inside
    [its slot, its slot + its claimed size rounded up to 16) -- the kernel's last row stores whole
    16-byte pieces -- and nothing in a slot that is not its own, the two guard slots included."""
    d, st = inflate_launch(payloads, sizes, crcs)
    n = len(payloads)
    if contained:
        clean = d == _inflate_pattern(len(d))
        for i in range(n):
            a = (i + 1) * SLOT
            own = min(SLOT, (sizes[i] + 15) // 16 * 16) if sizes[i] <= SLOT else 0
            bad = np.nonzero(~clean[a + own:a + SLOT])[0]
            assert len(bad) == 0, "block %d (status %d, size %d) wrote at byte %d of its slot" % (
                i, st[i], sizes[i], own + int(bad[0]))
        assert clean[:SLOT].all() and clean[(max(1, n) + 1) * SLOT:].all(), "a guard slot was written"
        if n == 0:
            assert clean.all()
    return [d[(i + 1) * SLOT:(i + 1) * SLOT + sizes[i]].tobytes() for i in range(n)], st
