"""Inputs and the read-loop driver shared by test_group_ingest_host.py and test_gpu_group_ingest.py: a
BGZF BAM shaped like the steady-state generator's (scripts/gen_reads.c: 60 % of the fragments unspliced,
the rest spliced), single-end or paired, with unmapped records, unmapped mates and secondaries on other
chromosomes among the unspliced ones; and one run of the native read loop over it."""
import ctypes
import struct

import numpy as np

NAMES = ["chr1", "chr2", "chr3"]


def group_sam(path, n_rich, seed, paired):
    """test_native_caller._rich_sam's spliced fragments (40 %) among unspliced ones (60 %), which come in
    runs; returns the FASTA."""
    from test_native_caller import _rich_sam
    fa = _rich_sam(path, n_rich, seed)
    rng = np.random.default_rng(seed + 1)
    head, frags = [], []
    for line in open(path).read().splitlines():
        if line.startswith("@"):
            head.append(line)
        elif frags and frags[-1][0].split("\t", 1)[0] == line.split("\t", 1)[0]:
            frags[-1].append(line)
        else:
            frags.append([line])

    def read():
        return "".join("ACGT"[k] for k in rng.integers(0, 4, 60)), "".join(chr(35 + int(q)) for q in rng.integers(0, 38, 60))

    def mapped(qn, flag, chrom=None):
        s, q = read()
        return "%s\t%d\t%s\t%d\t60\t60M\t*\t0\t0\t%s\t%s\tNM:i:0\tAS:i:60" % (
            qn, flag | (16 if rng.random() < 0.4 else 0), chrom or NAMES[int(rng.integers(3))], int(rng.integers(1, 80000)), s, q)

    def unmapped(qn, flag=0):
        s, q = read()
        return "%s\t%d\t*\t0\t0\t*\t*\t0\t0\t%s\t%s" % (qn, flag | 4, s, q)

    out, n_un = [], 0
    for f in frags:
        out += f
        for _ in range(int(rng.integers(0, 4))):        # a run of unspliced fragments: 1.5 per spliced one
            qn = "u%05d" % n_un
            n_un += 1
            r = rng.random()
            if paired and r < 0.7:
                recs = [mapped(qn, 0x41), mapped(qn, 0x81)]
                if r < 0.1:
                    recs[1] = unmapped(qn, 0x81)        # the mate did not align
            else:
                recs = [mapped(qn, 0x41 if paired else 0)]
            if rng.random() < 0.1:                      # a secondary elsewhere: another chromosome, never proper
                c = recs[0].split("\t")[2]
                recs.append(mapped(qn, (0x41 if paired else 0) | 256, NAMES[(NAMES.index(c) + 1) % 3]))
            if rng.random() < 0.08:
                recs += [unmapped("x%05d" % n_un)] * int(rng.integers(1, 7))
            out += recs
    with open(path, "w") as fh:
        fh.write("\n".join(head + out) + "\n")
    return fa


def bam_of(sam, path, block=3000, damage=None):
    """The SAM as a BGZF BAM of `block`-byte blocks; damage = a fraction of the file: the first tag of the
    record there gets a type BAM does not know."""
    from samgen import bgzf_compress, sam_to_bam
    sam_to_bam(open(sam).read(), path + ".raw", compress="none")
    data = bytearray(open(path + ".raw", "rb").read())
    if damage is not None:
        l_text, = struct.unpack_from("<i", data, 4)
        o = 8 + l_text
        n_ref, = struct.unpack_from("<i", data, o)
        o += 4
        for _ in range(n_ref):
            l_name, = struct.unpack_from("<i", data, o)
            o += 8 + l_name
        run = 0                                         # ... the first record after three unspliced fragments in a row
        while True:
            bs, _, _, l_name, _, _, n_cig, _, l_seq = struct.unpack_from("<iiiBBHHHi", data, o)
            name = bytes(data[o + 36:o + 36 + l_name - 1])
            if o > len(data) * damage and run >= 3 and not name.startswith(b"u"):
                break
            run = run + 1 if name.startswith(b"u") else 0
            o += 4 + bs
        t = o + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        assert t + 3 <= o + 4 + bs, "the record has tags"
        data[t + 2] = ord("?")
    open(path, "wb").write(bgzf_compress(bytes(data), block=block, level=1))
    return path


def caller_run(path, gpu=False, group=0, digest=None, **opts):
    """The native read loop (fc2_caller_next, every result "no breakpoint") over a BAM: what it handed out
    for evaluation (pair fields and read parts), the text streams and the counters -- or, in their place
    from the failing call on, the error -- then inflate_counts() and group_counts()."""
    from find_circ2_amd import _native as N
    from find_circ2_amd.caller import CallerOptions
    from find_circ2_amd.native_caller import NativeCaller
    nc = NativeCaller(path, True, CallerOptions(**opts), NAMES, genome_dummy=True, gpu_group=group)
    nc.open()
    L = N.lib()
    out, texts, end = [], ["", "", ""], None
    try:
        if gpu:
            ing = L.fc2_caller_ingest(nc.h)
            N.check(L.fc2_ingest_set_gpu_inflate(ing, 0, 1))
            if digest is not None:
                N.check(L.fc2_ingest_set_gpu_digest(ing, int(digest)))
        try:
            while True:
                b, eof = N.CallerBatch(), ctypes.c_int(0)
                N.check(L.fc2_caller_next(nc.h, ctypes.byref(b), ctypes.byref(eof)))
                n = int(b.n)
                assert int(b.n_long) == 0
                if n:
                    pairs = np.frombuffer(ctypes.string_at(b.pairs, 16 * n), N.PAIR_DTYPE)
                    offs = np.frombuffer(ctypes.string_at(b.read_off, 8 * n), np.uint64)
                    reads = ctypes.string_at(b.reads, int((offs + pairs["read_len"]).max()))
                    out += [(pairs[k].tobytes(), reads[int(o):int(o) + int(pairs["read_len"][k])]) for k, o in enumerate(offs)]
                while L.fc2_caller_queued(nc.h) > 0:
                    res = np.zeros(max(n, 1), N.RESULT_DTYPE)
                    res["best_x"] = -1
                    N.check(L.fc2_caller_submit(nc.h, res.ctypes.data, None, 0, n))
                    for k in range(3):
                        texts[k] += nc._take(k)
                if eof.value:
                    break
            end = sorted(nc.counters().items())
        except N.Fc2Error as ex:
            end = ("error", str(ex))
        c = N.IngestCounts()                            # (after an error: the counts up to it)
        N.check(L.fc2_ingest_counts_get(L.fc2_caller_ingest(nc.h), ctypes.byref(c)))
        counts = tuple(int(getattr(c, f)) for f, _ in c._fields_)
        return (out, texts, end, counts), nc.inflate_counts(), nc.group_counts()
    finally:
        nc.close()
