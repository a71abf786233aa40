"""The forged DEFLATE streams of deflate_forge.py, each classified by the CPU inflaters: zlib, and
libdeflate where libdeflate.so.0 loads (the library csrc/fc2_deflate.h prefers for BGZF blocks).

CASES is the one list the GPU test (test_gpu_inflate_forms.py) shares.  A case is

- valid:   zlib reaches the end of the stream with exactly the intended bytes, and so does libdeflate;
- invalid: both refuse the stream;
- split:   the two disagree (zlib refuses, libdeflate 1.10 accepts, in every form found).

split may hold only the forms of SPLIT_FORMS.  Three come down to one condition, a length or
distance codeword the block's code does not contain: the unused codeword of a single 1-bit distance
code, a length symbol in a block without any distance code (libdeflate decodes the code's one
distance, or distance 1), and an incomplete code-length code (no stream of that form was found that
either library accepts: those cases are invalid).  Two more were found while the list was written,
both places where libdeflate 1.10 checks less than RFC 1951 asks and zlib refuses: it does not hold
the header's counts against 286 and 30 and reads what they admit (HLIT 287 and 288, HDIST 31 and
32, the fixed code's symbols 286 and 287 as length 258, its distance code 30 as 32769..), and it
lets the last code-length repeat run past HLIT + HDIST.  Those streams are split where nothing else
is wrong with them, and the device must refuse them as zlib does (`device`); the fixed code's
symbols are invalid cases where they stand where libdeflate has a reason of its own to refuse (a
distance past the output so far)."""
import ctypes
import zlib
from collections import namedtuple

import numpy as np
import pytest

from deflate_forge import (DBASE, DEXT, LBASE, LEXT, Code, Forge, LenOnly, Raw, Sym, cl_plain, cl_rle, expand, kraft,
                           make_code)

Case = namedtuple("Case", "name cls payload want size form device")
SPLIT_FORMS = ("unused distance codeword", "length without a distance code", "incomplete code-length code",
               "counts past 286/30", "repeat past HLIT + HDIST")


# ---- the references ---------------------------------------------------------------------------
def zlib_inflate(payload):
    """The bytes, if zlib reaches the end of the stream; None if it refuses or runs out of input."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return None
    return out if d.eof else None


def _libdeflate():
    try:
        lib = ctypes.CDLL("libdeflate.so.0")
        lib.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
        lib.libdeflate_free_decompressor.argtypes = [ctypes.c_void_p]
        lib.libdeflate_deflate_decompress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                                      ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
        lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
        lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
        lib.libdeflate_deflate_compress_bound.restype = ctypes.c_size_t
        lib.libdeflate_deflate_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
        lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                                    ctypes.c_size_t]
        return lib
    except (OSError, AttributeError):
        return None


LIBDEFLATE = _libdeflate()


def libdeflate_inflate(payload, exact=None):
    """The bytes libdeflate inflates the stream to (into a buffer of `exact` bytes that it must fill,
    as the ingest asks; or of any size up to 128 KiB), None if it refuses."""
    d = LIBDEFLATE.libdeflate_alloc_decompressor()
    try:
        if exact is not None:
            buf = ctypes.create_string_buffer(max(1, exact))
            rc = LIBDEFLATE.libdeflate_deflate_decompress(d, payload, len(payload), buf, exact, None)
            return buf.raw[:exact] if rc == 0 else None
        buf = ctypes.create_string_buffer(1 << 17)
        n = ctypes.c_size_t(0)
        rc = LIBDEFLATE.libdeflate_deflate_decompress(d, payload, len(payload), buf, 1 << 17, ctypes.byref(n))
        return buf.raw[:n.value] if rc == 0 else None
    finally:
        LIBDEFLATE.libdeflate_free_decompressor(d)


def libdeflate_deflate(data, level):
    c = LIBDEFLATE.libdeflate_alloc_compressor(level)
    try:
        cap = LIBDEFLATE.libdeflate_deflate_compress_bound(c, len(data))
        buf = ctypes.create_string_buffer(cap)
        n = LIBDEFLATE.libdeflate_deflate_compress(c, data, len(data), buf, cap)
        assert n
        return buf.raw[:n]
    finally:
        LIBDEFLATE.libdeflate_free_compressor(c)


# ---- codes and tokens -------------------------------------------------------------------------
def spread(lengths, n, seed, keep=()):
    """`lengths` dealt to n symbols in a seeded random order (the rest 0); the symbols of `keep` get
    the longest codewords."""
    rng = np.random.default_rng(seed)
    syms = [int(s) for s in rng.permutation(n)]
    syms = [s for s in syms if s not in keep][:len(lengths) - len(keep)] + list(keep)
    out = [0] * n
    for s, l in zip(syms, sorted(lengths)):
        out[s] = l
    return out


# every symbol in use and 15-bit codewords in both codes; the longest for length 258, the literals
# 0 and 255, end-of-block, and the distance codes of 1 and of 24577..
L15 = spread(make_code(286, 15), 286, 15, keep=(0, 255, 285, 256))
D15 = spread(make_code(30, 15), 30, 16, keep=(0, 29))
assert kraft(L15) == kraft(D15) == 32768 and L15[256] == L15[285] == 15 and D15[29] == 15


def random_tokens(rng, p, count, lits, lens, dists, limit=65536):
    """`count` random tokens after p bytes of output: literals of `lits`, lengths of the symbols `lens`
    (257..285) and distances of the codes `dists`, every match inside the output so far and `limit`."""
    toks = []
    for _ in range(count):
        ds = [d for d in dists if DBASE[d] <= p]
        if lens and ds and rng.random() < 0.4:
            s = int(rng.choice(lens)) - 257
            length = min(LBASE[s] + int(rng.integers(0, 1 << LEXT[s])), 257 if s == 27 else 258)
            d = int(rng.choice(ds))
            dist = min(DBASE[d] + int(rng.integers(0, 1 << DEXT[d])), p)
            if p + length <= limit:
                toks.append((length, dist))
                p += length
                continue
        if p < limit:
            toks.append(int(rng.choice(lits)))
            p += 1
    return toks, p


def _random_case(seed):
    """1-6 blocks of random types; the dynamic ones with random complete codes of random maximum length
    7-15 over random symbol sets."""
    rng = np.random.default_rng(seed)
    f, out = Forge(), bytearray()
    nblocks = int(rng.integers(1, 7))
    for b in range(nblocks):
        final = b == nblocks - 1
        kind = int(rng.integers(0, 3))
        if kind == 0:
            data = rng.integers(0, 256, int(rng.integers(0, 2000)), dtype=np.uint8).tobytes()
            if len(out) + len(data) > 65536:
                data = b""
            f.stored(data, final)
            out += data
            continue
        count = int(rng.integers(0, 3000))
        if kind == 1:
            toks, _ = random_tokens(rng, len(out), count, list(range(256)), list(range(257, 286)), list(range(30)))
            f.fixed(toks, final)
        else:
            ml, md = int(rng.integers(7, 16)), int(rng.integers(7, 16))
            nl = int(rng.integers(max(ml + 1, 20), min(1 << ml, 286) + 1))
            syms = [256] + [int(s) for s in rng.permutation(286) if s != 256][:nl - 1]
            if not any(s < 256 for s in syms):
                syms[1] = 65
            nlen = max(max(syms) + 1, 257)
            ll = [0] * nlen
            for s, l in zip(syms, rng.permutation(make_code(nl, ml))):
                ll[s] = int(l)
            nd = int(rng.integers(md + 1, 31))
            dsyms = [int(s) for s in rng.permutation(30)][:nd]
            dl = [0] * (max(dsyms) + 1)
            for s, l in zip(dsyms, rng.permutation(make_code(nd, md))):
                dl[s] = int(l)
            toks, _ = random_tokens(rng, len(out), count, [s for s in syms if s < 256], [s for s in syms if s > 256],
                                    dsyms)
            f.dynamic(ll, dl, toks, final, cl_ops=cl_rle(ll + dl) if rng.random() < 0.5 else None)
        out += expand(out, toks)
    return bytes(f), bytes(out)


def _eob_only():
    ll = [0] * 257
    ll[256] = 1
    return ll


def _few(lits=(65, 66), lens=(257, 285)):
    """A small complete literal/length code: the literals, end-of-block and the length symbols given."""
    syms = list(lits) + [256] + list(lens)
    ll = [0] * (max(syms) + 1)
    for s, l in zip(syms, make_code(len(syms), len(syms) - 1)):
        ll[s] = l
    return ll


def _cases():
    out = []
    rng = np.random.default_rng(2024)
    noise = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()

    def valid(name, f, want):
        out.append(Case(name, "valid", bytes(f), bytes(want), len(want), None, None))

    def invalid(name, f, size):
        out.append(Case(name, "invalid", bytes(f), None, size, None, None))

    def split(name, f, want, form, device=None):
        out.append(Case(name, "split", bytes(f), bytes(want), len(want), form, device))

    # ---- valid: the forms RFC 1951 allows and zlib's compressor does not write ------------------
    everything = (list(range(256)), list(range(257, 286)), list(range(30)))
    head = [0, 255, (258, 1), (258, 2), (3, 24577), (258, 30000)]
    toks, _ = random_tokens(rng, 30000 + len(expand(noise[:30000], head)), 4000, *everything)
    valid("codes_15bit", Forge().stored(noise[:30000]).dynamic(L15, D15, head + toks, True),
          noise[:30000] + expand(noise[:30000], head + toks))
    toks, _ = random_tokens(rng, 0, 300, *everything)
    valid("codes_15bit_plain_hclen19", Forge().dynamic(L15, D15, toks, True, cl_ops=cl_plain(L15 + D15), hclen=19),
          expand(b"", toks))
    ll, dl = make_code(260, 12), make_code(30, 12)[::-1]
    ops, k, spans = cl_rle(ll + dl), 0, False
    for op in ops:
        n = 1 if isinstance(op, int) else op[1]
        spans |= k < len(ll) < k + n
        k += n
    assert spans and k == 290
    toks, _ = random_tokens(rng, 0, 3000, list(range(256)), list(range(257, 260)), list(range(30)))
    valid("repeat_spans_hlit_hdist", Forge().dynamic(ll, dl, toks, True, cl_ops=ops), expand(b"", toks))
    toks = [65, (3, 1), 66, (258, 1), 65, 66, (4, 1)]
    valid("single_distance_code", Forge().dynamic(_few(lens=(257, 258, 285)), [1], toks, True), expand(b"", toks))
    valid("single_distance_code_second_symbol", Forge().dynamic(_few(), [0, 1], [65, 66, (3, 2), (258, 2)], True),
          expand(b"", [65, 66, (3, 2), (258, 2)]))
    valid("no_distance_code", Forge().dynamic(_few(), [0], [65, 66, 66, 65] * 50, True), b"ABBA" * 50)
    valid("eob_only_code", Forge().dynamic(_eob_only(), [0], [], True), b"")
    valid("eob_only_then_data", Forge().dynamic(_eob_only(), [0], []).fixed([72, 105], True), b"Hi")
    toks, _ = random_tokens(rng, 0, 500, list(range(256)), [], [])
    valid("hlit_257", Forge().dynamic(make_code(257, 9), [1, 1], toks, True), bytes(toks))
    toks, _ = random_tokens(rng, 32768 + 516, 800, *everything)
    toks = [(258, 24577), (258, 32768)] + toks
    valid("hlit_286_hdist_30", Forge().stored(noise[:32768]).dynamic(make_code(286, 9)[::-1], make_code(30, 5), toks, True),
          noise[:32768] + expand(noise[:32768], toks))
    f = Forge().fixed([65])                       # 3 + 8 + 7 bits: the stored block's header starts mid-byte
    assert f.bit_length() % 8 == 2
    valid("stored_after_huffman_mid_byte", f.stored(noise[:300]).dynamic(_few(), [1], [65, (3, 1), (3, 1)]).stored(noise[300:1000], True),
          b"A" + noise[:300] + b"A" * 7 + noise[300:1000])
    f = Forge()
    for _ in range(5):
        f.stored(b"")
    for _ in range(5):
        f.fixed([])
    for _ in range(5):
        f.dynamic(_eob_only(), [0], [])
    for _ in range(3):
        f.stored(b"").fixed([]).dynamic(_few(), [1, 1], [])
    valid("empty_block_runs", f.fixed([65, (10, 1)], False).stored(b"", True), b"A" * 11)
    valid("empty_block_runs_no_output", Forge().fixed([]).dynamic(_eob_only(), [0], []).stored(b"").fixed([], True), b"")
    valid("trailing_bytes", Forge().dynamic(L15, D15, [1, 2, 3, (200, 3)], True).raw_bytes(b"\xff\x00left over\xff"),
          expand(b"", [1, 2, 3, (200, 3)]))
    valid("trailing_bytes_after_stored", Forge().stored(noise[:100], True).raw_bytes(bytes(9)), noise[:100])
    for seed in range(6):
        payload, want = _random_case(7000 + seed)
        valid("random_%d" % seed, payload, want)

    # ---- invalid ---------------------------------------------------------------------------------
    l_inc = list(L15)
    l_inc[285] = 0                                # one 15-bit symbol removed
    invalid("litlen_incomplete", Forge().dynamic(l_inc, D15, [1, 2, 3], True), 3)
    invalid("litlen_incomplete_one_2bit_code", Forge().dynamic([0] * 256 + [2], [1, 1], [], True), 0)
    invalid("dist_incomplete_two_2bit_codes", Forge().dynamic(L15, [2, 2], [1, 2, 3, (5, 2)], True), 8)
    invalid("dist_incomplete_one_2bit_code", Forge().dynamic(L15, [2], [1, 2, 3], True), 3)
    invalid("dist_incomplete_literals_only", Forge().dynamic(_few(), [3, 3, 3, 3, 3, 3, 3], [65, 66] * 20, True), 40)
    invalid("litlen_oversubscribed", Forge().dynamic([1, 1, 1] + [0] * 253 + [2], [1, 1], [], True, eob=False), 0)
    l_over = list(L15)
    l_over[285] = 14
    invalid("litlen_oversubscribed_by_one_15bit", Forge().dynamic(l_over, D15, [1, 2, 3], True), 3)
    invalid("dist_oversubscribed", Forge().dynamic(L15, [1, 1, 1], [1, 2, 3], True), 3)
    invalid("dist_oversubscribed_30", Forge().dynamic(L15, [4] * 17, [1, 2, 3], True), 3)
    cl = [0] * 19
    cl[8] = 1
    invalid("clcode_single_1bit", Forge().dynamic([8] * 257, [8], [], True, eob=False, cl_ops=[8] * 258, cl_lens=cl), 1)
    cl = [0] * 19
    cl[0] = cl[1] = cl[18] = 2
    invalid("clcode_incomplete", Forge().dynamic(_few((65,), ()), [0], [65], True, cl_lens=cl), 1)
    cl = [0] * 19
    cl[0] = cl[1] = cl[18] = 1
    invalid("clcode_oversubscribed", Forge().dynamic(_few((65,), ()), [0], [65], True, cl_lens=cl), 1)
    invalid("no_end_of_block_code", Forge().dynamic(make_code(256, 9) + [0], [1, 1], [1, 2, 3], True, eob=False), 3)
    invalid("block_type_3", Forge().header(True, 3).bits(0x5A5A, 16).raw_bytes(noise[:20]), 20)
    invalid("block_type_3_after_data", Forge().fixed([65]).header(True, 3).raw_bytes(noise[:20]), 21)
    invalid("stored_len_nlen_mismatch", Forge().stored(noise[:100], True, nlen=(~100 & 0xFFFF) ^ 0x0100), 100)
    invalid("stored_len_equals_nlen", Forge().stored(noise[:100], True, nlen=100), 100)
    invalid("fixed_symbol_286", Forge().fixed([Sym(286), Code(0, 5)], True), 258)
    invalid("fixed_symbol_287", Forge().fixed([Sym(287), Code(0, 5)], True), 258)
    invalid("fixed_distance_code_30", Forge().fixed([1, 2, 3, 4, 5, LenOnly(3), Code(30, 5), Raw(0, 13)], True), 8)
    invalid("fixed_distance_code_31", Forge().stored(noise).fixed([LenOnly(3), Code(31, 5), Raw(0, 13)], True), 40003)
    # (a distance is at most 32768, so p + 1 can be one only up to p = 32767; at p = 40000 the
    # farthest distance there is lies inside the output)
    invalid("distance_p_plus_1_at_0", Forge().fixed([(3, 1)], True), 3)
    invalid("distance_p_plus_1_at_0_dynamic", Forge().dynamic(L15, D15, [(258, 1)], True), 258)
    invalid("distance_p_plus_1_at_1000", Forge().stored(noise[:1000]).fixed([(3, 1001)], True), 1003)
    invalid("distance_p_plus_1_at_32767", Forge().stored(noise[:32767]).dynamic(L15, D15, [(258, 32768)], True), 33025)
    invalid("repeat_previous_first", Forge().dynamic(_few(), [1, 1], [65], True, cl_ops=[(16, 3)] + cl_rle((_few() + [1, 1])[3:])), 1)
    whole = bytes(Forge().dynamic(L15, D15, [1, 2, 3], True))
    invalid("cut_in_header", whole[:1], 3)
    invalid("cut_in_code_lengths", whole[:40], 3)
    f = Forge().fixed([200, 65, (200, 1), 66], True)   # 3 + 9 + 8 + 8 bits, then 5 extra bits: 28..33
    invalid("cut_in_extra_bits", bytes(f)[:4], 203)
    invalid("cut_in_codeword", bytes(f)[:1], 203)
    invalid("cut_in_distance_codeword", bytes(Forge().fixed([200, 200, (3, 1), 66], True))[:4], 6)  # 3 + 9 + 9 + 7: 28..33
    invalid("cut_in_stored_bytes", bytes(Forge().stored(noise[:100], True))[:60], 100)
    invalid("cut_in_stored_header", bytes(Forge().stored(noise[:100], True))[:3], 100)
    invalid("cut_before_final_block", Forge().fixed([65, 66]), 2)
    invalid("empty_stream", b"", 0)

    # ---- split: zlib refuses, libdeflate 1.10 accepts --------------------------------------------
    one = _few(lens=(257, 258, 285))
    split("unused_codeword_of_single_distance_code", Forge().dynamic(one, [1], [65, LenOnly(3), Code(1, 1), 66], True), b"AAAAB",
          SPLIT_FORMS[0])
    split("unused_codeword_of_single_distance_code_3", Forge().dynamic(_few((65, 66, 67), (257, 285)), [0, 0, 1],
                                                                       [65, 66, 67, LenOnly(258), Code(1, 1)], True),
          expand(b"", [65, 66, 67, (258, 3)]), SPLIT_FORMS[0])
    split("length_without_distance_code", Forge().dynamic(one, [0], [65, 66, LenOnly(4), Raw(0, 1), 65], True), b"ABBBBBA",
          SPLIT_FORMS[1])
    split("length_without_distance_code_bit_1", Forge().dynamic(one, [0], [65, LenOnly(258), Raw(1, 1)], True), b"A" * 259,
          SPLIT_FORMS[1])
    ll = make_code(257, 9)
    split("repeat_past_hlit_hdist", Forge().dynamic(ll, [1, 1], [65], True, cl_ops=cl_plain(ll) + [1, (16, 3)]), b"A",
          SPLIT_FORMS[4], "refuse")
    split("zero_repeat_past_hlit_hdist", Forge().dynamic(ll, [1, 0], [65], True, cl_ops=cl_plain(ll) + [1, (18, 11)]), b"A",
          SPLIT_FORMS[4], "refuse")
    two = [65, 66]
    split("hlit_287", Forge().dynamic(make_code(287, 9), [1, 1], two, True), b"AB", SPLIT_FORMS[3], "refuse")
    split("hlit_288", Forge().dynamic(make_code(288, 9), [1, 1], two, True), b"AB", SPLIT_FORMS[3], "refuse")
    split("hdist_31", Forge().dynamic(make_code(286, 9), make_code(31, 5), two, True), b"AB", SPLIT_FORMS[3], "refuse")
    split("hdist_32", Forge().dynamic(make_code(286, 9), make_code(32, 5), two, True), b"AB", SPLIT_FORMS[3], "refuse")
    split("fixed_symbol_286_as_length_258", Forge().fixed([65, Sym(286), Code(0, 5)], True), b"A" * 259, SPLIT_FORMS[3], "refuse")
    split("fixed_symbol_287_as_length_258", Forge().fixed([65, Sym(287), Code(0, 5)], True), b"A" * 259, SPLIT_FORMS[3], "refuse")
    split("fixed_distance_code_30_as_32769", Forge().stored(noise).fixed([LenOnly(3), Code(30, 5), Raw(0, 14)], True),
          noise + noise[40000 - 32769:40000 - 32769 + 3], SPLIT_FORMS[3], "refuse")
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_class_zlib(case):
    got = zlib_inflate(case.payload)
    if case.cls == "valid":
        assert got == case.want
    else:                                        # (every split form found is one zlib refuses)
        assert got is None


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_class_libdeflate(case):
    if LIBDEFLATE is None:
        pytest.skip("libdeflate.so.0 does not load")
    got = libdeflate_inflate(case.payload)
    if case.cls == "invalid":
        assert got is None
        assert libdeflate_inflate(case.payload, exact=case.size) is None
    else:
        assert got == case.want
        assert libdeflate_inflate(case.payload, exact=case.size) == case.want


def test_split_holds_only_the_known_forms():
    assert {c.cls for c in CASES} == {"valid", "invalid", "split"}
    for c in CASES:
        assert (c.form in SPLIT_FORMS) if c.cls == "split" else (c.form is None and c.device is None), c.name
        assert c.size <= 65536
    assert sum(len(c.payload) for c in CASES) < 1 << 20


def test_forms_asked_for_are_cases():
    names = {c.name: c.cls for c in CASES}
    for name in ("codes_15bit", "repeat_spans_hlit_hdist", "single_distance_code", "no_distance_code", "eob_only_code",
                 "hlit_257", "hlit_286_hdist_30", "stored_after_huffman_mid_byte", "empty_block_runs", "trailing_bytes"):
        assert names[name] == "valid"
    assert sum(n.startswith("random_") for n in names) >= 4


# ---- the helpers themselves ---------------------------------------------------------------------
@pytest.mark.parametrize("n,maxlen", [(2, 1), (3, 2), (19, 7), (30, 15), (30, 5), (32, 5), (257, 9), (286, 15), (286, 9),
                                      (288, 9), (128, 7), (16, 15)])
def test_make_code_is_complete(n, maxlen):
    ls = make_code(n, maxlen)
    assert len(ls) == n and max(ls) == maxlen and kraft(ls) == 32768


def test_forge_matches_zlib_on_plain_streams():
    """Stored, fixed and dynamic blocks of ordinary content: zlib inflates the forged stream to the
    bytes expand() gives."""
    rng = np.random.default_rng(5)
    toks, _ = random_tokens(rng, 0, 20000, list(range(256)), list(range(257, 286)), list(range(30)))
    want = expand(b"", toks)
    for f in (Forge().fixed(toks, True), Forge().dynamic(L15, D15, toks, True),
              Forge().dynamic(L15, D15, toks, True, cl_ops=cl_rle(L15 + D15))):
        assert zlib_inflate(bytes(f)) == want
    data = bytes(rng.integers(0, 256, 65535, dtype=np.uint8))
    assert zlib_inflate(bytes(Forge().stored(data[:7]).stored(data, True))) == data[:7] + data


# ---- match geometry (shared with the GPU test) ---------------------------------------------------
GEOMETRY_MATCHES = [(3, 1), (258, 1), (258, 2), (258, 63), (258, 64), (258, 65), (258, 257), (258, 258), (258, 259),
                    (258, 16126), (258, 16127), (3, 16381), (3, 16382), (3, 32768), (258, 32768), (258, None), (3, None),
                    # the farthest source the ring still holds (dist 16384, whatever the length), and the
                    # first it does not: the hand-over itself (dist + len 16384 / 16385, above) lies
                    # where both copy paths are right, so only these pin how far the ring path may reach
                    (3, 16384), (258, 16384), (3, 16385), (258, 16385)]


GEOMETRY_POSITIONS = [(16384, -300), (16384, -1), (16384, 0), (4096, -1), (4096, 1)]


def geometry_plan(outputs=16):
    """For each of `outputs` outputs the (p, len, dist) placed in it, p ascending: every match of
    GEOMETRY_MATCHES (dist None: p itself) before every kind of position of GEOMETRY_POSITIONS
    (unit * k + offset: on and around the ring's wrap and the flush granule), at a k where it fits,
    and then at as many further k as the outputs have room for.  (Positions one or two bytes apart
    cannot both start a match in one output: the outputs take the offsets -1 and 0 / +1 in turn.)"""
    where = {}
    for unit, off in GEOMETRY_POSITIONS:
        for k in range(1, 65536 // unit + 1):
            where.setdefault(unit * k + off, []).append((unit, off))
    count = {(pos, m): 0 for pos in GEOMETRY_POSITIONS for m in GEOMETRY_MATCHES}
    plan = []
    for i in range(outputs):
        p, here = 0, []
        for pos in sorted(where):
            fits = []
            for kind in where[pos]:
                if kind[1] in ((0, 1) if i % 2 == 0 else (-1,)):
                    continue
                for m in GEOMETRY_MATCHES:
                    dist = pos if m[1] is None else m[1]
                    if pos >= p and dist <= min(pos, 32768) and pos + m[0] <= 65536:
                        fits.append((count[kind, m], -kind[0], GEOMETRY_MATCHES.index(m), kind, m, dist))
            if fits:
                _, _, _, kind, m, dist = min(fits)
                count[kind, m] += 1
                here.append((pos, m[0], dist))
                p = pos + m[0]
        plan.append(here)
    assert min(count.values()) >= 1, [k for k, v in count.items() if not v]
    return plan


def geometry(kind, seed=31):
    """The outputs of geometry_plan(), one final block each (`kind`: "fixed", or "dyn15" for the
    15-bit codes L15/D15): (payloads, intended outputs).  Between the planned matches: random
    literals, and random matches to keep the symbols few."""
    rng = np.random.default_rng(seed)
    payloads, wants = [], []
    for here in geometry_plan():
        toks, p = [], 0
        for item in here:
            while p < item[0]:                   # fill up to the item's position
                gap = item[0] - p
                if p >= 600 and gap >= 3 and rng.random() < 0.03:
                    n = int(min(gap, 258, rng.integers(3, 600)))
                    toks.append((n, int(rng.integers(1, min(p, 32768) + 1))))
                    p += n
                else:
                    toks.append(int(rng.integers(0, 256)))
                    p += 1
            toks.append((item[1], item[2]))
            p += item[1]
        f = Forge()
        if kind == "fixed":
            f.fixed(toks, True)
        else:
            f.dynamic(L15, D15, toks, True)
        assert f.symbols < 40000
        payloads.append(bytes(f))
        wants.append(expand(b"", toks))
    return payloads, wants


@pytest.mark.parametrize("kind", ["fixed", "dyn15"])
def test_geometry_streams_are_valid(kind):
    payloads, wants = geometry(kind)
    for payload, want in zip(payloads, wants):
        assert zlib_inflate(payload) == want
        if LIBDEFLATE is not None:
            assert libdeflate_inflate(payload, exact=len(want)) == want
