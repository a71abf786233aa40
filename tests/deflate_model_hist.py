"""One tile of the GPU DEFLATE compressor with a history in front of it (deflate_kernel<level, true>
through fc2_deflate_launch_hist, find_circ2_amd/csrc/fc2_deflate.hip), at both levels: bit-exact, plain
Python, built on deflate_model.py / deflate_model2.py.  Their pass 1 takes no start offset and their
model() writes BFINAL = 1 itself, so pass 1 and the stream's assembly are restated here; the cost rule,
the codes, the run lengths, the bit writer and the CRC are theirs.

The rule (the kernel's header comment states the same):

History.  A launch's n bytes are one DEFLATE stream cut into tiles.  Tile i covers
text[i * tile, min(n, (i + 1) * tile)); its history is the h = min(hist, i * tile) bytes before it.  The
region is history and tile back to back, m = h + (the tile's bytes) <= 65536 long; positions in it are
counted from the history's first byte, so the tile starts at position h.

Pass 1.  Steps of 64 positions are laid over the whole region from position 0 (base = 0, 64, ...), so a
step may hold the last history positions and the first tile positions.  Every position p with
p + 4 <= m -- of the history or of the tile; a history position's four bytes may run into the tile --
enters the heads, and at level 2 writes its link[] entry, as deflate_model says: read first, then enter.
Pass 1 starts with skip = h: the history lies "inside a match" that ends where the tile begins, and that
alone is what keeps a history position from searching and from giving a token.  A tile position searches
as without a history: its candidate is any position below it, of the history too; the distance is at most
32768; the length at most min(258, m - p).  A match whose source starts in the history and runs on into
the tile is an overlapping match like any other.

Not the history's: the bytes' histogram and so the literal cost (the tile's bytes alone, divided by the
tile's length), the CRC-32, the tokens.

Stream.  The launch's last tile is written as without a history, with BFINAL = 1.  Every other tile:
the dynamic block with BFINAL = 0, then an empty stored block -- bits 000, zeros up to the byte boundary,
00 00 FF FF -- so the tile's stream ends on a byte boundary; this form is taken only if its bytes,
estimated as deflate_model estimates the block's and with those at most five bytes counted, are fewer
than the stored form's; the stored form is deflate_model.stored with BFINAL = 0 in every block and nothing
behind it.

Level 2's links.  link[] keeps its 32768 slots, indexed by p & 32767 with p a position of the region; the
walk's rules are deflate_model2's word for word, with n read as m.

model_hist(history, data, level, last, a=0, without=()) -> (stream, info); with no history and last it is
deflate_model.model / deflate_model2.model2 byte for byte.  launch_streams(text, tile, hist, level) ->
[(stream, crc, info)] of a launch, as fc2_deflate_launch_hist leaves them in its slots.

`without` takes the other models' names and: "histsrc" (a candidate in the history is refused), "maxdist"
(no limit on the distance: a longer one is written with the 15 bits a token has for it), "dist32768" (the limit is 32767), "straddle" (the steps are laid from the tile's start, the history's own steps
before them), "litcost" (the literal cost over history and tile), "shorthist" (a history under 4 bytes is
dropped), "nonfinal" (a tile that is not the last is written as the last is), "final" (the last tile is
written as the others are),
"tail" (no empty stored block), "align" (the Huffman form is chosen without its alignment bytes counted),
"firsthist" (a tile whose history would be shorter than hist gets none)."""
import deflate_model
from deflate_model import (CL_ORDER, HASH_BITS, MAX_DIST, MAX_MATCH, MIN_MATCH, _Writer, build_code, crc32, dist_sym,
                           len_sym, literal_cost, run_lengths)
from deflate_model2 import DEPTH, LINKS, NICE, model2


def _hash(v):
    return ((v * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def find_matches_hist(region, h, lit16, level, without=()):
    """Pass 1 over a region whose first h bytes are history: the tile's tokens in position order, the two
    symbol histograms, the tokens' extra bits, and what the search did."""
    m = len(region)
    pad = region + bytes(20)
    htab = [0] * (1 << HASH_BITS)
    link = [0] * LINKS
    lfreq, dfreq = [0] * 288, [0] * 32
    tokens, extra, skip = [], 0, h
    st = dict(deep=0, farther=0, nice=0, lazy=0, window=0, hist_src=0, into_tile=0, d32768=0, too_far=0, chain_into_hist=0,
              entered_hist=0)
    maxdist = MAX_DIST - 1 if "dist32768" in without else MAX_DIST
    depth = DEPTH if level == 2 and "depth" not in without else 1
    if "straddle" in without:
        steps = [(b, min(b + 64, h)) for b in range(0, h, 64)] + [(b, min(b + 64, m)) for b in range(h, m, 64)]
    else:
        steps = [(b, min(b + 64, m)) for b in range(0, m, 64)]
    for base, top in steps:
        word, cand = {}, {}
        for p in range(base, top):                  # read first ...
            v = int.from_bytes(pad[p:p + 4], "little")
            word[p] = v
            if p + MIN_MATCH <= m:
                cand[p] = htab[_hash(v)]
        for p, c1 in cand.items():                  # ... then enter the step's own positions
            hh = _hash(word[p])
            htab[hh] = max(htab[hh], p + 1)
            st["entered_hist"] += p < h
            if level == 2:
                d = p - (c1 - 1)
                link[p & (LINKS - 1)] = d if c1 and (d <= MAX_DIST or "maxdist" in without) else 0
        if skip >= base + 64:
            continue
        found = {}
        for p, c1 in cand.items():
            if not c1 or p < skip:
                continue
            c = c1 - 1
            maxlen = min(m - p, MAX_MATCH)
            best, bestd, fitted, depth_of_best, first = 0, 0, 0, 0, True
            for k in range(depth):
                d = p - c
                if d > maxdist and "maxdist" not in without:
                    st["too_far"] += 1
                    break
                if level == 2 and c + LINKS < base + 64 and "window" not in without:
                    st["window"] += 1
                    break
                if pad[c:c + 4] == pad[p:p + 4] and not (c < h and "histsrc" in without):
                    l = 4
                    while l < maxlen and pad[c + l] == pad[p + l]:
                        l += 1
                    l = min(l, maxlen)
                    fitted += 1
                    if l > best:
                        best, bestd, depth_of_best, first = l, d, k, fitted == 1
                    if best >= maxlen:
                        break
                    if level == 2 and best >= NICE and "nice" not in without:
                        st["nice"] += 1
                        break
                if level != 2:
                    break
                back = link[c & (LINKS - 1)]
                if not back or back > c:
                    break
                c -= back
            if not best:
                continue
            deb = (bestd - 1).bit_length() - 2 if bestd > 4 else 0
            if best * lit16 >= 16 * (11 + deb):
                found[p] = (best, (bestd - 1) % MAX_DIST + 1)      # (another distance only with "maxdist")
                st["deep"] += depth_of_best == DEPTH - 1
                st["farther"] += not first
                st["chain_into_hist"] += c1 - 1 >= h > p - bestd >= 0
        p = max(skip, base)
        while p < top:                              # from the lowest open position on
            if p in found:
                l, d = found[p]
                if level == 2 and "lazy" not in without and p + 1 < base + 64 and p + 1 in found and found[p + 1][0] > l:
                    st["lazy"] += 1
                    tokens.append(pad[p])
                    lfreq[pad[p]] += 1
                    p += 1
                    continue
                tokens.append(("m", l, d))
                st["hist_src"] += p - d < h
                st["into_tile"] += p - d < h < p - d + l
                st["d32768"] += d == MAX_DIST
                s, eb, _ = len_sym(l - 3)
                lfreq[s] += 1
                extra += eb
                s, eb, _ = dist_sym(d - 1)
                dfreq[s] += 1
                extra += eb
                p += l
                skip = p
            else:
                tokens.append(pad[p])
                lfreq[pad[p]] += 1
                p += 1
    lfreq[256] = 1
    return tokens, lfreq, dfreq, extra, st


def stored_open(data):
    """deflate_model.stored with BFINAL = 0 in every block."""
    s = bytearray(deflate_model.stored(data))
    s[0] = 0
    if len(data) > 65535:
        s[5 + 65535] = 0
    return bytes(s)


def model_hist(history, data, level, last, a=0, without=()):
    """The stream of one tile `data` behind `history`, and deflate_model.model's info with kind "stored" or
    "dynamic", est (the bytes the Huffman form was estimated at, its alignment bytes counted), stored_bytes,
    and the search's counters as info["hist"]."""
    history, data = bytes(history), bytes(data)
    if len(history) < 4 and "shorthist" in without:
        history = b""
    h, n = len(history), len(data)
    assert 1 <= n and h + n <= 65536 and h <= 32768 and level in (1, 2) and 0 <= a < 16
    lit16 = literal_cost(history + data if "litcost" in without else data)
    tokens, lfreq, dfreq, extra, st = find_matches_hist(history + data, h, lit16, level, without)
    ok_l, llen, lcode, clip_l = build_code(lfreq, 286, 15, without)
    ok_d, dlen, dcode, clip_d = build_code(dfreq, 30, 15, without)
    ok = ok_l and ok_d
    data_bits = extra + sum(lfreq[s] * llen[s] for s in range(286)) + sum(dfreq[s] * dlen[s] for s in range(30))
    hlit, hdist, rle = 286, 30, []
    if ok:
        while hlit > 257 and llen[hlit - 1] == 0:
            hlit -= 1
        while hdist > 1 and dlen[hdist - 1] == 0:
            hdist -= 1
        rle = run_lengths(llen[:hlit] + dlen[:hdist], without)
    cfreq = [0] * 20
    for s, _ in rle:
        cfreq[s] += 1
    ok_c, clen, ccode, clip_c = build_code(cfreq, 19, 7, without)
    ok = ok and ok_c
    info = dict(ntok=len(tokens), clipped=(clip_l, clip_d, clip_c), maxlen=(max(llen), max(dlen), max(clen)),
                hlit=hlit, hdist=hdist, hclen=0, rle=rle, widest=0, flushes=0, three_word=0,
                dfreq=dfreq[:30], tokens=tokens, crc=crc32(data), hist=st)
    if level == 2:
        info["l2"] = st
    last = (last or "nonfinal" in without) and "final" not in without
    final = last
    out = _Writer(a, without)
    if ok:
        out.put((1 if final else 0) | (2 << 1), 3)
        hclen = 19
        while hclen > 4 and clen[CL_ORDER[hclen - 1]] == 0:
            hclen -= 1
        info["hclen"] = hclen
        out.put(hlit - 257, 5)
        out.put(hdist - 1, 5)
        out.put(hclen - 4, 4)
        for k in range(hclen):
            out.put(clen[CL_ORDER[k]], 3)
        for s, e in rle:
            out.put(ccode[s], clen[s])
            if s >= 16:
                out.put(e, 2 if s == 16 else 3 if s == 17 else 7)
        out.three_word = 0
    tail = not last and "tail" not in without
    if tail and "align" not in without:
        est = ((out.bits + data_bits + 3 + 7) >> 3) + 4
    else:
        est = (out.bits + data_bits + 7) >> 3
    stored_bytes = n + (10 if n > 65535 else 5)
    info["est"], info["stored_bytes"] = est, stored_bytes
    if not (ok and est < stored_bytes):
        info["kind"] = "stored"
        return (deflate_model.stored(data) if final else stored_open(data)), info
    info["kind"] = "dynamic"
    for b0 in range(0, len(tokens), 64):
        for t in tokens[b0:b0 + 64]:
            if isinstance(t, tuple):
                s, eb, ev = len_sym(t[1] - 3)
                bits, nb = lcode[s] | (ev << llen[s]), llen[s] + eb
                s, eb, ev = dist_sym(t[2] - 1)
                bits |= dcode[s] << nb
                nb += dlen[s]
                bits |= ev << nb
                nb += eb
            else:
                bits, nb = lcode[t], llen[t]
            info["widest"] = max(info["widest"], nb)
            out.put(bits, nb)
        out.flush()
    out.put(lcode[256], llen[256])
    if tail:
        out.put(0, 3)
        out.put(0, -out.bits & 7)
        out.put(0xFFFF0000, 32)
    info["flushes"], info["three_word"] = out.flushes, out.three_word
    return out.bytes(), info


def launch_streams(text, tile, hist, level, without=()):
    """[(stream, crc, info)] of the tiles of one launch of fc2_deflate_launch_hist; hist = 0 is
    fc2_deflate_launch_level: every tile a stream of its own."""
    text = bytes(text)
    assert 1 <= tile <= 65536 and 0 <= hist <= 32768 and tile + hist <= 65536
    out = []
    for k in range(0, len(text), tile):
        data = text[k:k + tile]
        if not hist:
            s, info = (model2 if level == 2 else deflate_model.model)(data, 0, without)
        else:
            h = min(hist, k)
            if h < hist and "firsthist" in without:
                h = 0
            s, info = model_hist(text[k - h:k], data, level, k + tile >= len(text), 0, without)
        out.append((s, info["crc"], info))
    return out
