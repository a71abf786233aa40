"""Level 2 of the GPU DEFLATE compressor with more than one parse (deflate_kernel<2, .., .., true, true> through
fc2_deflate_launch_priced, find_circ2_amd/csrc/fc2_deflate.hip): bit-exact, plain Python, in all three launch
shapes.  The kernel's header comment states the same rule ("Priced passes").

The rule.  Pass 1 is level 2's pass 1 with `depth` and `nice` (deflate_model_deep.py), over the region: h bytes of
history, then the tile.  After a pass that is not the last, the literal/length and distance codes are built from
that pass's histograms as they are after the last -- lfreq[256] = 1, build_code(.., 286, 15), build_code(.., 30,
15), dummy symbols and overflow repair as they come out; no code-length code, no header.  If either is not ok, no
further pass runs.  Pass k >= 2 runs pass 1 again from the start of the same region -- heads and histograms zeroed,
no token, no extra bit, skip = h -- with one difference, the cost rule.  With llen and dlen the code lengths just
built,
    lit(b)      = llen[b], or 15 where that is 0;
    match(l, d) = (llen[length symbol] or 15) + the length's extra bits + (dlen[distance symbol] or 15) + the
                  distance's extra bits;
the walk's kept match (the longest; the first found among equals; the same three ends, `nice` and the cap) is a
found match iff the sum of lit over its bytes is strictly more than match(best, bestd).  lit16 is not consulted.
Links, the lazy step, the greedy resolution and history positions that enter but never search are level 2's.  The
last pass's tokens are written -- nothing compares passes -- and everything after it is deflate_model_hist's.

model_priced(data, depth, nice, passes)                          one independent tile
model_hist_priced(history, data, last, depth, nice, passes)      one tile behind a history
hist_streams_priced(text, tile, hist, depth, nice, passes)       a launch with a history (hist = 0: independent tiles)
group_streams_priced(text, group, tile, hist, depth, nice, passes)   groups: [[(stream, crc, info)] per group]
launch_priced(text, group, tile, hist, depth, nice, passes)      fc2_deflate_launch_priced's slots in order

passes = 1 is deflate_model_deep byte for byte: its code runs, not this module's pass.  info["priced"] counts, for
the last pass when it is a priced one: visits (candidates walked) and fit (those whose four bytes were the
position's), dropped (kept matches that the lit16 rule would take and the price refuses), gained (the reverse),
uncoded (terms priced at 15: a byte, a length symbol or a distance symbol without a codeword), and passes (the
passes run).  pass_(..., price=None) is the same walk under the lit16 rule: tests hold it against
deflate_model_hist.find_matches_hist.

`without` takes the other models' names and, for the tests alone: "price15" (a symbol without a codeword costs
nothing), "strict" (a match is found at equal cost too), "rezero" (a further pass adds to the histograms of the
one before)."""
import deflate_model_hist
from deflate_model import HASH_BITS, MAX_DIST, MAX_MATCH, MIN_MATCH, build_code, dist_sym, len_sym
from deflate_model2 import LINKS
from deflate_model_deep import search

PASSES_RANGE = (1, 3)
UNCODED = 15


def _hash(v):
    return ((v * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def pass_(region, h, lit16, depth, nice, price=None, without=(), carry=None):
    """One pass over a region whose first h bytes are history.  price = (llen, dlen): the priced rule; None: the
    lit16 rule.  carry = (lfreq, dfreq): histograms to add to ("rezero").  Returns tokens, lfreq, dfreq, extra and
    the counters."""
    m = len(region)
    pad = region + bytes(20)
    htab = [0] * (1 << HASH_BITS)
    link = [0] * LINKS
    lfreq, dfreq = (list(carry[0]), list(carry[1])) if carry else ([0] * 288, [0] * 32)
    tokens, extra, skip = [], 0, h
    st = dict(visits=0, fit=0, dropped=0, gained=0, uncoded=0)
    none = 0 if "price15" in without else UNCODED

    def coded(length):
        st["uncoded"] += not length
        return length if length else none

    for base in range(0, m, 64):
        top = min(base + 64, m)
        word, cand = {}, {}
        for p in range(base, top):                  # read first ...
            v = int.from_bytes(pad[p:p + 4], "little")
            word[p] = v
            if p + MIN_MATCH <= m:
                cand[p] = htab[_hash(v)]
        for p, c1 in cand.items():                  # ... then enter the step's own positions
            hh = _hash(word[p])
            htab[hh] = max(htab[hh], p + 1)
            d = p - (c1 - 1)
            link[p & (LINKS - 1)] = d if c1 and d <= MAX_DIST else 0
        if skip >= base + 64:
            continue
        found = {}
        for p, c1 in cand.items():
            if not c1 or p < skip:
                continue
            c = c1 - 1
            maxlen = min(m - p, MAX_MATCH)
            best, bestd = 0, 0
            for _ in range(depth):
                d = p - c
                if d > MAX_DIST or c + LINKS < base + 64:
                    break
                st["visits"] += 1
                if pad[c:c + 4] == pad[p:p + 4]:
                    st["fit"] += 1
                    l = 4
                    while l < maxlen and pad[c + l] == pad[p + l]:
                        l += 1
                    l = min(l, maxlen)
                    if l > best:
                        best, bestd = l, d
                    if best >= nice or best >= maxlen:
                        break
                back = link[c & (LINKS - 1)]
                if not back or back > c:
                    break
                c -= back
            if not best:
                continue
            deb = (bestd - 1).bit_length() - 2 if bestd > 4 else 0
            flat = best * lit16 >= 16 * (11 + deb)
            if price is None:
                take = flat
            else:
                llen, dlen = price
                ls, leb, _ = len_sym(best - 3)
                ds, deb2, _ = dist_sym(bestd - 1)
                cost = coded(llen[ls]) + leb + coded(dlen[ds]) + deb2
                lits = sum(coded(llen[b]) for b in pad[p:p + best])
                take = lits >= cost if "strict" in without else lits > cost
                st["dropped"] += flat and not take
                st["gained"] += take and not flat
            if take:
                found[p] = (best, bestd)
        p = max(skip, base)
        while p < top:                              # from the lowest open position on, a longer next one first
            if p in found:
                l, d = found[p]
                if p + 1 < base + 64 and p + 1 in found and found[p + 1][0] > l:
                    tokens.append(pad[p])
                    lfreq[pad[p]] += 1
                    p += 1
                    continue
                tokens.append(("m", l, d))
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


def _check(depth, nice, passes):
    assert PASSES_RANGE[0] <= passes <= PASSES_RANGE[1], passes
    with search(depth, nice):                       # (its assertion on depth and nice)
        pass


def _run(call, depth, nice, passes, without):
    """call() under search(depth, nice) with deflate_model_hist's pass 1 followed by passes - 1 priced ones; every
    tile's info gets "priced"."""
    _check(depth, nice, passes)
    first = deflate_model_hist.find_matches_hist
    done = []

    def passes_(region, h, lit16, level, wo=()):
        assert level == 2
        tokens, lfreq, dfreq, extra, st = first(region, h, lit16, level, wo)
        counters = dict(visits=0, fit=0, dropped=0, gained=0, uncoded=0, passes=1)
        for _ in range(passes - 1):
            lf, df = list(lfreq), list(dfreq)       # (build_code puts its dummy symbols into them)
            ok_l, llen, _, _ = build_code(lf, 286, 15, wo)
            ok_d, dlen, _, _ = build_code(df, 30, 15, wo)
            if not (ok_l and ok_d):
                break
            carry = (lf, df) if "rezero" in wo else None
            tokens, lfreq, dfreq, extra, c = pass_(region, h, lit16, depth, nice, (llen, dlen), wo, carry)
            counters = dict(c, passes=counters["passes"] + 1)
        done.append(counters)
        return tokens, lfreq, dfreq, extra, st

    deflate_model_hist.find_matches_hist = passes_
    try:
        with search(depth, nice):
            out = call()
    finally:
        deflate_model_hist.find_matches_hist = first
    return out, done


def model_hist_priced(history, data, last, depth, nice, passes, a=0, without=()):
    """deflate_model_hist.model_hist at level 2 with `passes` passes: (stream, info)."""
    if passes == 1:
        _check(depth, nice, passes)
        from deflate_model_deep import model_hist_deep
        return model_hist_deep(history, data, last, depth, nice, a, without)
    (stream, info), done = _run(lambda: deflate_model_hist.model_hist(history, data, 2, last, a, without), depth, nice,
                                passes, without)
    assert len(done) == 1
    info["priced"] = done[0]
    return stream, info


def model_priced(data, depth, nice, passes, a=0, without=()):
    """One independent tile: (stream, info)."""
    if passes == 1:
        _check(depth, nice, passes)
        from deflate_model_deep import model_deep
        return model_deep(data, depth, nice, a, without)
    return model_hist_priced(b"", data, True, depth, nice, passes, a, without)


def group_streams_priced(text, group, tile, hist, depth, nice, passes, without=()):
    """deflate_model_groups.group_streams at level 2 with `passes` passes: [[(stream, crc, info)] per group]."""
    from deflate_model_deep import group_streams_deep
    from deflate_model_groups import group_streams
    if passes == 1:
        _check(depth, nice, passes)
        return group_streams_deep(text, group, tile, hist, depth, nice, without)
    out, done = _run(lambda: group_streams(text, group, tile, hist, 2, without), depth, nice, passes, without)
    flat = [t for g in out for t in g]
    assert len(flat) == len(done)
    for (_, _, info), c in zip(flat, done):
        info["priced"] = c
    return out


def hist_streams_priced(text, tile, hist, depth, nice, passes, without=()):
    """A launch that is one stream cut into tiles (hist = 0: every tile a stream of its own): [(stream, crc, info)]."""
    from deflate_model_deep import hist_streams_deep
    if passes == 1:
        _check(depth, nice, passes)
        return hist_streams_deep(text, tile, hist, depth, nice, without)
    text = bytes(text)
    assert 1 <= tile <= 65536 and 0 <= hist <= 32768 and tile + hist <= 65536
    out = []
    for k in range(0, len(text), tile):
        h = min(hist, k)
        last = not hist or k + tile >= len(text)
        s, info = model_hist_priced(text[k - h:k], text[k:k + tile], last, depth, nice, passes, 0, without)
        out.append((s, info["crc"], info))
    return out


def launch_priced(text, group, tile, hist, depth, nice, passes, without=()):
    """The slots of fc2_deflate_launch_priced in the launch's order: group = 0 is the history's shape (hist = 0:
    independent tiles), group >= 1 the groups'."""
    if group:
        return [t for tiles in group_streams_priced(text, group, tile, hist, depth, nice, passes, without) for t in tiles]
    return hist_streams_priced(text, tile, hist, depth, nice, passes, without)
