"""Level 2 of the GPU DEFLATE compressor (deflate_kernel<2>, find_circ2_amd/csrc/fc2_deflate.hip) as
deflate_model.py is level 1's: bit-exact, plain Python.  Level 2 changes pass 1 alone -- which matches
are found and which are taken; the cost rule, the codes, the header and the stream are deflate_model's.

The level-2 rule (the kernel's header comment states the same):

Links.  Beside the table of heads (the last position + 1 per hash, as at level 1) there is link[], one
16-bit entry per position, indexed by p & 32767: the distance from p back to the head its step read for
it before the step's own positions were entered (1..32768), or 0 for none -- no head, or one more than
32768 back.  Every position with p + 4 <= n writes its entry where it enters itself into the heads.

Search.  A position p >= skip walks at most 8 candidates: the head it read, then c - link[c & 32767]
(so every candidate lies strictly below the one before).  The walk ends before a candidate that is
none, that is more than 32768 back, or whose link slot this very step has rewritten
(c + 32768 < base + 64: position c + 32768 is one of the step's own).  A candidate whose first four
bytes are p's gets its length as at level 1, at most min(n - p, 258); the longest is kept, the first
found (the nearest) among equal ones; once the kept length reaches 32 or the cap the walk ends.  The
kept match must pass level 1's cost rule.

Lazy resolution.  Going up from the lowest open position of the step: the match at step index i is
dropped for a literal if i + 1 < 64 and index i + 1 found a longer one; else it is taken as at level 1.
Nothing is deferred from index 63 to the next step.

model2(data, a=0, without=()) -> (stream, info) as deflate_model.model, info["l2"] counting what the
search did: deep (matches kept from the 8th candidate), farther (kept matches that were not the first
candidate whose four bytes fitted), nice (walks ended by a length >= 32 below the cap), lazy (matches
dropped for a literal), window (walks ended by a rewritten slot).  `without` takes deflate_model's
names and "depth" (one candidate only), "lazy", "nice" (no end at 32), "window" (no end at a rewritten
slot: the stale entry is followed)."""
import deflate_model
from deflate_model import (HASH_BITS, MAX_DIST, MAX_MATCH, MIN_MATCH, dist_sym, len_sym)

DEPTH, NICE, LINKS = 8, 32, 32768


def find_matches2(data, lit16, without=()):
    """Pass 1 at level 2: deflate_model.find_matches' results, and the search's counters."""
    n = len(data)
    pad = data + bytes(20)
    htab = [0] * (1 << HASH_BITS)
    link = [0] * LINKS
    lfreq, dfreq = [0] * 288, [0] * 32
    tokens, extra, skip = [], 0, 0
    stats = dict(deep=0, farther=0, nice=0, lazy=0, window=0)
    depth = 1 if "depth" in without else DEPTH
    for base in range(0, n, 64):
        top = min(base + 64, n)
        word, cand = {}, {}
        for p in range(base, top):                  # read first ...
            v = int.from_bytes(pad[p:p + 4], "little")
            word[p] = v
            if p + MIN_MATCH <= n:
                cand[p] = htab[((v * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)]
        for p, c1 in cand.items():                  # ... then enter the step's own positions
            h = ((word[p] * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)
            htab[h] = max(htab[h], p + 1)
            link[p & (LINKS - 1)] = p - (c1 - 1) if c1 and p - (c1 - 1) <= MAX_DIST else 0
        if skip >= base + 64:
            continue
        found = {}
        for p, c1 in cand.items():
            if not c1 or p < skip:
                continue
            c = c1 - 1
            maxlen = min(n - p, MAX_MATCH)
            best, bestd, fitted, depth_of_best = 0, 0, 0, 0
            for k in range(depth):
                d = p - c
                if d > MAX_DIST:
                    break
                if c + LINKS < base + 64 and "window" not in without:
                    stats["window"] += 1
                    break
                if pad[c:c + 4] == pad[p:p + 4]:
                    l = 4
                    while l < maxlen and pad[c + l] == pad[p + l]:
                        l += 1
                    l = min(l, maxlen)
                    fitted += 1
                    if l > best:
                        best, bestd, depth_of_best, first = l, d, k, fitted == 1
                    if best >= maxlen:
                        break
                    if best >= NICE and "nice" not in without:
                        stats["nice"] += 1
                        break
                back = link[c & (LINKS - 1)]
                if not back or back > c:            # (back > c: only a stale entry, without "window")
                    break
                c -= back
            if not best:
                continue
            deb = (bestd - 1).bit_length() - 2 if bestd > 4 else 0
            if best * lit16 >= 16 * (11 + deb):
                found[p] = (best, bestd)
                stats["deep"] += depth_of_best == DEPTH - 1
                stats["farther"] += not first
        p = max(skip, base)
        while p < top:                              # from the lowest position on, a longer next one first
            if p in found:
                l, d = found[p]
                if "lazy" not in without and p + 1 < base + 64 and p + 1 in found and found[p + 1][0] > l:
                    stats["lazy"] += 1
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
    return tokens, lfreq, dfreq, extra, stats


def model2(data, a=0, without=()):
    """deflate_model.model with pass 1 at level 2: the stream deflate_kernel<2> writes for one tile, and
    model's info with the search's counters as info["l2"]."""
    stats = {}

    def pass1(d, lit16):
        tokens, lfreq, dfreq, extra, st = find_matches2(d, lit16, without)
        stats.update(st)
        return tokens, lfreq, dfreq, extra

    # everything after pass 1 is level 1's own code: model() with its find_matches exchanged for the call
    level1 = deflate_model.find_matches
    deflate_model.find_matches = pass1
    try:
        stream, info = deflate_model.model(data, a, without)
    finally:
        deflate_model.find_matches = level1
    assert stats, "deflate_model.model() no longer calls the module's find_matches: level 2's pass 1 did not run"
    info["l2"] = stats
    return stream, info
