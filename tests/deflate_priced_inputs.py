"""The inputs that the tests of level 2's priced passes share (test_deflate_model_priced.py on the CPU,
test_gpu_deflate_priced.py on the GPU): one planted input per branch of the priced cost rule
(deflate_model_priced.py's counters and `without` names).

gained          two-letter filler, so lit16 is 18 and the flat rule wants 10 bytes and more, with a phrase of eight
                rare bytes repeated: eight of them cost some 70 bits as literals, and the priced pass takes the match.
dropped         1024 random bytes, then 2048 of two letters in which nothing repeats for 11 bytes: the tile's average
                lit16 (some 3 bits a byte) lets the flat rule take matches of 5 to 8 in the two-letter part, whose
                literals cost a bit or two each; the priced pass refuses a hundred of them.
uncoded_dist    a two-letter de Bruijn sequence, where nothing repeats for 10 bytes, with a phrase of eight rare
                bytes twice: pass 1 finds no match at all, the distance code holds only its two dummy symbols and
                there is no length symbol, so pass 2 prices every match with 15 twice -- and still takes the phrase.
uncoded_literal (history shape) a byte value that occurs in the history and, in the tile, only as the first byte of a
                phrase that pass 1 takes as a match from the history: it has no codeword, and pass 2 prices it at 15.

Each is (history, data); the history is empty but for the last."""
from functools import lru_cache

import numpy as np

RARE = bytes(range(200, 208))                       # the phrase of eight rare bytes


def two_letters(rng, n):
    return np.frombuffer(b"xy", np.uint8)[rng.integers(0, 2, n)].tobytes()


def de_bruijn(k):
    """The binary de Bruijn sequence B(2, k) in the letters x and y: 2 ** k bytes, every k of them (cyclically)
    once, so no two positions agree for k bytes."""
    a, seq = [0] * (2 * k), []

    def db(t, p):
        if t > k:
            if k % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 2):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return bytes(b"xy"[s] for s in seq)


def gained(seed=21):
    rng = np.random.default_rng(seed)
    a = bytearray(two_letters(rng, 4096 + 33))
    for at in (300, 900, 1700, 2500, 3300, 4000):
        a[at:at + 8] = RARE
    return b"", bytes(a)


def dropped(seed=22):
    rng = np.random.default_rng(seed)
    return b"", bytes(rng.integers(0, 256, 1024, dtype=np.uint8)) + de_bruijn(11) + b"xyxxy"


def uncoded_dist():
    a = bytearray(de_bruijn(10))
    for at in (200, 700):                           # (the bytes around the two differ: the match is the eight)
        a[at - 1:at + 9] = (b"x" if at == 200 else b"y") + RARE + (b"x" if at == 200 else b"y")
    return b"", bytes(a)


def uncoded_literal(seed=24):
    rng = np.random.default_rng(seed)
    phrase = b"\xf0" + two_letters(rng, 13)
    history = bytearray(de_bruijn(10))
    history[1000:1000 + len(phrase)] = phrase
    data = bytearray(de_bruijn(10)[::-1])
    data[40:40 + len(phrase)] = phrase
    return bytes(history), bytes(data)


PLANTED = {"gained": gained, "dropped": dropped, "uncoded_dist": uncoded_dist, "uncoded_literal": uncoded_literal}
# the counter of info["priced"] each is there for, and the `without` switch that changes its bytes
BRANCH = {"gained": ("gained", "rezero"), "dropped": ("dropped", "strict"), "uncoded_dist": ("uncoded", "price15"),
          "uncoded_literal": ("uncoded", "price15")}


@lru_cache(maxsize=None)
def planted(name):
    return PLANTED[name]()
