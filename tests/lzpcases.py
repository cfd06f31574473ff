"""Inputs shared by tests/test_lzp_model.py (no GPU) and tests/test_gpu_lzp.py: the hand-worked vectors, the 67 / 66 band pair,
the hash collision pair, the damaged inputs and the fuzz generator.  Nothing here calls the device; expected bytes that are not
worked out by hand come from tests/lzpmodel.py.  Everything expensive is computed once per process."""
import functools

import numpy as np

import lzpmodel

FC, FE, FF = b"\xfc", b"\xfe", b"\xff"
# two contexts with the same table slot: (0x7FEB352D * ctx mod 2^32) >> 16 == 58 795 for both
COLLIDING = (0xFDB17F54, 0x0B8A276B)
COLLIDING_SLOT = 58795


def noise(n, seed, exclude=(0xFC,)):
    """n random bytes without the values in `exclude` (no 0xFC: nothing is escaped unless a test plants it)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256 - len(exclude), n, dtype=np.uint8).astype(np.int32)
    for v in sorted(exclude):
        a[a >= v] += 1
    return a.astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def unit300():
    return noise(300, 300)


@functools.lru_cache(maxsize=None)
def hand_vectors():
    """[(label, input, expected output)]; the expected bytes are derived by hand in test_lzp_model.py's docstrings"""
    u = unit300() * 30
    return [
        ("zeros", bytes(5000), bytes(5) + FC + FE * 19 + b"\x66" + bytes(3)),
        ("flags", FC * 5000, FC * 5 + FC + FE * 19 + b"\x66" + (FC + FF) * 3),
        ("abc", b"abc" * 2000, b"abcabcabca" + FC + FE * 23 + b"\x4e" + b"abcabc"),
        ("unit300", u, u[:308] + FC + FE * 33 + b"\xf2" + u[8996:]),
    ]


def planted(n, seed, at, ref, length, before=b"", cut=True):
    """noise of n bytes in which the `length` bytes at `ref` (and the four in front of them) are repeated at `at`; `before`
    replaces the bytes just in front of the four context bytes at `at`; with `cut` the byte behind the copy differs from the one behind
    the original, so that the match is exactly `length` bytes long"""
    d = bytearray(noise(n, seed))
    d[at - 4:at + length] = d[ref - 4:ref + length]
    if d[at - 5] == d[ref - 5]:                                  # the contexts one position earlier must differ
        d[at - 5] = (d[ref - 5] + 1) % 0xFC
    if before:
        d[at - 4 - len(before):at - 4] = before
    if cut and at + length < n:
        d[at + length] = (d[ref + length] + 1) % 0xFC
    return bytes(d)


def band_pair():
    """4 096 bytes free of 0xFC with one repeat of 67 / 66 bytes behind equal contexts: the match saves length - 2 bytes, dstEnd is
    4 096 - 64 = 4 032, and the verdict asks for dstIdx < dstEnd"""
    return planted(4096, 67, 2004, 104, 67), planted(4096, 67, 2004, 104, 66)


def collision_block(foreign=True):
    """1 024 bytes of noise with one 120-byte match: the four bytes of COLLIDING[0] at 100 (its slot is written at position 104), the four bytes of
    COLLIDING[1] at 300 and 0xFC at 304.  The 0xFC is escaped only because a FOREIGN context left an entry in the slot; without it
    (`foreign=False`: the bytes at 100 stay noise) the slot is empty and the 0xFC goes out alone."""
    d = bytearray(planted(1024, 9, 800, 600, 120))              # one match, so that the block applies
    if foreign:
        d[100:104] = COLLIDING[0].to_bytes(4, "big")
    d[300:304] = COLLIDING[1].to_bytes(4, "big")
    d[304] = 0xFC
    return bytes(d)


@functools.lru_cache(maxsize=None)
def short_coded_block():
    """(data, coded): 1 600 bytes with a 200-byte match, a 500-byte match (one 0xFE) and 0xFC literals: short enough to cut at
    every offset"""
    d = bytearray(noise(1600, 21))
    d[60] = 0xFC
    d[400 - 4:400 + 200] = d[100 - 4:100 + 200]
    d[700] = 0xFC
    d[1060 - 4:1060 + 500] = d[540 - 4:540 + 500]                # 64 + 254 + 182: one 0xFE
    d[1584 - 4:1584] = d[60 - 4:60]                              # the context of position 60 again: this 0xFC finds an entry, is escaped
    d[1584] = 0xFC
    data = bytes(d)
    ok, coded = lzpmodel.forward(data)
    assert ok
    return data, coded


@functools.lru_cache(maxsize=None)
def damaged_inputs():
    """[(label, coded bytes, dst_len)] for the inverse: every truncation of the short block, a 0xFE chain to the end, a 0xFC as the
    last byte, dst_len one short, counts 0 to 4"""
    data, coded = short_coded_block()
    out = [("cut%d" % k, coded[:k], len(data)) for k in range(len(coded) + 1)]
    p = coded.index(FC + FE)                                     # the chained match
    out.append(("fe_to_end", coded[:p + 1] + FE * 40, 1 << 16))
    out.append(("fe_to_end_long", coded[:p + 1] + FE * 200, 1 << 16))
    out.append(("flag_last", coded[:p + 1], len(data)))
    out.append(("one_short", coded, len(data) - 1))
    out.append(("exact", coded, len(data)))
    out.append(("roomy", coded, len(data) + 1000))
    out.append(("dst_below_count", coded, len(coded) - 1))
    for n in range(5):
        out.append(("count%d" % n, bytes(range(1, n + 1)), 16))
    out.append(("count4_flags", FC * 4, 4))
    out.append(("count5_flag", b"abcd" + FC, 16))
    return out


def fuzz_block(seed, n=24576):
    """A block that reaches every branch: a stretch of full-alphabet noise fills about a third of the table (so that the mixed
    contexts right behind a match find an entry about as often as not), then stretches over a small alphabet with 0xFC in it, with
    repeats of 64 to 900 bytes planted from earlier data, some of them overlapping their own source (short distances), each
    followed by 0xFC bytes."""
    rng = np.random.default_rng(seed)
    d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    alpha = np.array([0x41, 0x42, 0xFC, 0x43, 0x00, 0xFF, 0xFE], dtype=np.uint8)
    pos = n // 2
    small = alpha[rng.integers(0, len(alpha), n - pos)]
    d[pos:] = small.tobytes()
    p = 2000
    while p < n - 1200:
        length = int(rng.choice([64, 65, 70, 100, 317, 318, 400, 900]))
        dist = int(rng.choice([1, 2, 3, 7, 63, 64, 65, 500, 1500]))
        dist = min(dist, p - 8)
        for i in range(length + 4):                              # byte by byte: a short distance makes the data periodic
            d[p - 4 + i] = d[p - 4 + i - dist]
        q = p + length
        d[q] = (d[q - dist] + 1) & 0xFF                         # cut
        k = int(rng.integers(0, 4))
        d[q + k] = 0xFC                                          # an 0xFC at one of the first positions behind the match (if it is coded)
        p = q + int(rng.integers(20, 400))
    return bytes(d)


# ---- inputs built for the seams of the device parse (windows of W positions, the first one starts at position 4) --------------------
_EARLY = {5: b"AAAAA", 6: b"AAABAA", 7: b"AABAAAA", 8: b"ABAAAAAA"}


def match_at(at, n=1024):
    """a block whose first match starts at position `at` (5 .. n - 200) with only literals in front of it.  Position 4 cannot match:
    it is the first one visited and finds an empty table.  5 to 8: a run of one byte behind a prefix chosen so that the mixed-order
    contexts of positions 4.. differ until `at`.  From 9 on: the block is periodic from position 4 with period at - 8, so that
    position `at` repeats the context of position 8."""
    if at in _EARLY:
        d = bytearray(_EARLY[at])
        d += bytes([d[-1]]) * (300 - len(d))
        return bytes(d) + noise(n - 300, at)
    p = at - 8
    for seed in range(at, at + 4000, 1000):                      # (a chance hit on the slot of position 8 moves the match: next seed)
        d = bytearray(noise(n, seed))
        if d[at - 5] == d[0]:                                    # position at - 1 must not repeat the mixed context of position 7
            d[at - 5] = (d[0] + 1) % 0xFC
        for i in range(at - 4, at + 100):
            d[i] = d[i - p]
        d[at + 100] = (d[at + 100 - p] + 1) % 0xFC
        ok, out = lzpmodel.forward(bytes(d))
        if ok and out[:at] == d[:at] and out[at] == 0xFC:
            return bytes(d)
    raise AssertionError(at)


def late_match(off, flags=0, n=2048):
    """noise with the 80 bytes at 1000 repeated at 1100 + off: the windows in front of it start at 4 + 64 k, so off = 0 .. 2 W - 1
    puts the match on every lane twice.  `flags` 0xFC bytes stand right in front of its four context bytes."""
    return planted(n, 1000 + off, 1100 + off, 1000, 80, before=FC * flags)


def broken_runs(with_tail=True):
    """runs of 8 to 63 equal bytes, every second one of 0xFC: every lane of a window has the hash of its neighbour, the entries come
    from inside the window, and no run is long enough to match.  The zeros behind them are one long match that lets the block apply."""
    d = bytearray()
    for k, length in enumerate(range(8, 64)):
        d += bytes([0xFC if k % 2 else 0x30 + k]) * length
    return bytes(d) + (bytes(3000) if with_tail else b"")


def periodic(p, n=3000, flag=False):
    u = bytearray(noise(p, 40 + p))
    if flag:
        u[p // 2] = 0xFC
    return (bytes(u) * (n // p + 1))[:n]


def match_to_end(k, n=1000):
    """a match from position 600 (source at 100) that ends k bytes before the block's end"""
    return planted(n, 50 + k, 600, 100, n - 600 - k)


def dst_end_cases():
    """[(label, data)]: blocks that decline because dstIdx reaches dstEnd (a) at a literal, (b) at the 0xFF of an escape, (c) inside a
    chain of 0xFE.  (b): a 66-byte match leaves dstIdx = srcIdx - 64, the last byte is an 0xFC behind the context of position 60.
    (c): 104 runs of forty 0xFC (escaped from the sixth on, no match: under 64 bytes) push dstIdx ahead of srcIdx, then a run of zeros
    to the end is coded with fourteen 0xFE of which the last ones do not fit."""
    a = planted(4096, 67, 2004, 104, 66)
    b = bytearray(planted(4096, 31, 2004, 104, 66))
    b[4091:4095] = b[56:60]
    b[4095] = 0xFC
    c = bytearray()
    for i in range(104):
        c += FC * 40 + bytes([i])
    c += noise(34, 5)
    c += bytes(8192 - len(c))
    return [("literal", a), ("escape", bytes(b)), ("chain", bytes(c))]
