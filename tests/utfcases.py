"""The deterministic case set of the device UTF forward (kanzi_amd/csrc/kz_utf_fwd_gpu.hip): UTF-8 blocks that TEXT declines with the
"dataType" UTF8, built to sit on the kernel's own boundaries -- alias width (128 symbols), the sort's padding and UF_MAXSYM, the
16-byte thread / 1024-byte wave / 4096-byte tile seams, 256 tiles, UF_MIN_BLOCK, start / adjust, the three decline exits, the
walk-breaking bytes that the byte-pair statistics of TextCodec.detectType (K/transform/TextCodec.java:379-455) do not see, four-unit
code points -- and the batch shapes around them.  No GPU import: tests/test_utf_cases.py checks every case against the oracle and
tests/katmodels.py on the CPU, tests/test_gpu_utf_forward.py runs the batches on the device.

analyse() is a third, small statement of UTFCodec.forward's walk (K/transform/UTFCodec.java:135-219): it names WHICH exit a block
takes and the figures around it, which neither the oracle nor katmodels.utf_forward give away.  expected_class() says what the device
form must do with a block it was given."""
import collections
import functools

import numpy as np

import katmodels
import textgen

Case = collections.namedtuple("Case", "label block bs kind")        # kind: "taken", or the "dataType" TEXT leaves for a block UTF on the device must not see

TILE = 4096
MAXSYM = 16384                                                       # UF_MAXSYM
# ASCII that is neither a letter nor a digit: TEXT must not take these blocks for text, nor for BASE64 / NUMERIC
PUNCT = [ord(c) for c in " .,;:!?-()\n\"'/*[]{}<>|~^_`@#$%&+="]
TWO = list(range(0x400, 0x500)) + list(range(0x100, 0x400)) + list(range(0x500, 0x800))
# the first five: first units E0, ED, EE, EF, whose second unit TextCodec.detectType restricts
THREE = [0x800, 0xFFF, 0xD7FF, 0xE000, 0xFFFD] + list(range(0x4E00, 0xA000)) + list(range(0x3400, 0x4DC0)) + list(range(0xAC00, 0xD7A4))
FOUR = b"\xf0\x9f\x98\x80"                                           # U+1F600
TAIL = b".,;:"
_SIZES = (1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 2, 2, 3, 4)            # UTFCodec.SIZES (:32)


def enc(cps):
    return "".join(map(chr, cps)).encode("utf-8")


def alphabet(ns):
    """ns code points of one, two and three units"""
    n1 = min(20, max(2, ns // 4))
    n2 = min(700, (ns - n1 + 1) // 2)
    return PUNCT[:n1] + TWO[:n2] + THREE[:ns - n1 - n2]


def text(rng, alpha, nbytes, power=3.0):
    """exactly nbytes of whole code points drawn from alpha (skewed use), filled up with '.'"""
    if nbytes <= 0:
        return b""
    a = np.asarray(alpha)
    w = rng.random(len(a)) ** power
    cps = a[rng.choice(len(a), size=nbytes, p=w / w.sum())]
    units = 1 + (cps >= 0x80) + (cps >= 0x800)
    k = int(np.searchsorted(np.cumsum(units), nbytes, side="right"))
    out = enc(cps[:k].tolist())
    return out + b"." * (nbytes - len(out))


def from_counts(alpha, counts, seed):
    """every code point of alpha as often as counts says, shuffled; the four tail bytes behind"""
    idx = np.repeat(np.arange(len(alpha)), counts)
    np.random.default_rng(seed).shuffle(idx)
    a = np.asarray(alpha)
    return enc(a[idx].tolist()) + TAIL


def band(ns, seed):
    """ns distinct code points, each at least once, about 6 ns in all (16 bytes per symbol: the transform applies)"""
    rng = np.random.default_rng(seed)
    m = max(6 * ns, 700)
    w = rng.random(ns) ** 3
    counts = 1 + np.bincount(rng.choice(ns, size=m - ns, p=w / w.sum()), minlength=ns)
    return from_counts(alphabet(ns), counts, seed + 1)


def exits_block(n, ns, asc_pairs, low_units):
    """n bytes, ns symbols: 128 frequent ones (28 ASCII, 100 of two units; at least twice each) and ns - 128 that occur once (of
    low_units units).  The bytes left over are frequent symbols: 2 * asc_pairs ASCII, the rest two-unit -- one ASCII pair more
    instead of one two-unit code point is one alias byte more at the same n and ns."""
    tops1, tops2 = PUNCT[:28], TWO[:100]
    lows = (THREE if low_units == 3 else TWO[100:])[:ns - 128]
    left = n - 4 - (2 * 28 + 2 * 2 * 100 + low_units * len(lows))
    rest = left - 2 * asc_pairs
    assert len(lows) == ns - 128 and rest >= 0, (n, ns, asc_pairs)
    cps = 2 * tops1 + 2 * tops2 + lows + [tops1[i % 28] for i in range(2 * asc_pairs + rest % 2)] + [tops2[i % 100] for i in range(rest // 2)]
    idx = np.arange(len(cps))
    np.random.default_rng(n + ns).shuffle(idx)
    out = enc([cps[i] for i in idx]) + TAIL
    assert len(out) == n
    return out


@functools.lru_cache(maxsize=None)
def analyse(block):
    """UTFCodec.forward's walk and exits on a block whose "dataType" is UTF8 -> dict:
    start, adjust, ns, four (a four-unit code point in the walk), bad (a byte that cannot start a code point, or a three-unit code
    point whose third byte is no continuation byte: what the device form declines on), ref_stop (why the reference's loop breaks:
    "unit", "third", "fourth", "n32768", or None), exit (None: applied; "walk", "map", "estimate", "length"), max_target, estimate,
    outlen, c127 / c128 (the counts of the symbols ranked 127 and 128)."""
    n = len(block)
    assert n >= 1024
    pad = block + bytes(8)
    body = n - 4
    start = 0
    if block[:3] == b"\xef\xbb\xbf":
        start = 3
    else:
        while start < 4 and katmodels._utf_len_seq(block[start]) == 0:
            start += 1
    counts = {}
    four = bad = False
    ref_stop = None
    i = start
    while i < body:
        b0 = pad[i]
        s = _SIZES[b0 >> 4]
        if s == 1:
            key = b0
        elif s == 2:
            key = (1 << 19) | (b0 << 8) | pad[i + 1]
        elif s == 3:
            key = (2 << 19) | ((b0 & 0x0F) << 12) | ((pad[i + 1] & 0x3F) << 6) | (pad[i + 2] & 0x3F)
            if not 0x80 <= pad[i + 2] <= 0xBF:
                bad = True
                ref_stop = ref_stop or "third"
        elif s == 4:
            key = (4 << 19) | ((b0 & 0x07) << 18) | ((pad[i + 1] & 0x3F) << 12) | ((pad[i + 2] & 0x3F) << 6) | (pad[i + 3] & 0x3F)
            four = True
            if (((pad[i + 2] << 8) | pad[i + 3]) & 0xC0C0) != 0x8080:
                ref_stop = ref_stop or "fourth"
        else:
            bad = True
            ref_stop = ref_stop or "unit"
            break
        c = counts.get(key, 0)
        if c == 0 and len(counts) + 1 >= 32768:
            ref_stop = ref_stop or "n32768"
        counts[key] = c + 1
        i += s
    ns = len(counts)
    mt = n - n // 10
    r = dict(start=start, adjust=max(i - body, 0), ns=ns, four=four, bad=bad, ref_stop=ref_stop, max_target=mt, estimate=None, outlen=None,
             c127=None, c128=None, exit=None)
    if ref_stop or ns == 0:
        r["exit"] = "walk"
        return r
    if 3 * ns + 6 >= mt:
        r["exit"] = "map"
        return r
    ranked = sorted(counts.items(), key=lambda kv: (kv[1], kv[0]), reverse=True)
    one = sum(c for _, c in ranked[:128])
    two = sum(c for _, c in ranked[128:])
    if ns > 128:
        r["c127"], r["c128"] = ranked[127][1], ranked[128][1]
    r["estimate"] = 10 + one + 2 * two
    r["outlen"] = 4 + 3 * ns + start + one + 2 * two + 4 - r["adjust"]
    if r["estimate"] >= mt:
        r["exit"] = "estimate"
    elif r["outlen"] >= mt:
        r["exit"] = "length"
    return r


@functools.lru_cache(maxsize=None)
def expected_class(block):
    """what the device UTF forward must do with a block it was given: "finish" (it writes the reference's bytes), "decline" (by the
    reference's rules; the block stays), "host" (left to the host stage: four-unit code points, more than 16384 symbols)"""
    a = analyse(block)
    if a["bad"]:
        return "decline"
    if a["four"] or a["ns"] > MAXSYM:
        return "host"
    # the verdict of the model: analyse()'s exits, which tests/test_utf_cases.py holds against katmodels.utf_forward and the oracle on
    # every case (one walk of a 2 MiB block in Python instead of three)
    return "finish" if a["exit"] is None else "decline"


BAND_NS = (8, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4097, 16383, 16384, 16385, 20000, 32767, 32768)


def _bands():
    small = [Case("band ns=%d" % ns, band(ns, 100 + ns), 0, "taken") for ns in BAND_NS if ns <= 4097]
    big = [Case("band ns=%d" % ns, band(ns, 100 + ns), 0, "taken") for ns in BAND_NS if ns > 4097]
    return small, big


def _order():
    out = []
    a = alphabet(600)
    for k in (1, 3, 8):                                              # k = 1 and 3 decline (map + aliases too long); k = 8 applies: the tie order is in its bytes
        out.append(Case("flat: 600 symbols x %d" % k, from_counts(a, np.full(600, k), 7 + k), 0, "taken"))
    # one, two and three units interleaved in the alphabet's order, all equally frequent: the order goes by the size tags
    mix = [x for t in zip(PUNCT[:30], TWO[:30], THREE[:30]) for x in t] * 2
    mix = mix[:90] + TWO[300:400] + THREE[500:600]
    out.append(Case("flat: mixed sizes, 290 symbols x 7", from_counts(mix, np.full(len(mix), 7), 12), 0, "taken"))
    a = alphabet(300)
    rng = np.random.default_rng(13)
    for nhi in (128, 127, 129):                                      # two count levels; the step at rank 127/128, one before, one behind
        perm = rng.permutation(300)
        counts = np.full(300, 6)
        counts[perm[:nhi]] = 9
        out.append(Case("two levels: %d symbols x 9, the rest x 6" % nhi, from_counts(a, counts, 14 + nhi), 0, "taken"))
    return out


def _around(rng, alpha, at, piece, n):
    """n bytes: text, `piece` from byte `at` on, text, tail"""
    return text(rng, alpha, at) + piece + text(rng, alpha, n - 4 - at - len(piece)) + TAIL


def _seams():
    out = []
    a = alphabet(200)
    c2, c3 = enc([TWO[650]]), enc([THREE[3000]])                     # symbols that occur only on the seam
    rng = np.random.default_rng(21)
    n = 3 * TILE + 37
    for name, piece, bd in (("two units over a thread seam", c2, 77 * 16), ("three units over a thread seam", c3, TILE + 131 * 16),
                            ("three units over the wave seam", c3, TILE + 1024), ("two units over the tile seam", c2, TILE),
                            ("three units over the tile seam", c3, 2 * TILE)):
        for before in range(1, len(piece)):
            out.append(Case("%s, %d before" % (name, before), _around(rng, a, bd - before, piece, n), 0, "taken"))
    return out


def _lengths():
    a = alphabet(200)
    rng = np.random.default_rng(31)
    small = [Case("length %d" % n, text(rng, a, n - 4) + TAIL, 0, "taken") for n in (1024, 1025, 1039, TILE - 1, TILE, TILE + 1, TILE + 4, TILE + 5, 5003)]
    # the last code point begins at n - 5 = 4095: its units lie on both sides of the tile seam and two of them in the tail
    small.append(Case("length 4100, three units from 4095", text(rng, a, TILE - 1) + enc([THREE[9]]) + b".,", 0, "taken"))
    big = [Case("length 1 MiB", text(rng, a, (1 << 20) - 4) + TAIL, 0, "taken"),
           Case("length 1 MiB + 4097", text(rng, a, (1 << 20) + 4097 - 4) + TAIL, 0, "taken"),
           Case("length 2 MiB + 12345, three units", text(rng, PUNCT[:12] + THREE[:400], (2 << 20) + 12345 - 4) + TAIL, 0, "taken")]
    return small, big


def _front_tail():
    a = alphabet(200)
    rng = np.random.default_rng(41)
    n = 3000
    out = [Case("start %d" % s, bytes([0x87, 0xA1, 0xBF, 0x80][:s]) + text(rng, a, n - 4 - s) + TAIL, 0, "taken") for s in range(5)]
    out.append(Case("byte order mark", b"\xef\xbb\xbf" + text(rng, a, n - 7) + TAIL, 0, "taken"))
    out.append(Case("byte order mark, continuation byte", b"\xef\xbb\xbf\x85" + text(rng, a, n - 8) + TAIL, 0, "taken"))
    c2, c3 = enc([TWO[5]]), enc([THREE[40]])
    out.append(Case("adjust 1: two units from n - 5", text(rng, a, n - 5) + c2 + b".,;", 0, "taken"))
    out.append(Case("adjust 1: three units from n - 6", text(rng, a, n - 6) + c3 + b".,;", 0, "taken"))
    out.append(Case("adjust 2: three units from n - 5", text(rng, a, n - 5) + c3 + b".,", 0, "taken"))
    out.append(Case("adjust 3: four units from n - 5", text(rng, a, n - 5) + FOUR + b".", 0, "taken"))
    out.append(Case("third unit in the tail is a letter", text(rng, a, n - 5) + c3[:2] + b"A.,", 0, "taken"))
    return out


# (n, ns, ASCII pairs, units of the rare symbols): worked from exits_block's arithmetic, checked by test_utf_cases.py through analyse()
EXITS = (("map", 1026, 305, 0, 3), ("map", 1026, 306, 0, 3), ("map", 1026, 307, 0, 3),                  # 3 ns + 6 = maxTarget - 3, maxTarget, maxTarget + 3
         ("estimate", 4096, 628, 1102, 2), ("estimate", 4096, 628, 1103, 2), ("estimate", 4096, 628, 1104, 2),   # estimate = maxTarget - 1, maxTarget, + 1
         ("length", 4096, 450, 93, 3), ("length", 4096, 450, 94, 3), ("length", 4096, 450, 96, 3), ("length", 4096, 450, 97, 3))   # length = maxTarget - 1, + 0, + 2, + 3


def _exits():
    return [Case("exit %s: n %d, ns %d, %d ASCII pairs" % (e, n, ns, ap), exits_block(n, ns, ap, lu), 0, "taken") for e, n, ns, ap, lu in EXITS]


def _mutations():
    a = PUNCT[:12] + TWO[:40] + THREE[5:150]
    rng = np.random.default_rng(51)
    n = 3 * TILE + 100
    c3 = enc([THREE[777]])
    taken, other = [], []
    for where, at in (("first tile", 700), ("last tile", n - 300), ("tile seam", TILE)):
        taken.append(Case("continuation byte inserted, " + where, _around(rng, a, at, b"\x9a", n), 0, "taken"))
        # the third unit is missing / a letter: it sits at `at` (the first byte of a tile for the seam)
        taken.append(Case("continuation byte dropped, " + where, _around(rng, a, at - 2, c3[:2], n), 0, "taken"))
        taken.append(Case("third unit a letter, " + where, _around(rng, a, at - 2, c3[:2] + b"A", n), 0, "taken"))
    # what TextCodec.detectType does not let through as UTF8 (:398-404, :427-443): the device UTF forward never sees these blocks
    other.append(Case("two-unit first byte in front of a letter", _around(rng, a, 700, b"\xd0A", n), 0, "UNDEFINED"))
    for name, piece, at in (("C0", b"\xc0\x80", 700), ("C1", b"\xc1\xbf", n - 300), ("F5", b"\xf5\x80\x80\x80", TILE - 2), ("FF", b"\xff", TILE)):
        other.append(Case("first byte " + name, _around(rng, a, at, piece, n), 0, "UNDEFINED"))
    return taken, other


def _four():
    a = PUNCT[:12] + TWO[:40] + THREE[5:150]
    rng = np.random.default_rng(61)
    n = 5 * TILE + 11
    out = [Case("one four-unit code point, " + where, _around(rng, a, at, FOUR, n), 0, "taken")
           for where, at in (("first tile", 1000), ("middle tile", 2 * TILE + 1500), ("last tile", n - 200))]
    broken = enc([THREE[777]])[:2] + b"A"
    out.append(Case("four units, then a broken third unit", text(rng, a, 1000) + FOUR + text(rng, a, 14000) + broken + text(rng, a, n - 4 - 15007) + TAIL, 0, "taken"))
    out.append(Case("a broken third unit, then four units", text(rng, a, 1000) + broken + text(rng, a, 14000) + FOUR + text(rng, a, n - 4 - 15007) + TAIL, 0, "taken"))
    return out


def _many_small():
    rng = np.random.default_rng(71)
    out = []
    for i in range(300):
        n = int(rng.integers(1024, 8193))
        a = alphabet((8, 40, 129, 300)[i % 4])
        front = bytes([0x91, 0xA2][:(i % 7 == 3) + (i % 14 == 3)])
        piece = FOUR if i % 29 == 5 else (b"\xe4\xb8A" if i % 31 == 7 else b"")
        at = int(rng.integers(8, n - 16))
        out.append(Case("small %d" % i, front + _around(rng, a, at, piece, n - len(front)), 0, "taken"))
    return out


def _bs(blocks):
    n = max(len(c.block) for c in blocks)
    bs = 16384
    while bs < n:
        bs <<= 1
    return [c._replace(bs=bs) for c in blocks]


@functools.lru_cache(maxsize=None)
def batches():
    """name -> list of Case; one batch = one kz_encode_blocks call with the block size the cases carry"""
    bands_small, bands_big = _bands()
    lengths_small, lengths_big = _lengths()
    mut_taken, mut_other = _mutations()
    front, four, exits, seams, order = _front_tail(), _four(), _exits(), _seams(), _order()
    rng = np.random.default_rng(81)
    prose = lambda n, seed: Case("English prose", textgen.bulk_text(n, seed).tobytes(), 0, "TEXT")
    others = [Case("binary", bytes(rng.integers(0, 256, 8192, dtype=np.uint8)), 0, "BIN"), Case("15 bytes", enc(THREE[:5]), 0, "UNDEFINED"),
              Case("empty", b"", 0, "UNDEFINED"), Case("1023 bytes of UTF-8", text(rng, alphabet(40), 1023), 0, "UNDEFINED")]
    taken = [bands_small[3], seams[4], mut_taken[2], four[1], front[2], exits[6], mut_taken[0], order[4], lengths_small[7], four[3], front[10]]
    mixed = [prose(40000, 1)]
    for i, c in enumerate(taken):
        mixed.append(c)
        if i < len(others):
            mixed.append(others[i])
    mixed += [mut_other[0], prose(5000, 2), mut_other[3]]
    assert max(len(c.block) for c in taken) < 40000
    longest = Case("length 50001", text(rng, alphabet(300), 50001 - 4) + TAIL, 0, "taken")
    mixed_b = mixed[1:8] + [longest] + mixed[8:] + [prose(40000, 3)]
    b = {"bands small": bands_small, "bands big": bands_big, "order": order, "seams": seams, "lengths small": lengths_small,
         "lengths big": lengths_big, "front and tail": front, "exits": exits, "mutations": mut_taken + mut_other, "four units": four,
         "mixed, longest not taken": mixed, "mixed, longest taken": mixed_b, "many small": _many_small()}
    return {k: _bs(v) for k, v in b.items()}


MIXED = ("mixed, longest not taken", "mixed, longest taken")


@functools.lru_cache(maxsize=None)
def race_batch():
    """48 blocks of 512 KiB (128 tiles each: 6144 workgroups a pass, more than are resident at once), valid UTF-8 with mostly
    three-unit code points and exactly one four-unit code point each: in the first tile for blocks 0, 3, ..., in the middle tile for
    1, 4, ..., in the last for 2, 5, ...  -> (blocks, block size)"""
    n = 512 << 10
    rng = np.random.default_rng(91)
    a = np.asarray(PUNCT[:10] + TWO[:30] + THREE[5:400])
    w = rng.random(len(a)) ** 2
    cps = a[rng.choice(len(a), size=n, p=w / w.sum())]
    units = 1 + (cps >= 0x80) + (cps >= 0x800)
    k = int(np.searchsorted(np.cumsum(units), n - 8, side="right"))
    cps = np.concatenate([cps[:k], np.full(n - 8 - int(units[:k].sum()), 0x2E)])      # n - 8 bytes: the four units and the tail come on top
    blocks = []
    for i in range(48):
        c = np.roll(cps, 997 * i)
        cum = np.cumsum(1 + (c >= 0x80) + (c >= 0x800))
        at = int(np.searchsorted(cum, (2000, n // 2 + 100, n - 2000)[i % 3]))
        blocks.append(enc(c[:at].tolist()) + FOUR + enc(c[at:].tolist()) + TAIL)
        assert len(blocks[-1]) == n
    return blocks, n
