"""Blocks for the device TEXT forward of TextCodec1 streams (FPAQ / CM / ANS1; kz_text_fwd_gpu.hip), aimed at the seams at which
TextCodec1 differs from TextCodec2 -- the strict text verdict, the two escape words that hold map slot 0 until the first learn, the
map of blockSize / 8 slots, the byte costs and encodings of the output -- and at the device's granules: rows of 64 bytes, steps of
256, tiles of 1 024 positions.  Deterministic; built from textgen.

cases(bs) -> list of Case for the stream block size bs (32 768: map log 13, 1 MiB: log 17, 4 MiB: log 19).  `device`: the device
form accepts the block and has to finish it (text by the strict rule, no Magic number, 1 024 .. 2^24 - 1 bytes, no wrap of the
word list, output at least 8 bytes short of the input); False: it goes through the host stage or TEXT declines it, `why` says which."""
import random
import re

import textgen

E1, E2 = 0x0F, 0x0E
_H1, _H2 = 0x7FEB352D, 0x846CA68B
SEAMS = (63, 64, 255, 256, 1023, 1024)


class Case:
    """`block` is built when it is first asked for (listing the cases costs nothing)"""

    def __init__(self, name, make, bs, device, why=""):
        self.name, self._make, self.bs, self.device, self.why, self._block = name, make, bs, device, why, None

    @property
    def block(self):
        if self._block is None:
            self._block = bytes(self._make())
        return self._block

    def __repr__(self):
        return "Case(%s, bs %d, device=%s)" % (self.name, self.bs, self.device)


_TEXT = {}


def _english(n, seed, crlf=False):
    """n bytes of English: textgen.english for small blocks, textgen.bulk_text (array operations) from 256 KiB on; kept per call"""
    key = (n, seed, crlf)
    if key not in _TEXT:
        if n < 1 << 18:
            _TEXT[key] = textgen.english(n, seed, crlf=crlf)
        else:
            _TEXT[key] = bytes(textgen.bulk_text(n, (seed << 2) | (3 if crlf else 0), "english"))
    return _TEXT[key]


def _xml(n, seed):
    return textgen.xml(n, seed) if n < 1 << 18 else bytes(textgen.bulk_text(n, seed << 2, "xml"))


def word_hash(w):
    """TextCodec's hash of a word as written (TextCodec.java:709-718; letters: no sign to extend)"""
    h = (_H1 * _H1 ^ w[0] * _H2) & 0xFFFFFFFF
    for c in w[1:]:
        h = ((h * _H1) ^ (c * _H2)) & 0xFFFFFFFF
    return h


def slot0_word(log, seed=7):
    """a lower-case word of 5 .. 8 letters whose hash lands on map slot 0 of a map of 2^log slots"""
    rng = random.Random(seed)
    mask = (1 << log) - 1
    while True:
        w = bytes(rng.randrange(97, 123) for _ in range(rng.randrange(5, 9)))
        if word_hash(w) & mask == 0:
            return w


COLLIDE = (b"tkbjhea", b"aspodtj")                   # in textgen.big_blocks' block of invented words
SLOT0 = {13: b"loqjdk", 17: b"useiyuor"}              # slot0_word(13), slot0_word(17) (test_text1_cases checks both)


def _at(block, positions, values):
    b = bytearray(block)
    for k, p in enumerate(positions):
        b[p] = values[k % len(values)]
    return bytes(b)


def _seam_lines(e):
    """a byte e directly behind a found word and its delimiter, where the implied space between two found words would be, behind a
    delimiter that is no space, and as the byte in front of a found word"""
    e = bytes([e])
    return b"which the " + e + b"and there," + e + b" about the" + e + b"and their would " + e + e + b" there which\n"


def _ascii_edge(n, seed, high):
    """English with exactly `high` bytes >= 0x80 in place of letters, spread over the block"""
    b = bytearray(_english(n, seed))
    step = n // high
    for k in range(high):
        b[k * step + 7] = 0x80 + (k * 37) % 128
    assert sum(1 for c in b if c >= 0x80) == high
    return bytes(b)


def _nuls(n, seed, count):
    b = bytearray(_english(n, seed))
    step = n // count
    for k in range(count):
        b[k * step + 5] = 0
    assert b.count(0) == count
    return bytes(b)


def _big(k):
    if "big" not in _TEXT:
        _TEXT["big"] = textgen.big_blocks(4 << 20)
    return _TEXT["big"][k]


def cases(bs):
    n = bs
    out = []
    add = lambda name, make, device, why="": out.append(Case(name, make, bs, device, why))
    if bs == 4 << 20:
        # 11. the 4 MiB group (textgen.big_blocks): the map has 2^19 slots.  Its block of invented words does NOT wrap the word list at
        #     2^19 under either codec (a word is learned only into an empty slot: test_text1_cases sees the list grow to 2^18 and no
        #     further), and its TextCodec1 output is 2 265 bytes short of the input.  But two of its words, COLLIDE, have the same 32-bit
        #     hash at equal length: the walk takes the second for the first, the size pass's letter check (sameWords) finds out, and the
        #     device leaves the block to the host stage whole.  It is this group's block that is kept and not finished
        names = ("english", "english2", "xml", "utf8", "vocab_150k", "many_words", "english_escapes", "random", "ragged_english")
        dev = ("english", "english2", "xml", "vocab_150k", "english_escapes", "ragged_english")
        why = {"utf8": "not text: TEXT declines (UTF-8)", "random": "not text: TEXT declines",
               "many_words": "two words with one hash and length: the letter check fails the block on the device, host stage"}
        for k, nm in enumerate(names):
            add("big_" + nm, lambda k=k: _big(k), nm in dev, why.get(nm, ""))
        return out
    log = 13 if bs == 32768 else 17
    eng = lambda: _english(n, 105)
    # 1. plain text
    add("english_lf", lambda: _english(n, 101), True)
    add("english_crlf", lambda: _english(n - 1, 102, crlf=True), True)
    add("xml", lambda: _xml(n - 3, 103), True)
    add("capitalised_words", lambda: re.sub(rb"\b[a-z]", lambda m: m.group(0).upper(), _english(n, 104).lower()), True)   # flipped lookups: 0x0E tokens
    # 2. literal 0x0E / 0x0F
    add("esc_at_seams", lambda: _at(eng(), SEAMS, (E2, E1)), True)
    add("esc_at_seams_swapped", lambda: _at(eng(), SEAMS, (E1, E2)), True)
    add("esc1_last_byte", lambda: eng()[:n - 1] + bytes([E1]), True)
    add("esc2_last_byte", lambda: eng()[:n - 70] + bytes([E2]), True)
    add("esc_around_words", lambda: (eng()[:997] + _seam_lines(E1) + _seam_lines(E2)) * 3 + eng()[3000:n // 2], True)
    # 3. bytes >= 0x80
    add("high_at_seams", lambda: _at(eng(), SEAMS + (n - 1,), (0x80, 0xFF, 0xC3, 0xA9)), True)
    add("high_around_words", lambda: (eng()[:997] + _seam_lines(0x80) + _seam_lines(0xFF)) * 3 + eng()[3000:n // 2], True)
    hi = n - 95 * (n // 100)                                                         # nbAscii / 95 == count / 100 with exactly this many
    add("ascii_at_the_edge", lambda: _ascii_edge(n, 106, hi), True)
    add("ascii_past_the_edge", lambda: _ascii_edge(n, 106, hi + 1), False, "not text by the strict rule: TEXT declines")
    # 4. NUL bytes: count / 100 - 1 is text under TextCodec1, count / 100 is not; both are text under TextCodec2
    add("nuls_below_1_percent", lambda: _nuls(n, 107, n // 100 - 1), True)
    add("nuls_at_1_percent", lambda: _nuls(n, 107, n // 100), False, "not text by the strict rule: TEXT declines")
    # 5. no spaces: text under TextCodec1 (no space-frequency rule), not text under TextCodec2
    add("lf_for_spaces", lambda: _english(n, 108).replace(b" ", b"\n"), True)
    # 6. data type tags
    add("pk_magic_english", lambda: b"PK\x03\x04" + _english(n, 109)[:n - 4], False, "Magic number: host stage (tagged BIN, TextCodec1 codes it)")
    add("bm_magic_english", lambda: b"BM" + _english(n, 110)[:n - 2], False, "tagged MULTIMEDIA: TEXT declines before its statistics")
    # 7. the slot-0 seam
    W = SLOT0[log]
    add("slot0_word_first", lambda: (b" " + W) * 6 + b" " + _english(n, 111)[:n - 200], True)
    add("slot0_word_after_a_learn", lambda: b" zzyzxq" + (b" " + W) * 6 + b" " + _english(n, 112)[:n - 200], True)
    if bs == 1 << 20:
        # 8. word numbers pass 128 and 16 384 (one-, two-, three-byte indexes; the three-letter rule switches off); checked in
        #    test_text1_cases: TextCodec1 succeeds with 599 820 bytes, 180 short of the input
        add("many_words", lambda: textgen.many_words(600000, 6), True)
    # 9. the output outgrows the block
    if bs == 32768:
        add("esc_every_12th", lambda: _at(eng(), range(5, n, 12), (E1,)), False, "TEXT fails: the output outgrows the block")
    else:                                                                            # (1 MiB of this text saves more: every 12th still fits)
        add("esc_every_12th", lambda: _at(eng(), range(5, n, 12), (E1,)), True)
        add("esc_every_4th", lambda: _at(eng(), range(5, n, 4), (E1,)), False, "TEXT fails: the output outgrows the block")
    # 10. lengths
    add("len_1023", lambda: textgen.english(1023, 113), False, "under 1 024 bytes: TEXT declines")
    add("len_1024", lambda: textgen.english(1024, 114), True)
    add("len_15", lambda: textgen.english(15, 115), False, "copy block")
    add("spaces_only", lambda: b" " * 3000, False, "not text: TEXT declines")
    return out


def writer_tag(block):
    """the "dataType" entry the writer sets from a block's first bytes, for the two Magic cases here (CompressedOutputStream.java:795-804)"""
    if block[:4] == b"PK\x03\x04":
        return "BIN"
    if block[:2] == b"BM":
        return "MULTIMEDIA"
    return "UNDEFINED"
