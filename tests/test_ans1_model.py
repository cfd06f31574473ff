"""The order-0 / order-1 range ANS model (tests/ans1model.py) against the reference's order-0 model, a hand-worked order-1 vector and
round trips over the cases where order 1 differs from order 0 (K/ = java/src/main/java/io/github/flanglet/kanzi/)."""
import os
import random
import re

import pytest

import ans1model
import datagen
import katmodels
import refinputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _roundtrip(data, **kw):
    bits, nbits = ans1model.encode(data, 1, **kw)
    r, out, used, clean = ans1model.decode(bits, nbits, len(data), 1, chunk=kw.get("chunk"))
    assert (r, out, used, clean) == (len(data), bytes(data), nbits, True), len(data)
    return bits, nbits


def test_order0_equals_the_ans0_model():
    inputs = refinputs.entropy_inputs() + [datagen.block(c, 20000).tobytes() for c in range(5)]
    for d in inputs:
        enc = ans1model.encode(d, 0)
        assert enc == katmodels.ans0_encode(d)
        assert ans1model.decode(enc[0], enc[1], len(d), 0) == katmodels.ans0_decode(enc[0], enc[1], len(d))


def test_hand_worked_order1_vector():
    """data = b"ab" * 20 (40 bytes: quarter 10, no tail).  Histogram (Global.computeHistogramOrder1 per quarter, each walk starting in
    context 0): ctx 0 = {a: 4} (each quarter's first byte), ctx 'a' = {b: 20}, ctx 'b' = {a: 16}.  Every context is one symbol, so
    normalizeFrequencies gives freq = scale = 2048 (EntropyUtils.java:189-192) and Symbol.reset clamps it to 2047 with cum 0: xMax =
    16 << 16 * 2047 = 2047 << 20, invFreq = ceil(2^42 / 2047) & 0xFFFFFFFF = 0x00200400, invShift = 42, cmplFreq = 1, bias = 0.
    Header: lr - 8 = 3 in 3 bits ('011'); contexts 0, 'a', 'b' each write PARTIAL_ALPHABET '1', lastMask (5 bits) and lastMask + 1
    mask bytes ('a' = 97: lastMask 12, mask 0x02; 'b' = 98: mask 0x04), no frequency chunks (alphabet size 1); the 253 other
    contexts write ALPHABET_0 '01'.  Coding: each state codes its quarter's 10 bytes; from x = 32768 a step is
    x + (x * 0x00200400 >> 42) * 1, i.e. x grows by 16 per step and never reaches xMax, so no byte is emitted: payload size 0 (varint 0x00) and the four final states are equal:
    32768 -> 32784 -> 32800 -> 32816 -> 32832 -> 32848 -> 32864 -> 32880 -> 32896 -> 32912 -> 32928 = 0x000080A0."""
    data = b"ab" * 20
    bits, nbits = ans1model.encode(data, 1)
    ctx0 = "1" + format(12, "05b") + "00000000" * 12 + format(0x02, "08b")
    ctx_a = "1" + format(12, "05b") + "00000000" * 12 + format(0x04, "08b")
    ctx_b = "1" + format(12, "05b") + "00000000" * 12 + format(0x02, "08b")
    want = "011" + ctx0 + "01" * 96 + ctx_a + ctx_b + "01" * (255 - 98) + "00000000" + format(0x80A0, "032b") * 4
    got = format(int.from_bytes(bits, "big"), "0%db" % (8 * len(bits)))[:nbits]
    assert nbits == len(want) and got == want
    assert ans1model.decode(bits, nbits, len(data), 1) == (len(data), data, nbits, True)


def test_order1_round_trips():
    rnd = random.Random(7)
    # 33-40 and 127-129: quarters under and over 32 bytes, len % 4 = 1, 2, 3
    for n in list(range(33, 41)) + [127, 128, 129]:
        _roundtrip(bytes(rnd.randrange(5) for _ in range(n)))
    _roundtrip(b"qu" * 300 + b"q")                                        # one-symbol contexts (after q comes u)
    pairs = bytes(x for i in range(256) for j in range(256) for x in (i, j))  # every one of the 65 536 pairs
    _roundtrip(pairs)
    text = datagen.block(3, 30000).tobytes()
    for lr in (8, 14, 15):
        bits, nbits = _roundtrip(text, lr=lr)
        assert (bits[0] >> 5) == lr - 8
    # several chunks (small chunk size): a tail chunk of 1-3 bytes codes the previous chunk's last byte in context 0
    for tail in (1, 2, 3, 33):
        _roundtrip(bytes(rnd.randrange(3) for _ in range(4096 + tail)), chunk=4096)


def test_tiny_last_chunk_quirk():
    """A last chunk of 1-3 bytes codes block[start - 1] four times in context 0 (encodeChunk :361-389 with quarter 0) with whatever
    Symbol the block left there; a Symbol never reset is all zero and each state then emits two bytes.  The decoder reads the
    tail bytes from the front of the buffer (:436-437), so they come back wrong and n != sz stops the walk -- decode still
    returns count (ANSRangeDecoder.java:217-219)."""
    data = bytes([1, 2] * 2048) + b"\x07"                               # 0x02 ends chunk 0 and never follows a 0 byte
    bits, nbits = ans1model.encode(data, 1, chunk=4096)
    r, out, used, clean = ans1model.decode(bits, nbits, len(data), 1, chunk=4096)
    assert r == len(data) and not clean and out[:4096] == data[:4096] and out[4096:] == b"\x80"


def test_java_adapters_list_ans1():
    for name in ("HipEntropyEncoder.java", "HipEntropyDecoder.java"):
        src = open(os.path.join(ROOT, "integration", "java", name)).read()
        m = re.search(r"static boolean supports\(int type\) \{([^}]*)\}", src)
        assert m and "type == 8" in m.group(1), name
