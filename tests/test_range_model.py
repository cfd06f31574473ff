"""The order-0 range coder model (tests/rangemodel.py, written from K/entropy/RangeEncoder.java and RangeDecoder.java; K/ =
java/src/main/java/io/github/flanglet/kanzi/): round trips, hand-worked vectors, the low-range branch, every decodeHeader
rejection, and the verdicts of the damaged-stream set that tests/test_gpu_range.py runs on the device."""
import os
import re

import pytest

import datagen
import katmodels
import rangecases
import rangemodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bitstring(bits, nbits):
    return format(int.from_bytes(bits, "big"), "0%db" % (8 * len(bits)))[:nbits] if nbits else ""


def test_round_trips():
    for label, d in rangecases.parity_inputs():
        bits, nbits = rangemodel.encode(d)
        assert len(bits) == (nbits + 7) // 8, label
        assert rangemodel.decode(bits, nbits, len(d)) == (len(d), d, nbits), label
    text = datagen.block(3, 20000).tobytes()
    for lr in (8, 9, 15):
        bits, nbits = rangemodel.encode(text, lr=lr)
        assert rangemodel.decode(bits, nbits, len(text)) == (len(text), text, nbits), lr


def test_hand_worked_vectors():
    """(1) b"a" * 100, a chunk that is skipped (RangeEncoder.java:265-269): lr falls to 8 (100 < 256), the header is encodeAlphabet
    -- PARTIAL_ALPHABET '1', lastMask = 97 >> 3 = 12 in 5 bits, 12 empty masks, mask 12 = 1 << (97 & 7) = 0x02 -- then lr - 8 = 0 in 3
    bits; alphabet size 1 writes no frequencies, no payload and no flush: 113 bits.
    (2) b"ab" * 8: lr = 8, both counts 8 scale to 128, cumFreqs a = 0, b = 128.  Header: '1', lastMask 12, masks 0 .. 11 empty, mask 12
    = 0x06, lr - 8 = '000'; one group of 6 (alphabet size < 64) holding only 'b': llr = 4 (1 << 3 <= 8), logMax = 7 ('0111'), freq - 1 =
    127 in 7 bits: 124 bits.  Coding: range starts at 2^60 - 1; step k leaves range = 2^(60 - k) - 128 (range >>> 8 loses the low
    bits, then * 128), and 'b' at the even step k adds 128 * (range >>> 8) = 2^(60 - k) - 128 to low.  After 16 steps range = 2^44 - 128
    is still above 2^32, so the top 28 bits never agreed and no group left; low = 2^58 + 2^56 + ... + 2^44 - 8 * 128 =
    0x5554FFFFFFFFC00, written in 60 bits (:277): its first 28-bit group is 0x5554FFF."""
    bits, nbits = rangemodel.encode(b"a" * 100)
    assert _bitstring(bits, nbits) == "1" + format(12, "05b") + "00000000" * 12 + format(0x02, "08b") + "000"
    assert rangemodel.decode(bits, nbits, 100) == (100, b"a" * 100, 113)
    bits, nbits = rangemodel.encode(b"ab" * 8)
    header = "1" + format(12, "05b") + "00000000" * 12 + format(0x06, "08b") + "000" + "0111" + "1111111"
    low = sum(1 << (60 - 2 * j) for j in range(1, 9)) - 8 * 128
    assert low == 0x5554FFFFFFFFC00 and low >> 32 == 0x5554FFF
    assert len(header) == 124 and _bitstring(bits, nbits) == header + format(low, "060b")
    assert rangemodel.decode(bits, nbits, 16) == (16, b"ab" * 8, 184)


def test_low_range_branch_is_reached():
    """`range = -low & 0xFFFF` (RangeEncoder.java:309) runs in each of the two chunks of rangecases.low_range_input(), in the encoder
    and, mirrored, in the decoder; it does not on the bench's five data classes at 65 836 bytes."""
    data = rangecases.low_range_input()
    bits, nbits = rangemodel.encode(data)
    assert len(rangemodel.low_range_hits) == 2 and all(h >= 1 for h in rangemodel.low_range_hits)
    enc_hits = list(rangemodel.low_range_hits)
    assert rangemodel.decode(bits, nbits, len(data)) == (len(data), data, nbits)
    assert rangemodel.low_range_hits == enc_hits
    for c in range(5):
        rangemodel.encode(datagen.block(c, 65836).tobytes())
        assert sum(rangemodel.low_range_hits) == 0, c


def _stream(alphabet, lr, groups, tail_bits=64):
    """a chunk header written field by field: groups = [(logMax, [freq - 1, ...]), ...]"""
    bs = rangemodel._Bits()
    katmodels._encode_alphabet(bs, alphabet)
    if alphabet:
        bs.write(lr - 8, 3)
        llr = 3
        while (1 << llr) <= lr:
            llr += 1
        for log_max, values in groups:
            bs.write(log_max, llr)
            for v in values:
                bs.write(v, log_max)
    bs.write(0, tail_bits)
    return bs.bytes(), bs.n


def test_every_header_rejection():
    """decodeHeader's three BitStreamExceptions (RangeDecoder.java:192-196, :204-208, :216-221), the empty alphabet (:164-165,
    decode returns the bytes done so far) and a read past the block's bits"""
    for label, (bits, nbits) in (("1 << logMax > scale", _stream([1, 2], 8, [(9, [0])])),
                                 ("freq >= scale", _stream([1, 2], 8, [(8, [255])])),
                                 ("sum >= scale", _stream([1, 2, 3], 8, [(8, [127, 127])]))):
        with pytest.raises(katmodels.JavaException):
            rangemodel.decode(bits, nbits, 10)
    bits, nbits = _stream([1, 2], 8, [(7, [127])])                           # the same shape, accepted: freq 128 / 128
    assert rangemodel.decode(bits, nbits, 10)[0] == 10
    bits, nbits = _stream([], 8, [])
    assert rangemodel.decode(bits, nbits, 10) == (0, bytes(10), 2)
    good, nbits = rangemodel.encode(datagen.block(3, 5000).tobytes())
    with pytest.raises(katmodels.JavaException):
        rangemodel.decode(good, nbits - 28, 5000)


def test_stale_f2s_entries():
    """A chunk at lr 8 after one at lr 15 in the same block: a quotient above 255 reads the first chunk's f2s entries
    (rangecases.unusual_streams asserts the read happened).  A symbol that has frequency 0 in the second chunk makes range 0: the
    normalisation loop never ends and reads to the end of the stream, the block fails.  The undamaged streams decode."""
    cases = {label: (bits, nbits, count, verdict) for label, bits, nbits, count, verdict in rangecases.unusual_streams()}
    for label in ("lr 8", "lr 9", "lr 15", "lr 15 then 8"):
        assert cases[label][3][0] and cases[label][3][2] == cases[label][1], label
    assert not cases["stale symbol absent"][3][0]
    assert "stale symbol present" in cases


def test_damaged_set_has_both_verdicts():
    """the 48 damaged streams of tests/test_gpu_range.py: the model accepts some and rejects some, so the device test cannot pass
    on failures alone"""
    verdicts = [v[0] for _, _, _, _, _, v in rangecases.damaged_trials()]
    assert len(verdicts) == 48 and any(verdicts) and not all(verdicts)


def test_java_adapters_list_range():
    for name in ("HipEntropyEncoder.java", "HipEntropyDecoder.java"):
        src = open(os.path.join(ROOT, "integration", "java", name)).read()
        m = re.search(r"static boolean supports\(int type\) \{([^}]*)\}", src)
        assert m and "type == 4" in m.group(1), name
