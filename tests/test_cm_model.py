"""The CM model (tests/cmmodel.py, written from K/entropy/CMPredictor.java, BinaryEntropyEncoder.java and BinaryEntropyDecoder.java; K/ =
java/src/main/java/io/github/flanglet/kanzi/): round trips, hand-worked vectors, the facts the device code relies on (counters fit
16 bits, predictions stay inside (0, 4096), one flush per bit at most), what the case set of tests/cmcases.py reaches, the verdicts
of the damaged-stream set that tests/test_gpu_cm.py runs on the device, and the public interface as far as it needs no GPU."""
import os
import re

import pytest

import cmcases
import cmmodel
import kanzi_amd as kz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_trips():
    dec = cmcases.decoded()
    for label, (d, bits, nbits, _) in cmcases.encoded().items():
        assert len(bits) * 8 == nbits, label
        (ok, out, used), _ = dec[label]
        assert ok and out == d, label
        assert used == (nbits if d else 0), label               # decode(0 bytes) reads nothing; dispose() wrote the tail all the same
    assert cmcases.encoded()["random0"][1:3] == (bytes([0, 0, 0, 0, 0xFF, 0xFF, 0xFF]), 56)


def test_the_two_codings_of_the_model_agree():
    """encode() carries the predictor inline, for speed; encode_steps() calls the Predictor class the way the Java calls
    CMPredictor.  The greedy adversary is built with the class."""
    enc = cmcases.encoded()
    for label in ("random0", "random1", "random65", "random4097", "runs", "english", "adversary", "first flush in the last byte"):
        d, bits, nbits, _ = enc[label]
        assert cmmodel.encode_steps(d) == (bits, nbits), label


def test_hand_worked_vectors():
    """A fresh predictor (CMPredictor.java:100-124): every counter1 entry is 32768, so p = (13 * 65536 + 6 * 32768) >> 5 = 32768 and
    idx = p >> 12 = 8; counter2[.][8] = 8 << 12 = 32768 and counter2[.][9] = 36864, so
        get() = (2 * 32768 + 3 * (32768 + 36864) + 64) >> 7 = 274496 >> 7 = 2144
    (not 2048: the two interpolation points straddle p from above, 8 << 12 and 9 << 12).  The first three bits of a byte use rows 1, 2
    and 4 (or 3, 5 .. 7), all fresh: pred is 2144 three times.
    Byte 0x20 = 0 0 1 ...: low = 0, high = 2^56 - 1.
      bit 0:  split = (((2^56 - 1) >> 4) * 2144) >> 8 = ((2^52 - 1) * 2144) >> 8 = 2144 * 2^44 - 9   (2144 / 256 = 8.375 is lost)
              low = split + 1 = 2144 * 2^44 - 8
      bit 0:  range = 2^56 - 1 - low = 1952 * 2^44 + 7;  range >> 4 = 1952 * 2^40;  split = 1952 * 2144 * 2^32 = 4185088 * 2^32
              low = 2144 * 2^44 + 4185088 * 2^32 - 7
      bit 1:  range = 2^56 - 1 - low = (1952 * 4096 - 4185088) * 2^32 + 6 = 3810304 * 2^32 + 6;  range >> 4 = 3810304 * 2^28
              split = 3810304 * 2144 * 2^20;  high = low + split
    No flush: the top 32 of the 56 bits still differ.  Byte 0x80 = 1 ...: high = split = 2144 * 2^44 - 9, low = 0.
    The first update with bit 0 (:141-145): counter1[1][256] = 32768 - 8192, counter1[1][0] = 32768 - 2048,
    counter2[1][8] = 32768 - 512, counter2[1][9] = 36864 - 576."""
    tr = []
    cmmodel.encode_steps(b"\x20", tr)
    low1 = 2144 * 2 ** 44 - 8
    low2 = 2144 * 2 ** 44 + 4185088 * 2 ** 32 - 7
    high3 = low2 + 3810304 * 2144 * 2 ** 20
    assert tr[0] == (2144, low1, 2 ** 56 - 1)
    assert tr[1] == (2144, low2, 2 ** 56 - 1)
    assert tr[2] == (2144, low2, high3)
    assert all(((lo ^ hi) & cmmodel.MASK_24_56) != 0 for _, lo, hi in tr[:3])
    tr = []
    cmmodel.encode_steps(b"\x80", tr)
    assert tr[0] == (2144, 0, 2144 * 2 ** 44 - 9)
    pr = cmmodel.Predictor()
    assert pr.get() == 2144
    pr.update(0)
    assert (pr.counter1[1][256], pr.counter1[1][0], pr.counter2[1][8], pr.counter2[1][9], pr.ctx) == (24576, 30720, 32256, 36288, 2)
    # one byte: no flush in 8 bits, so the stream is varint(0) and the tail
    bits, nbits = cmmodel.encode(b"\x80")
    assert nbits == 64 and bits[0] == 0 and bits[5:] == b"\xFF\xFF\xFF"


def test_facts_the_device_code_relies_on():
    """every counter stays in [0, 65535] (the device keeps them as 16-bit words), every prediction in [2, 4095] (split never makes
    low > high; the model asserts that at every bit), and at most one flush or read follows a bit (the device has an `if` where
    the reference has a `while`), in the encoder and in the decoder, on every case"""
    dec = cmcases.decoded()
    for label, (d, _, _, st) in cmcases.encoded().items():
        for s in (st, dec[label][1]):
            assert 0 <= s["cmin"] and s["cmax"] <= 65535, label
            assert s["max_flushes"] <= 1, label
            if d:
                assert 2 <= s["pmin"] and s["pmax"] <= 4095, label
        assert dec[label][1]["overruns"] == 0, label


def test_the_case_set_reaches_the_edges():
    enc, dec = cmcases.encoded(), cmcases.decoded()
    sizes = {len(d) for d, _, _, _ in enc.values()}
    assert set(cmcases.SIZES) <= sizes and (1 << 16) in sizes and max(sizes) == 1 << 16
    assert enc["zeros"][3]["pmin"] == 2 and enc["ones"][3]["pmax"] == 4095
    assert min(st["pmin"] for d, _, _, st in enc.values() if d) == 2 and max(st["pmax"] for d, _, _, st in enc.values() if d) == 4095
    assert max(st["cmax"] for _, _, _, st in enc.values()) == 65535 and min(st["cmin"] for _, _, _, st in enc.values()) == 0
    assert any(d and cmcases.sz_bytes(bits)[0] == 0 for d, bits, _, _ in enc.values())
    # the decoder takes its last payload word while it decodes its last byte
    last = [label for label, (d, bits, _, _) in enc.items()
            if d and dec[label][1]["read_at"] and dec[label][1]["read_at"][-1] == len(d) - 1
            and 4 * len(dec[label][1]["read_at"]) == cmcases.sz_bytes(bits)[0]]
    assert "first flush in the last byte" in last
    d, bits, _, st = enc["first flush in the last byte"]
    assert set(d) == set(b"ab") and st["flush_at"] == [len(d) - 1] and cmcases.sz_bytes(bits) == (4, 1)
    # runs: runMask was on and off
    assert len(set(enc["runs"][0])) > 2
    # the adversary expands, and stays far below the stride the batched calls ask for
    d, bits, _, _ = enc["adversary"]
    assert len(d) < len(bits) < len(d) + (len(d) >> 3)


def test_unusual_streams():
    cases = {label: (bits, nbits, count, want) for label, bits, nbits, count, want in cmcases.unusual_streams()}
    assert [cases[k][3][0] for k in ("long varint", "trailing payload", "szBytes == count << 5", "szBytes == (count << 5) + 1")] == [True, True, True, False]
    for k in ("long varint", "trailing payload", "szBytes == count << 5"):
        assert cases[k][3][2] == cases[k][1], k                   # everything behind the varint counts as read


def test_damaged_set_has_both_verdicts():
    """the 32 damaged streams of tests/test_gpu_cm.py: the model accepts some and rejects some, so the device test cannot pass on
    failures alone.  A cut stream always fails; flipped payload bits decode to other bytes, or fail where the damaged chain asks for
    more words than the payload has."""
    trials = cmcases.damaged_trials()
    verdicts = [v[0] for _, _, _, _, _, v in trials]
    assert len(verdicts) == 32 and any(verdicts) and not all(verdicts)
    by = {}
    for cls, _, _, _, _, v in trials:
        by.setdefault(cls, []).append(v[0])
    assert sorted(by) == ["flipped", "garbage", "shrunken", "truncated"] and all(len(v) == 8 for v in by.values())
    assert not any(by["truncated"]) and any(by["flipped"])
    src = {len(e[0]): e[0] for e in cmcases.encoded().values()}
    for cls, _, _, _, count, v in trials:
        if cls == "flipped" and v[0]:
            assert v[1] != src[count]


def test_blocks_of_64_mib_are_refused():
    class Long(bytes):
        def __len__(self):
            return 1 << 26
    with pytest.raises(ValueError):
        cmmodel.encode(Long())
    with pytest.raises(ValueError):
        cmmodel.decode(b"", 0, 1 << 26)


def test_java_adapters_list_cm():
    for name in ("HipEntropyEncoder.java", "HipEntropyDecoder.java"):
        src = open(os.path.join(ROOT, "integration", "java", name)).read()
        m = re.search(r"static boolean supports\(int type\) \{([^}]*)\}", src)
        assert m and "type == 6" in m.group(1), name


def test_public_names():
    assert kz.ENTROPY_IDS["CM"] == 6 and kz.E_CM == 6
    assert kz.CMEncoder.TYPE == 6 and kz.CMDecoder.TYPE == 6
    with pytest.raises(kz.KanziError) as e:
        kz.level_chain(7)                                       # LZP+TEXT+UTF+BWT+LZP&CM: every stage is built, the order is not
    assert e.value.code == 3 and "in front of TEXT / UTF" in str(e.value) and "LZP" in str(e.value) and "order" in str(e.value)
    for lvl in (4, 8, 9):
        with pytest.raises(kz.KanziError) as e:
            kz.level_chain(lvl)
        assert e.value.code == 3 and "not built here" in str(e.value)
    assert kz.level_chain(6) == ("TEXT+UTF+BWT+SRT+ZRLT", "FPAQ")
