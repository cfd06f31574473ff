"""The comparisons of tests/test_gpu_layout.py bite: each is fed, without a GPU, a result that a subtly wrong library would give
-- one that depends on the filled slot behind the stream, a neighbour's block, a frame with one clobbered guard byte -- and must
fire; and the accepted / rejected mix of the damaged streams is what that module asserts on the GPU."""
import types

import numpy as np
import pytest

import datagen
import oracle
import layouthelp as lh
from layouthelp import FILLS, Frame


def test_frame_places_rows_and_keeps_the_fill():
    for fill in FILLS + ("a5",):
        f = Frame(1000, fill, guard=256)
        f.put(3, b"abc")
        f.put_stream(100, bytes([0xF0, 0xFF]), 13)                 # 13 bits: the last three bits of byte 1 stay the fill's
        p = f.ptr(0)
        assert p == f.img.ctypes.data + 256
        a = f.after()
        assert bytes(a[256 + 3:256 + 6]) == b"abc" and a[256 + 100] == 0xF0
        assert a[256 + 101] == (0xF8 | (int(f.fill[256 + 101]) & 7))
        assert a[256 + 102] == f.fill[256 + 102]
        assert f.guards_intact() and f.untouched()
        assert [bytes(r) for r in f.rows(3, 97, 2, 3)][0] == b"abc"
    with pytest.raises(AssertionError):
        Frame(10, "zero", guard=16).put(8, b"abc")                 # rows never reach into a guard by accident


@pytest.mark.parametrize("where", [0, 255, 256 + 1000, 256 + 1000 + 255])
def test_one_clobbered_guard_byte_is_seen(where):
    for fill in FILLS:
        f = Frame(1000, fill, guard=256)
        f.ptr(0)
        f.img[where] ^= 0x40
        assert not f.guards_intact() and not f.untouched()
        with pytest.raises(AssertionError):
            lh.assert_guards(f, "clobbered")
    f = Frame(1000, "rand", guard=256)
    f.ptr(0)
    f.img[256 + 500] ^= 1                                          # inside the payload: the guards are fine, the frame is not untouched
    assert f.guards_intact() and not f.untouched()


def test_decode_comparison_fires_on_a_result_taken_from_the_filled_slot():
    """a decoder that lets the slot behind bit W count: the oracle run on the FILLED slot, with the bits the fill adds"""
    data = datagen.block(1, 2000).tobytes()
    fired = 0
    for ent in ("NONE", "ANS0", "HUFFMAN", "FPAQ"):
        s, w = oracle.entropy_encode(ent, data)
        nb = w - 16                                                # a cut stream: the reference rejects it
        r, o, used = oracle.entropy_decode(ent, s[:(nb + 7) // 8], nb, len(data))
        assert r != len(data)
        for fill in ("ones", "rand"):
            f = Frame((nb + 7) // 8 + 64, fill, guard=64)
            f.put_stream(0, s, nb)
            slot = bytes(f.rows(0, 0, 1, (nb + 7) // 8 + 64)[0])
            r2, o2, used2 = oracle.entropy_decode(ent, slot, nb + 64 * 8, len(data))      # reads on into the fill
            if r2 == len(data):                                    # the wrong decoder accepts what the reference rejects
                with pytest.raises(AssertionError):
                    lh.check_entropy_decoded((ent, fill), r2, o2, used2, len(data), r, o, used)
                fired += 1
    assert fired >= 2
    # block level: whole stream, the last byte's spare bits and the byte before it taken from the fill
    blk = datagen.block(0, 20000).tobytes()
    s, w, _, _ = oracle.encode_block("LZ", "HUFFMAN", blk, block_size=65536)
    r, o = oracle.decode_block("LZ", "HUFFMAN", 65536, s, w, 65536)
    assert r == len(blk)
    f = Frame(len(s), "ones", guard=64)
    f.put_stream(0, s[:-2], 8 * (len(s) - 2))                      # the fill leaks into the stream's last 16 bits
    r2, o2 = oracle.decode_block("LZ", "HUFFMAN", 65536, bytes(f.rows(0, 0, 1, len(s))[0]), w, 65536)
    assert (r2, o2) != (r, o)
    with pytest.raises(AssertionError):
        lh.check_decoded("leak", 0 if r2 >= 0 else r2, max(r2, 0), np.frombuffer(o2 + bytes(len(blk)), dtype=np.uint8), r, o)
    with pytest.raises(AssertionError):                            # a failed block must not report a length
        lh.check_decoded("length", -13, 5, np.zeros(5, dtype=np.uint8), -13, b"")
    assert lh.check_decoded("fine", 0, r, np.frombuffer(o, dtype=np.uint8), r, o)
    assert not lh.check_decoded("fine", -19, 0, np.zeros(1, dtype=np.uint8), -19, b"")


def _res(ref, **k):
    d = dict(status=0, bits=ref[1], length=ref[3], skipFlags=ref[2], mode=ref[0][0] if ref[1] else 0)
    d.update(k)
    return types.SimpleNamespace(**d)


def test_encode_comparison_fires_on_a_neighbours_block():
    blocks = [datagen.block(c, 5000 + c).tobytes() for c in range(3)]
    refs = [oracle.encode_block("BWT+RANK+ZRLT", "ANS0", b) for b in blocks]
    row = lambda r: np.frombuffer(r[0] + bytes(64), dtype=np.uint8)
    lh.check_stream("own", _res(refs[1]), row(refs[1]), refs[1])
    for other in (0, 2):                                           # the stream, or only the result, of the block next door
        with pytest.raises(AssertionError):
            lh.check_stream("neighbour", _res(refs[other]), row(refs[other]), refs[1])
        with pytest.raises(AssertionError):
            lh.check_stream("neighbour's bytes", _res(refs[1]), row(refs[other]), refs[1])
    for k in (dict(bits=refs[1][1] + 1), dict(length=refs[1][3] - 1), dict(skipFlags=refs[1][2] ^ 0x20), dict(mode=refs[1][0][0] ^ 1), dict(status=-13)):
        with pytest.raises(AssertionError):
            lh.check_stream("field", _res(refs[1], **k), row(refs[1]), refs[1])
    bad = row(refs[1]).copy()
    bad[len(refs[1][0]) - 1] ^= 0x80                               # one bit of the last stream byte
    with pytest.raises(AssertionError):
        lh.check_stream("last byte", _res(refs[1]), bad, refs[1])


def test_damaged_streams_are_accepted_and_rejected_often_enough():
    """the cap on the GPU module's case mix, settled on the CPU: per coder >= 10 damaged block streams the oracle accepts and >= 30
    it rejects; the same for the cut and mildly damaged entropy streams"""
    import test_gpu_layout as t
    tally = {}
    for chain, ent in t.COMBOS:
        a, r = tally.get(ent, (0, 0))
        for c in t.decode_cases(chain, ent):
            if c[3]:
                a += c[4] >= 0
                r += c[4] < 0
        tally[ent] = (a, r)
    for ent, (a, r) in tally.items():
        assert a >= 10 and r >= 30, (ent, a, r)
    for ent in ("ANS0", "HUFFMAN", "FPAQ", "NONE"):
        cs = t.entropy_cases(ent)
        a = sum(1 for c in cs if c[4] == c[3])
        assert a >= 10 and len(cs) - a >= 30, (ent, a, len(cs) - a)
