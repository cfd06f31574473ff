"""Inputs and expected results shared by tests/test_cm_model.py (no GPU) and tests/test_gpu_cm.py: the single-block inputs with the
model's streams and statistics, streams the encoder never writes, and the damaged-stream set with the model's verdicts.  Every block
is at most 64 KiB (the model codes about 25 000 bytes a second); everything expensive is computed once per process."""
import functools

import numpy as np

import cmmodel
import textgen

SIZES = (0, 1, 2, 15, 16, 63, 64, 65, 4095, 4096, 4097)


def runs_input(n, seed):
    """runs of 200-900 equal bytes, each ended by a random byte: runMask switches on and off, counter2[.][16] is in use"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([int(rng.integers(0, 256))]) * int(rng.integers(200, 901))
        out.append(int(rng.integers(0, 256)))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def first_flush_in_last_byte():
    """a two-symbol input cut behind the byte in which the encoder flushes for the first time: szBytes is 4 and the decoder reads
    that word while it decodes the last byte"""
    rng = np.random.default_rng(21)
    seq = bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), 256))
    cmmodel.encode(seq)
    return seq[:cmmodel.stats["flush_at"][0] + 1]


@functools.lru_cache(maxsize=None)
def inputs():
    """[(label, bytes)]"""
    rng = np.random.default_rng(6)
    out = [("random%d" % n, bytes(rng.integers(0, 256, n, dtype=np.uint8))) for n in SIZES]
    out.append(("random64k", bytes(rng.integers(0, 256, 1 << 16, dtype=np.uint8))))
    out.append(("zeros", bytes(4097)))
    out.append(("ones", b"\xFF" * 4097))
    out.append(("alternating", b"\x00\xFF" * 2048))
    out.append(("runs", runs_input(12001, 7)))
    out.append(("english", textgen.english(8191, 3)[:8191]))
    out.append(("adversary", cmmodel.greedy_adversary(2048)))
    out.append(("first flush in the last byte", first_flush_in_last_byte()))
    return out


@functools.lru_cache(maxsize=None)
def encoded():
    """{label: (data, bits, nbits, stats of the model's encode)}"""
    res = {}
    for label, d in inputs():
        d = bytes(d)
        bits, nbits = cmmodel.encode(d)
        st = dict(cmmodel.stats)
        st["flush_at"] = list(st["flush_at"])
        res[label] = (d, bits, nbits, st)
    return res


@functools.lru_cache(maxsize=None)
def decoded():
    """{label: ((ok, bytes, bits consumed), stats of the model's decode)} of the model's own streams"""
    res = {}
    for label, (d, bits, nbits, _) in encoded().items():
        r = cmmodel.decode(bits, nbits, len(d))
        st = dict(cmmodel.stats)
        st["read_at"] = list(st["read_at"])
        res[label] = (r, st)
    return res


def sz_bytes(bits):
    """(szBytes, length of the varint) of a block stream"""
    v, sz, shift, n = bits[0], bits[0] & 0x7F, 7, 1
    while v >= 128:
        v = bits[n]
        n += 1
        sz |= (v & 0x7F) << shift
        shift += 7
    return sz, n


@functools.lru_cache(maxsize=None)
def unusual_streams():
    """[(label, bits, nbits, count, the model's (ok, bytes, bits consumed))]: streams that decode (or must not) though the encoder
    never writes them"""
    enc = encoded()
    out = []

    def add(label, bits, count):
        out.append((label, bits, 8 * len(bits), count, cmmodel.decode(bits, 8 * len(bits), count)))

    d, bits, _, _ = enc["english"]
    sz, vl = sz_bytes(bits)
    assert vl == 2
    body = bits[vl:]
    add("long varint", bytes([0x80 | (sz & 0x7F), 0x80 | (sz >> 7), 0x80, 0x00]) + body, len(d))
    add("trailing payload", cmmodel.varint(sz + 8) + body + bytes(range(1, 9)), len(d))
    d1, bits1, _, _ = enc["random1"]
    assert sz_bytes(bits1) == (0, 1)
    junk = bytes(np.random.default_rng(9).integers(0, 256, 40, dtype=np.uint8))
    add("szBytes == count << 5", cmmodel.varint(32) + bits1[1:] + junk[:32], 1)
    add("szBytes == (count << 5) + 1", cmmodel.varint(33) + bits1[1:] + junk[:33], 1)
    assert [o[4][0] for o in out] == [True, True, True, False]
    assert out[0][4][1] == d and out[1][4][1] == d and out[2][4][1] == d1
    assert out[1][4][2] == 8 * (vl + 7 + sz + 8)
    return out


@functools.lru_cache(maxsize=None)
def damaged_trials():
    """[(class, trial, bits, nbits, count, the model's (ok, bytes, bits consumed))], 8 seeded trials of each of four classes.  CM
    has no check of its own: a flipped payload bit decodes to other bytes, or fails where the damaged chain asks for more words than
    the payload has; a shrunken szBytes fails only if the decoder wants the missing words before the block is done."""
    enc = encoded()
    rng = np.random.default_rng(33)
    sources = [enc[k] for k in ("random4096", "english", "runs", "random65")]
    out = []
    for t in range(8):
        d, bits, nbits, _ = sources[t % 4]
        sz, vl = sz_bytes(bits)
        cut = nbits - int(rng.integers(1, 8 * sz + 56))
        out.append(("truncated", t, bits, cut, len(d), cmmodel.decode(bits, cut, len(d))))
        small = max(0, sz - 4 * int(rng.integers(1, 4))) if t < 6 else 0
        sv = cmmodel.varint(small)
        sv = sv if len(sv) == vl else bytes([0x80 | sv[0], 0x00])           # the same layout: only the count changes
        shr = sv + bits[vl:]
        out.append(("shrunken", t, shr, nbits, len(d), cmmodel.decode(shr, nbits, len(d))))
        fl = bytearray(bits)
        for _ in range(1 + t % 3):
            at = int(rng.integers(8 * vl, 8 * (vl + sz)))
            fl[at >> 3] ^= 0x80 >> (at & 7)
        fl = bytes(fl)
        out.append(("flipped", t, fl, nbits, len(d), cmmodel.decode(fl, nbits, len(d))))
        g = bytearray(rng.integers(0, 256, 600, dtype=np.uint8))
        if t & 1:                                                            # a header that passes, garbage behind it
            g[0:2] = cmmodel.varint(400)
        g = bytes(g)
        out.append(("garbage", t, g, 8 * len(g), 100, cmmodel.decode(g, 8 * len(g), 100)))
    return out
