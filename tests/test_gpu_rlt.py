"""RLT on the device against tests/rltmodel.py (a restatement of K/transform/RLT.java): single blocks, seams of the tile-parallel
kernels, the context's data type, the array-length band, damaged input, chains through the batched calls and the stream calls.
Every expected byte comes from the CPU models, never from the device."""
import os
import re

import numpy as np
import pytest
import torch

import datagen
import katmodels
import kanzi_amd as kz
import oracle
import refinputs
import rltmodel
import textgen
from test_rlt_model import band_example

pytestmark = pytest.mark.gpu

DT_NAME = {v: k for k, v in kz.DATA_TYPES.items()}
TILE = 4096                                   # bytes per workgroup of the forward and the inverse kernels (kz_rlt.hip)
PIECE = rltmodel.MAX_RUN4                     # 73 469


@pytest.fixture(scope="module")
def ctx():
    return kz.Context(0)


def dev_forward(ctx, data, dst_len, entropy="NONE", data_type="UNDEFINED"):
    ctx.set_data_type(data_type)
    t = kz.RLT(ctx, entropy)
    src = kz.SliceByteArray(np.frombuffer(data, dtype=np.uint8).copy())
    dst = kz.SliceByteArray(np.zeros(dst_len, dtype=np.uint8))
    ok = t.forward(src, dst)
    return ok, dst.array[:dst.index].tobytes(), DT_NAME[ctx.get_data_type()]


def dev_inverse(ctx, data, dst_len):
    t = kz.RLT(ctx)
    src = kz.SliceByteArray(np.frombuffer(data, dtype=np.uint8).copy())
    dst = kz.SliceByteArray(np.zeros(dst_len, dtype=np.uint8))
    ok = t.inverse(src, dst)
    return ok, dst.array[:dst.index].tobytes()


def model_inverse(data, dst_len):
    """(ok, bytes); an exception of the reference fails the block (a one-byte input reads src[1]: the device answers "failed")"""
    try:
        return rltmodel.inverse(data, dst_len)
    except katmodels.JavaException:
        return False, b""


def check_forward(ctx, data, dst_len=None, entropy="NONE", data_type="UNDEFINED", tag=None):
    data = bytes(data)
    dst_len = rltmodel.max_encoded_length(len(data)) if dst_len is None else dst_len
    want = rltmodel.forward(data, dst_len, entropy, data_type)
    got = dev_forward(ctx, data, dst_len, entropy, data_type)
    assert got[0] == want[0], (tag, len(data), dst_len, entropy, "verdict", got[0], want[0], len(got[1]), len(want[1]))
    assert got[2] == want[2], (tag, len(data), entropy, "dataType", got[2], want[2])
    if want[0]:
        assert len(got[1]) == len(want[1]) and got[1] == want[1], (tag, len(data), dst_len, entropy, len(got[1]), len(want[1]))
    return want


def check_inverse(ctx, data, dst_len, tag=None):
    want = model_inverse(bytes(data), dst_len)
    got = dev_inverse(ctx, bytes(data), dst_len)
    assert got[0] == want[0], (tag, len(data), dst_len, "verdict", got[0], want[0])
    if want[0]:
        assert got[1] == want[1], (tag, len(data), dst_len, len(got[1]), len(want[1]))
    return want


def check_both(ctx, data, entropy="NONE", tag=None):
    data = bytes(data)
    ok, out, _ = check_forward(ctx, data, None, entropy, tag=tag)
    if ok:
        assert check_inverse(ctx, out, len(data), tag) == (True, data), tag
        check_inverse(ctx, out, len(data) - 1, tag)
    return ok, out


# ---- 4. single blocks ------------------------------------------------------------------------------------------------------------
def test_hand_vectors_and_reference_inputs(ctx):
    tail = bytes(range(10, 30))
    vecs = [b"\x07" * 80000, b"\xfb\x01\x02" + b"\x09" * 30 + tail, b"\x01\x02\xfb\x03" + b"\xfb" * 10 + tail,
            b"\x01\x02" + b"\x09" * (2 * PIECE + 2) + tail]
    vecs += [b"\x01\x02" + b"\x09" * r + tail for r in (226, 227, 7938, 7939, PIECE)]
    applied = 0
    for i, v in enumerate(vecs):
        for e in ("NONE", "FPAQ"):
            applied += check_both(ctx, v, e, ("vec", i))[0]
    assert applied == 2 * len(vecs)
    for dst_len in (1000, 1001):
        check_forward(ctx, band_example(), dst_len, tag="band")
    counts = []
    for items in (refinputs.transform_inputs(), refinputs.edge_inputs()):
        n_ok = 0
        for i, d in enumerate(items):
            if len(d) == 0:
                continue
            ok, out, _ = check_forward(ctx, d, len(d) + 32, tag=("ref", i))
            n_ok += ok
            if ok:
                assert check_inverse(ctx, out, len(d), ("ref", i)) == (True, bytes(d))
        counts.append(n_ok)
    assert counts[0] >= 40 and counts[1] >= 25                  # (with a context: the model's own counts are in test_rlt_model.py)


def _classes(n):
    blocks = [(str(c), datagen.block(c, n).tobytes()) for c in range(5)]
    blocks.append(("exe", bytes(datagen.exe_like(n, 1))))
    blocks.append(("sensor", bytes(datagen.sensor_like(n, 1))))
    return blocks


def test_block_classes_256k(ctx):
    got = {}
    for name, b in _classes(256 << 10):
        for e in ("NONE", "FPAQ"):
            ok, out = check_both(ctx, b, e, (name, e))
            got[(name, e)] = len(out) if ok else None
    assert [got[(c, "NONE")] for c in ("0", "1", "4")] == [258511, 262066, 86497]
    assert [got[(c, "NONE")] for c in ("2", "3", "exe", "sensor")] == [None] * 4
    assert got[("0", "FPAQ")] and got[("1", "FPAQ")] and got[("exe", "FPAQ")] and got[("sensor", "FPAQ")]
    assert got[("4", "FPAQ")] == 86475 and got[("2", "FPAQ")] is None and got[("3", "FPAQ")] is None
    assert dev_forward(ctx, datagen.block(4, 256 << 10).tobytes(), 256 << 10, "FPAQ")[2] == "BIN"


def test_block_classes_4m(ctx):
    applied = 0
    for name, b in _classes(4 << 20):
        for e in ("NONE", "FPAQ"):
            applied += check_both(ctx, b, e, (name, e))[0]
    assert applied >= 6


# ---- 5. seams --------------------------------------------------------------------------------------------------------------------
def _noise(n, seed):
    """bytes without runs and without fb"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 100, n, dtype=np.uint8)
    a[1:][a[1:] == a[:-1]] += 100
    return a


def test_seams(ctx):
    cases = []
    n = 3 * TILE + 500
    for base in (64, 1024, TILE, 2 * TILE):
        for off in range(-2, 3):
            for val in (150, 0xFB):
                a = _noise(n, base + off)
                a[base + off:base + off + 50] = val                # starts at the seam
                cases.append((("start", base, off, val), a))
                a = _noise(n, base + off + 7)
                a[base + off - 50:base + off] = val                # ends at the seam
                cases.append((("end", base, off, val), a))
                a = _noise(n, base + off + 9)
                a[base + off - 3:base + off] = val                 # three copies in front of the seam, a coded run behind it
                a[base + off] = 151
                a[base + off + 1:base + off + 6] = 152
                cases.append((("short", base, off, val), a))
    for base in (19 * TILE, 18 * TILE + 1024, 18 * TILE + 64):       # the cut at 73 469 counted bytes falls on the seam
        for off in range(-2, 3):
            for extra in (0, 1, 3, 4, 100):
                a = _noise(base + 3000, base + off)
                s = base + off - PIECE
                a[s:s + PIECE + extra] = 150
                cases.append((("cut", base, off, extra), a))
    for off in range(-2, 3):                                          # a run from byte 0: the first piece has 73 473 bytes
        for extra in (0, 1, 3, 4, 5):
            a = _noise(2 * PIECE + 500, off + 10)
            a[:rltmodel.MAX_RUN + off] = 150
            a[rltmodel.MAX_RUN + off:rltmodel.MAX_RUN + off + extra] = 151
            cases.append((("first", off, extra), a))
    for n in (2 * TILE, 2 * TILE + 3, 5000):                          # the block's last bytes
        for k in range(0, 10):
            for length in (2, 3, 4, 5, 9, 40):
                for val in (150, 0xFB):
                    a = _noise(n, n + k)
                    a[max(n - k - length, 1):n - k] = val
                    cases.append((("last", n, k, length, val), a))
    for tag, a in cases:
        check_both(ctx, a.tobytes(), "NONE", tag)
    for tag, a in cases[::7]:
        check_both(ctx, a.tobytes(), "FPAQ", tag)


def test_small_blocks_and_tile_sizes(ctx):
    for n in (16, 17, 18, 31, 64, 65, 511, 512, 513, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1):
        for seed in range(3):
            rng = np.random.default_rng(n + seed)
            a = np.repeat(rng.integers(0, 4, n, dtype=np.uint8) + 0xF9, rng.integers(1, 9, n))[:n]
            for e in ("NONE", "FPAQ"):
                check_both(ctx, a.tobytes(), e, ("small", n, seed))
        check_both(ctx, b"\x00" * n, "NONE", ("zeros", n))
        check_both(ctx, b"\xfb" * n, "NONE", ("escapes", n))
    assert dev_forward(ctx, b"\x07" * 15, 64)[0] is False


def test_one_run_over_a_whole_block(ctx):
    for val in (0, 0xFB):
        ok, out = check_both(ctx, bytes([val]) * (4 << 20), "NONE", ("whole", val))
        assert ok and len(out) < 400
    ok, out = check_both(ctx, b"\x07" * (4 << 20), "FPAQ", "whole fpaq")
    assert ok and out[0] == 0


# ---- 6. data type ----------------------------------------------------------------------------------------------------------------
def test_data_type(ctx):
    runs = b"\x07" * 100 + bytes(range(30))
    for dt in ("DNA", "BASE64", "UTF8"):
        for e in ("NONE", "FPAQ"):
            assert check_forward(ctx, runs, None, e, dt)[0] is False
    for dt in ("TEXT", "BIN", "EXE"):
        for e in ("NONE", "FPAQ"):
            assert check_forward(ctx, runs, None, e, dt)[0] is True
    rng = np.random.default_rng(3)
    dna = np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, 64 << 10)].tobytes()
    want = check_forward(ctx, dna, None, "FPAQ")
    assert want[0] is False and want[2] == "DNA"
    want = check_forward(ctx, dna, None, "NONE")
    assert want[0] is True and want[2] == "UNDEFINED" and len(want[1]) == 64462
    b64 = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/", dtype=np.uint8)[rng.integers(0, 64, 5000)].tobytes()
    assert check_forward(ctx, b64, None, "FPAQ")[2] == "BASE64"
    digits = np.repeat(np.frombuffer(b"0123456789", dtype=np.uint8)[rng.integers(0, 10, 2000)], 5).tobytes()
    want = check_forward(ctx, digits, None, "FPAQ")
    assert want[0] is True and want[2] == "NUMERIC"
    ctx.set_data_type("UNDEFINED")


# ---- 7. the array-length band ----------------------------------------------------------------------------------------------------
def _band_family():
    """blocks whose coded length lies within a few bytes of n, with a coded run in the last 16 bytes"""
    rng = np.random.default_rng(77)
    out = [band_example()]
    for k in range(60):
        n = int(rng.choice([600, 1000, 1500, 5000]))
        a = ((7 * np.arange(n)) % 200).astype(np.uint8)
        for _ in range(int(rng.integers(0, 5))):                   # each early run of five saves two bytes
            p = int(rng.integers(20, n - 60))
            a[p:p + 5] = 201 + (p & 7)
        for p in rng.integers(20, n - 60, int(rng.integers(0, 8))):  # each escape costs one
            a[p] = 0xFB
        p = n - int(rng.integers(6, 17))
        a[p:p + int(rng.integers(4, 6))] = 220
        out.append(a.tobytes())
    return out


def test_dst_len_band_single_calls(ctx):
    flips = 0
    for i, b in enumerate(_band_family()):
        n = len(b)
        w0 = check_forward(ctx, b, n, tag=("band", i, "n"))
        w1 = check_forward(ctx, b, n + 33, tag=("band", i, "n+33"))
        flips += w0[0] != w1[0]
    assert flips >= 3                                             # the family does sit in the band


# ---- stage-by-stage model of a block stream ----------------------------------------------------------------------------------------
def _max_encoded(name, n):
    """getMaxEncodedLength of the stages used here (BWTBlockCodec.java:222, LZCodec.java:961-964, UTFCodec.java:308-310,
    SRT.java:365, RLT.java:419-421, TextCodec.java:512-515; ZRLT.java:243 and SBRT.java:224 return n)"""
    if name == "BWT":
        return n + 33
    if name in ("LZ", "LZX"):
        return (n + 16 if n <= 1024 else n + n // 64) + 2
    if name == "UTF":
        return n + 8192
    if name == "SRT":
        return n + 1024
    if name == "RLT":
        return rltmodel.max_encoded_length(n)
    if name == "TEXT":
        return kz.load_library().kz_transform_max_encoded_len(10, n)
    return n


def rlt_array_length(names, block_size, applied_before):
    """dst.length for RLT inside Sequence.forward under the reference's writer (one job, blocks of block_size): the two buffers swap after
    every applied stage (Sequence.java:107-114).  Even: EncodingTask's `buffer`, grown to Sequence.getMaxEncodedLength(block_size)
    (CompressedOutputStream.java:793,806-811).  Odd: `data`, max(block_size + block_size / 8, 256 KiB) (:215-216)."""
    even = block_size
    for nm in names:
        even = max(even, _max_encoded(nm, even))
    if applied_before % 2 == 0:
        return even
    return max(block_size + (block_size >> 3), 256 * 1024, even)


_WORDS = None


def _static_dict():
    global _WORDS
    if _WORDS is None:
        src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "kzo_text_dict.h")).read()
        _WORDS = katmodels.text_static_dictionary(b"".join(m.group(1).encode() for m in re.finditer(r'^\s*"([^"]*)"', src, re.M)))
    return _WORDS


def model_block(block, names, entropy, block_size, checksum=0):
    """EncodingTask.encodeBlock (CompressedOutputStream.java:733-985) stage by stage, as katmodels._knz_block states it, with RLT, LZ
    and HUFFMAN added -> (stream bytes, bits, skipFlags, mode)"""
    n = len(block)
    mode = 0
    if n <= 15:
        names, entropy = ["NONE"], "NONE"
        mode |= 0x80
    data_type = "UNDEFINED"
    if n >= 4:
        c, m, x = katmodels._magic_class(katmodels.magic_type(block))
        data_type = "BIN" if c else ("MULTIMEDIA" if m else ("EXE" if x else "UNDEFINED"))
    skip_flags = 0xFF
    cur = bytes(block)
    applied = 0
    variant = 1 if entropy in ("FPAQ", "TPAQ", "TPAQX", "CM", "ANS1") else 2
    for i, name in enumerate(names):
        if name == "NONE":
            ok, out = True, cur
        elif name == "RLT":
            ok, out, data_type = rltmodel.forward(cur, rlt_array_length(names, block_size, applied), entropy, data_type)
        elif name == "TEXT":
            ok, out, data_type = katmodels.text_forward(cur, variant, block_size, _static_dict(), data_type)
        elif name == "UTF":
            ok, out, data_type = katmodels.utf_forward(cur, data_type)
        elif name == "BWT":
            ok, out = oracle.transform_forward("BWT", cur)          # the CPU oracle (katmodels.bwt_block_forward sorts by doubling in Python;
                                                                    # on the periodic block b"xy" * 20 it also disagrees with the oracle: 15 bytes
                                                                    # behind ZRLT against 13, a matter of those two, not of RLT)
        elif name == "RANK":
            ok, out = True, katmodels.sbrt_forward(cur, 2)
        elif name == "SRT":
            ok, out = True, katmodels.srt_forward(cur)
        elif name == "ZRLT":
            ok, out = katmodels.zrlt_forward(cur)
        elif name == "LZ":
            ok, out = katmodels.lz_forward(cur, False, data_type)
        else:
            raise ValueError(name)
        if not ok:
            continue
        skip_flags &= ~(1 << (7 - i)) & 0xFF
        cur = bytes(out)
        applied += 1
    post = len(cur)
    data_size = 1 if post < 256 else (katmodels._ilog2(post) >> 3) + 1
    nb = len(names)
    mode |= ((data_size - 1) & 3) << 5
    ck_bytes = {0: 0, 32: 4, 64: 8}[checksum]

    def build(mode_byte, with_flags, payload_bits, payload_nbits):
        os_ = katmodels.JavaOutputBitStream(16384)
        os_.write_bits(mode_byte, 8)
        if with_flags:
            os_.write_bits(skip_flags, 8)
        os_.write_bits(post, 8 * data_size)
        os_.write_bits(0, 8)
        assert ck_bytes == 0
        os_.write_bytes(payload_bits, 0, payload_nbits)
        os_.close()
        return bytearray(os_.sink), os_.written()

    if (mode & 0x80) or nb <= 4:
        mode |= skip_flags >> 4
        hsf = 0 if (mode & 0x80) else ((mode << 4) | 0x0F) & 0xFF
        with_flags = False
    else:
        mode |= 0x10
        hsf = skip_flags
        with_flags = True
    if entropy == "NONE":
        bits, nbits = cur, 8 * post
    elif entropy == "ANS0":
        bits, nbits = katmodels.ans0_encode(cur)
    elif entropy == "FPAQ":
        bits = katmodels.fpaq_encode(cur)
        nbits = 8 * len(bits)
    elif entropy == "HUFFMAN":
        bits, nbits = katmodels.huffman_encode_exact(cur)
    else:
        raise ValueError(entropy)
    blob, written = build(mode, with_flags, bits, nbits)
    ck_index = (2 if with_flags else 1) + data_size
    if not (mode & 0x80) and post < ((written + 7) >> 3):
        mode = mode | 0x80 | 0x10
        with_flags = nb > 4
        hsf = skip_flags if with_flags else ((mode << 4) | 0x0F) & 0xFF
        blob, written = build(mode, with_flags, cur, post << 3)
        ck_index = (2 if with_flags else 1) + data_size
    HASH = 0x1E35A7BD
    ck = (HASH * 0x01030507) & 0xFFFFFFFF
    for v in (mode & 0xFF, hsf & 0xFF, post, (written >> 32) & 0xFFFFFFFF, written & 0xFFFFFFFF):
        ck = katmodels._mix32(ck, HASH, v)
    ck = (ck >> 23) ^ (ck >> 3)
    blob[ck_index] = ck & 0xFF
    return bytes(blob), written, skip_flags, mode & 0xFF, post


def _batch(blocks):
    bs = max(len(b) for b in blocks)
    inp = np.zeros((len(blocks), bs), dtype=np.uint8)
    lens = np.zeros(len(blocks), dtype=np.int32)
    for i, b in enumerate(blocks):
        inp[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[i] = len(b)
    return inp, lens, bs


def _check_batch(ctx, blocks, chain, entropy, block_size_set=None):
    """encode on the device (host memory), compare every block with model_block, decode; returns (out, res, want)"""
    inp, lens, bs = _batch(blocks)
    names = chain.split("+")
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, chain, entropy, inp, bs, lens, out, ostride)
    want = [model_block(b, names, entropy, block_size_set or bs) for b in blocks]
    for i, b in enumerate(blocks):
        w = want[i]
        tag = (chain, entropy, i, len(b))
        assert res[i].status == 0, tag
        assert res[i].skipFlags == w[2], tag + ("skipFlags", hex(res[i].skipFlags), hex(w[2]))
        assert res[i].mode == w[3] and res[i].length == w[4] and res[i].bits == w[1], tag + (res[i].mode, w[3], res[i].length, w[4], res[i].bits, w[1])
        assert out[i, :(w[1] + 7) // 8].tobytes() == w[0], tag
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(blocks), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, chain, entropy, block_size_set or bs, out, ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert res2[i].status == 0 and res2[i].length == len(b) and dec[i, :len(b)].tobytes() == b, (chain, entropy, i)
    return inp, lens, bs, out, res, want, dec


def test_dst_len_band_in_chains(ctx):
    ctx.reset()
    fam = [b for b in _band_family() if len(b) == 1000]
    assert len(fam) >= 8
    # RLT first: no stage applied before it, the array is Sequence.getMaxEncodedLength(1000) = 1000 bytes long
    _, _, _, _, res, want, _ = _check_batch(ctx, fam, "RLT+ZRLT", "NONE")
    declined_first = sum(1 for w in want if w[2] & 0x80)
    # behind ZRLT: blocks ZRLT accepts (every byte shifted down by one, so that its output is the band block) see the 256 KiB array,
    # blocks it declines (an fe / ff early on: two bytes each, the output would not fit) the 1000-byte one
    acc = [bytes((v - 1) & 0xFF for v in b) for b in fam if 0 not in b]
    dec = [b[:8] + b"\xff\xfe" + b[10:] for b in fam]
    for b in acc:
        assert katmodels.zrlt_forward(b)[0]
    for b in dec:
        assert not katmodels.zrlt_forward(b)[0]
    _, _, _, _, res, want, _ = _check_batch(ctx, acc + dec, "ZRLT+RLT", "NONE")
    applied_behind = sum(1 for w in want[:len(acc)] if not (w[2] & 0x40))
    declined_behind = sum(1 for w in want[len(acc):] if w[2] & 0x40)
    assert declined_first >= 2 and applied_behind > len(acc) - declined_first and declined_behind >= 2


# ---- 8. damaged input ------------------------------------------------------------------------------------------------------------
def test_inverse_failure_rules(ctx):
    hand = ["fbfb05", "fbfb00", "fbfb", "fb", "fb01", "fb0102fb", "fb01fbe0", "fb01fbff00", "fb01fbff", "fb01fb05", "fb0102", "fb01fb00",
            "fb01fb0002", "fb01fb00fb03", "fb01fb02fb03", "fb01fbffffff", "fb01fbfe00", "fb01fbe000", "0001000500", "fb01fb05fb00fb06",
            "fbfb00fb09", "fb01fbff0000fbff0001"]
    for h in hand:
        d = bytes.fromhex(h)
        ok, out = model_inverse(d, 1 << 20)
        for cap in sorted({1, 2, 7, 8, 9, 100, len(out), max(len(out) - 1, 1), len(out) + 1, 1 << 20}):
            check_inverse(ctx, d, cap, (h, cap))
    assert dev_inverse(ctx, b"\xfb", 100)[0] is False                # deliberate: the reference reads src[1] outside the block


def test_damaged_input_follows_the_reference(ctx):
    rng = np.random.default_rng(2024)
    cases = fails = 0
    for k in range(120):
        n = int(rng.choice([4 << 10, 16 << 10, 64 << 10]))
        a = np.repeat(rng.integers(0, 256, n, dtype=np.uint8), rng.choice([1, 1, 1, 2, 4, 5, 30, 300, 9000], n))[:n]
        a[rng.integers(0, n, 40)] = 0xFB
        ok, enc, _ = rltmodel.forward(a.tobytes(), n + 32)
        if not ok:
            continue
        bad = bytearray(enc)
        kind = k % 3
        if kind == 0:
            for p in rng.integers(1, len(bad), int(rng.integers(1, 6))):
                bad[p] = int(rng.choice([bad[0], 0, 0xFF, 0xE0, 0xFE, int(rng.integers(0, 256))]))
        elif kind == 1:
            bad = bad[:int(rng.integers(2, len(bad)))]
        else:
            p = int(rng.integers(1, len(bad)))
            bad[p:p] = bytes([bad[0], int(rng.choice([0, 3, 0xE5, 0xFF]))])
        bad = bytes(bad)
        full = model_inverse(bad, 1 << 22)
        length = len(full[1]) if full[0] else n
        for cap in (length, max(length - 1, 1), length + 70000):
            want = check_inverse(ctx, bad, cap, (k, kind, cap))
            cases += 1
            fails += not want[0]
    assert cases >= 300 and 30 <= fails < cases


# ---- 9. chains -------------------------------------------------------------------------------------------------------------------
def _mixed_blocks():
    rng = np.random.default_rng(11)
    blocks = [datagen.block(3, 30000).tobytes(), datagen.block(4, 28111).tobytes(), datagen.block(4, 30000).tobytes()[100:], datagen.block(0, 17000).tobytes(),
              b"0123456789abcde", bytes(rng.integers(0, 256, 5000, dtype=np.uint8)), np.repeat(rng.integers(0, 4, 400, dtype=np.uint8), 9).tobytes(),
              b"xy" * 20, b"\x00" * 20000]
    return blocks


@pytest.mark.parametrize("chain,entropy", [("RLT", "NONE"), ("RLT+BWT+RANK+ZRLT", "ANS0"), ("RLT+LZ", "HUFFMAN")])
def test_chains(ctx, chain, entropy):
    ctx.reset()
    blocks = _mixed_blocks()
    inp, lens, bs, out, res, want, dec = _check_batch(ctx, blocks, chain, entropy)
    flags = [w[2] & 0x80 for w, b in zip(want, blocks) if len(b) > 15]
    assert any(flags) and not all(flags)                         # RLT accepted some blocks and declined others
    ostride = out.shape[1]
    bits = np.array([r.bits for r in res], dtype=np.int64)
    # device memory, and the asynchronous calls
    d_in = torch.from_numpy(inp).cuda()
    d_out = torch.zeros((len(blocks), ostride), dtype=torch.uint8, device="cuda")
    res_d = kz.encode_blocks(ctx, chain, entropy, d_in.data_ptr(), bs, lens, d_out.data_ptr(), ostride, kz.MEM_DEVICE)
    host = d_out.cpu().numpy()
    for i in range(len(blocks)):
        assert res_d[i].bits == want[i][1] and res_d[i].skipFlags == want[i][2] and host[i, :(want[i][1] + 7) // 8].tobytes() == want[i][0], (chain, i)
    d_dec = torch.zeros((len(blocks), bs), dtype=torch.uint8, device="cuda")
    kz.decode_blocks(ctx, chain, entropy, bs, d_out.data_ptr(), ostride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
    assert np.array_equal(d_dec.cpu().numpy(), dec)
    out2 = np.zeros_like(out)
    kz.submit_encode_blocks(ctx, chain, entropy, inp, bs, lens, out2, ostride).wait()
    for i in range(len(blocks)):
        assert out2[i, :(want[i][1] + 7) // 8].tobytes() == want[i][0], (chain, i)
    dec2 = np.zeros_like(dec)
    kz.submit_decode_blocks(ctx, chain, entropy, bs, out, ostride, bits, dec2, bs).wait()
    assert np.array_equal(dec2, dec)


def test_chain_behind_the_host_stages(ctx):
    ctx.reset()
    bs = 30000
    text = [textgen.bulk_text(bs, s).tobytes() for s in range(2)]
    runs = bytearray(text[0])
    runs[5000:9000] = b" " * 4000
    blocks = text + [bytes(runs), textgen.bulk_text(20000, 5, "utf8").tobytes(), datagen.block(4, 25000).tobytes(), datagen.block(3, 22000).tobytes(), b"short text"]
    ctx.set_block_size(bs)
    _, _, _, _, res, want, _ = _check_batch(ctx, blocks, "TEXT+UTF+RLT+BWT+SRT+ZRLT", "FPAQ", bs)
    assert any(not (w[2] & 0x20) for w in want) and any(w[2] & 0x20 for w in want[:6])
    with pytest.raises(kz.KanziError) as e:
        _check_batch(ctx, blocks, "RLT+TEXT", "NONE", bs)
    assert "host stages in front of the GPU stages" in str(e.value)
    ctx.reset()


# ---- 10. streams -----------------------------------------------------------------------------------------------------------------
def test_whole_stream(ctx):
    ctx.reset()
    bs = 1 << 20
    parts = [datagen.block(c % 5, bs).tobytes() for c in range(8)] + [datagen.block(4, bs // 3).tobytes()]
    data = b"".join(parts)
    ctx.set_checksum(32)
    cos = kz.CompressedOutputStream(ctx, "RLT+BWT+RANK+ZRLT", "ANS0", bs, checksum=32)
    cos.write(data)
    cos.close()
    idx = kz.knz_index(cos.output)
    assert idx["transform"] == kz.transform_type("RLT+BWT+RANK+ZRLT") and (idx["transform"] >> 42) == 5
    assert kz.CompressedInputStream(ctx, cos.output).read() == data
    # every block's stream equals the batched call's for the same block (whose bytes test_chains checks against the models)
    ctx.reset()
    ctx.set_checksum(32)
    ctx.set_block_size(bs)
    inp, lens, _ = _batch(parts)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(parts), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, "RLT+BWT+RANK+ZRLT", "ANS0", inp, bs, lens, out, ostride)
    applied = 0
    assert len(idx["blocks"]) == len(parts)
    for i, (off, nbits) in enumerate(idx["blocks"]):
        assert nbits == res[i].bits, i
        assert kz.extract_bits(cos.output, off, nbits) == out[i, :(nbits + 7) // 8].tobytes(), i
        applied += not (res[i].skipFlags & 0x80)
    assert 0 < applied < len(parts)
    ctx.reset()
