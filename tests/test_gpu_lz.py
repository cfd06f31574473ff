"""LZ / LZX on the device (kanzi_amd/csrc/kz_lz.hip) on the case set of tests/lzcases.py: every case was built to land on one seam of
k_lz_fwd's or k_lz_inv's shortcuts, and tests/test_lz_cases.py proves on the CPU that it does.  The parse is a choice -- any valid parse
round-trips -- so every comparison here is byte equality with the oracle's output: there is no tolerance anywhere in this file."""
import ctypes
import functools

import numpy as np
import pytest

import kanzi_amd as kz
import lzcases
import oracle

pytestmark = pytest.mark.gpu

GUARD = 64


@functools.lru_cache(maxsize=None)
def _want(name, codec):
    """the oracle's (applied, bytes) of a case, computed once for every test of this module"""
    c = next(c for c in lzcases.cases() if c.name == name)
    ok, out, _ = oracle.transform_forward(codec, c.data, data_type=oracle.DT[c.dtype])
    return ok, out


def _fwd(ctx, codec, data):
    tid = kz.TRANSFORM_IDS[codec]
    cap = ctx.lib.kz_transform_max_encoded_len(tid, len(data))
    out = np.zeros(cap + GUARD, dtype=np.uint8)
    p = ctypes.c_int32(0)
    a = np.frombuffer(data, dtype=np.uint8)
    rc = ctx.lib.kz_transform_forward(ctx.h, tid, a.ctypes.data, len(data), out.ctypes.data, cap, ctypes.addressof(p))
    assert rc >= 0, ctx.error()
    assert not out[cap:].any(), "kz_transform_forward wrote behind dstCap"
    return rc == 1, out[:p.value].tobytes()


def _inv(ctx, codec, data, cap):
    tid = kz.TRANSFORM_IDS[codec]
    out = np.zeros(cap + GUARD, dtype=np.uint8)
    p = ctypes.c_int32(0)
    a = np.frombuffer(data, dtype=np.uint8)
    rc = ctx.lib.kz_transform_inverse(ctx.h, tid, a.ctypes.data, len(data), out.ctypes.data, cap, ctypes.addressof(p))
    assert rc >= 0, ctx.error()
    assert not out[cap:].any(), "kz_transform_inverse wrote behind dstCap"
    return rc == 1, out[:p.value].tobytes()


def _groups():
    """the cases by size: the two of 256 KiB, those above 16 KiB, the rest"""
    cs = lzcases.cases()
    return {"small": [c for c in cs if len(c.data) <= 16 << 10], "medium": [c for c in cs if 16 << 10 < len(c.data) < 200 << 10],
            "big": [c for c in cs if len(c.data) >= 200 << 10]}


@pytest.mark.parametrize("group", ["small", "medium", "big"])
def test_forward_single_calls(ctx, group):
    """every case through kz_transform_forward with its data type: the applied flag and every byte are the oracle's, nothing is
    written behind dstCap"""
    n = 0
    for c in _groups()[group]:
        for codec in c.codecs:
            ok_o, enc_o = _want(c.name, codec)
            try:
                ctx.set_data_type(c.dtype)
                ok, enc = _fwd(ctx, codec, c.data)
            finally:
                ctx.set_data_type(0)
            assert ok == ok_o, (c.name, codec, ok, ok_o)
            if ok_o:
                assert len(enc) == len(enc_o) and enc == enc_o, (c.name, codec, len(enc), len(enc_o), _first_difference(enc, enc_o))
            n += 1
    assert n >= 4


def _first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


@pytest.mark.parametrize("codec", ["LZ", "LZX"])
def test_forward_batched(ctx, codec):
    """all UNDEFINED cases of a codec as one ragged batch (per-block hash tables, the three-way split of each scratch row): bits, skip
    flags, length and bytes of every block are oracle.encode_block's; the rows are filled with 0xA5 behind the blocks' lengths.  Then
    the same batch in reversed order on the same context: no block's result may change (stale arena or table state)."""
    cs = [c for c in lzcases.cases() if c.dtype == "UNDEFINED" and codec in c.codecs]
    bs = max(len(c.data) for c in cs)
    assert bs == 262154 and len(cs) >= 30
    ostride = kz.max_block_stream_bytes(bs)
    want = [oracle.encode_block(codec, "NONE", c.data) for c in cs]
    firsts = None
    for order in (list(range(len(cs))), list(range(len(cs) - 1, -1, -1))):
        inp = np.full((len(cs), bs), 0xA5, dtype=np.uint8)
        lens = np.zeros(len(cs), dtype=np.int32)
        for row, i in enumerate(order):
            inp[row, :len(cs[i].data)] = np.frombuffer(cs[i].data, dtype=np.uint8)
            lens[row] = len(cs[i].data)
        out = np.zeros((len(cs), ostride), dtype=np.uint8)
        res = kz.encode_blocks(ctx, codec, "NONE", inp, bs, lens, out, ostride)
        got = {}
        for row, i in enumerate(order):
            so, w, sf, pl = want[i]
            assert res[row].status == 0, (cs[i].name, row)
            assert (res[row].bits, res[row].skipFlags, res[row].length) == (w, sf, pl), (cs[i].name, row, res[row].bits, w, res[row].skipFlags, sf, res[row].length, pl)
            got[i] = out[row, :(w + 7) // 8].tobytes()
            assert got[i] == so, (cs[i].name, row, _first_difference(got[i], so))
        assert firsts is None or got == firsts
        firsts = got
    applied = sum(1 for so, w, sf, pl in want if not sf & 0x80)
    assert applied >= 25 and applied < len(cs)


@pytest.mark.parametrize("group", ["small", "medium", "big"])
def test_inverse_single_calls(ctx, group):
    """the oracle's frame of every applied case through kz_transform_inverse, with room for exactly the block and for one byte more"""
    n = 0
    for c in _groups()[group]:
        for codec in c.codecs:
            ok_o, enc_o = _want(c.name, codec)
            if not ok_o:
                continue
            for cap in (len(c.data), len(c.data) + 1):
                assert _inv(ctx, codec, enc_o, cap) == (True, c.data), (c.name, codec, cap)
            n += 1
    assert n >= 4


@pytest.mark.parametrize("codec", ["LZ", "LZX"])
def test_inverse_batched(ctx, codec):
    """the oracle's block streams of all UNDEFINED cases as one ragged batch through kz_decode_blocks: every block comes back"""
    cs = [c for c in lzcases.cases() if c.dtype == "UNDEFINED" and codec in c.codecs]
    bs = max(len(c.data) for c in cs)
    ostride = kz.max_block_stream_bytes(bs)
    streams = np.zeros((len(cs), ostride), dtype=np.uint8)
    bits = np.zeros(len(cs), dtype=np.int64)
    for i, c in enumerate(cs):
        so, w, sf, pl = oracle.encode_block(codec, "NONE", c.data)
        streams[i, :len(so)] = np.frombuffer(so, dtype=np.uint8)
        bits[i] = w
    dec = np.full((len(cs), bs), 0xA5, dtype=np.uint8)
    res = kz.decode_blocks(ctx, codec, "NONE", bs, streams, ostride, bits, dec, bs)
    for i, c in enumerate(cs):
        assert res[i].status == 0 and res[i].length == len(c.data), (c.name, res[i].status, res[i].length)
        assert dec[i, :len(c.data)].tobytes() == c.data, c.name


@pytest.mark.parametrize("codec", ["LZ", "LZX"])
def test_inverse_recoded_and_edited_frames(ctx, codec):
    """a frame whose match-length stream holds a 4-byte code (no forward pass writes one; the decoder must read it), and valid frames
    with one edit each: the device gives the reference's verdict, and its bytes where the reference accepts.  Every frame ends in the
    reference's decoder (tests/test_lz_cases.py); bytes of a refused frame are not part of the contract."""
    small, big = (next(c for c in lzcases.cases() if c.name == n) for n in lzcases.SURGERY_CASES)
    frame, big_frame = _want(small.name, codec)[1], _want(big.name, codec)[1]
    assert _inv(ctx, codec, lzcases.recode_mlen_4byte(frame), len(small.data)) == (True, small.data)
    verdicts = []
    for label, bad in lzcases.surgery(frame, big_frame):
        cap = len(big.data) if "window" in label else len(small.data)
        ok_o, out_o = oracle.transform_inverse(codec, bad, cap)
        ok, out = _inv(ctx, codec, bad, cap)
        assert ok == ok_o, (label, ok, ok_o)
        if ok_o:
            assert out == out_o, label
        verdicts.append(ok_o)
    assert verdicts.count(False) == 5 and verdicts.count(True) == 1
