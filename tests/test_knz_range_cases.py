"""The case set of tests/knzrange.py reaches the seams the seekable .knz calls are tested at, its re-assembly helper reproduces a
stream from its own blocks, and its model of the index check accepts true entries and rejects every mutant.  No GPU: streams come
from the oracle (the chains it has) and from random block streams, placed by the host kz_knz_assemble / kz_knz_index.  If the set is
thinned, these fail."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import knzrange
import oracle


def _compress(chain, ent, bs, data, checksum):
    return oracle.compress(chain, ent, bs, data, jobs=2, checksum=checksum)


def _encode_block(chain, ent, bs, block, checksum):
    s, w, _, _ = oracle.encode_block(chain, ent, block, checksum=checksum, block_size=bs)
    return s, w


@pytest.fixture(scope="module")
def built_streams(built):
    """name -> (case, stream, index) for the chains the oracle codes (CM is the library's alone)"""
    out = {}
    for s in knzrange.streams():
        if s.ent != "CM":
            knz = s.build(_compress, _encode_block)
            out[s.name] = (s, knz, kz.knz_index(knz))
    return out


def test_the_binding_declares_the_four_calls(built):
    L = ctypes.CDLL(kz.LIB_PATH)
    for name in ("kz_decompress_range", "kz_decompress_range_device", "kz_decode_indexed", "kz_decode_indexed_device"):
        assert name in kz.ABI_SYMBOLS and hasattr(L, name), name
    for name in ("decompress_range", "decompress_range_device", "decode_indexed", "decode_indexed_device", "KnzReader"):
        assert hasattr(kz, name), name


def test_streams_by_kind():
    ss = knzrange.streams()
    assert all(8 <= s.nblocks() <= 12 for s in ss), [(s.name, s.nblocks()) for s in ss]
    assert {s.bs for s in ss} == {1024, 4096, 65536}
    assert {s.checksum for s in ss} == {0, 32, 64}
    assert {(s.chain, s.ent) for s in ss} == {("NONE", "NONE"), ("BWT+RANK+ZRLT", "ANS0"), ("LZ", "HUFFMAN"), ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0"),
                                              ("LZP+BWT", "CM")}
    assert sum(1 for s in ss if s.block_lengths()[-1] == 1) >= 2                       # a 1-byte last block
    short = [s for s in ss if s.lens]
    assert len(short) == 1 and sum(1 for l in short[0].lens[:-1] if l < short[0].bs) >= 3   # short blocks in the middle
    assert any(s.n % s.bs == 0 for s in ss if not s.lens)                              # and a stream of whole blocks only
    for s in ss:
        assert len(s.original()) == s.n and [len(b) for b in s.block_data()] == s.block_lengths(), s.name


def test_ranges_by_kind():
    for nb in (8, 10, 12):
        rs = knzrange.ranges(nb)
        got = {(f, c) for _, f, c in rs}
        assert {(0, 0), (0, nb), (0, 1), (nb - 1, 1), (nb - 1, 5), (nb, 3), (nb + 7, 1)} <= got
        assert {(f, 1) for f in range(nb)} <= got
        ch = knzrange.CHUNK
        # the skipping walk goes [0, ch), [ch, 2 ch), ...: a first block inside the second step, a range on both sides of a seam of
        # the walk, and a range longer than a chunk (decoded in two steps, which start at its first block)
        assert any(ch < f < 2 * ch and c > 0 for f, c in got)
        assert any(0 < f < ch < f + c for f, c in got)
        assert any(f > 0 and ch < c < nb - f for f, c in got)
        assert len({n for n, _, _ in rs}) == len(rs)


def test_streams_have_the_blocks_they_say(built_streams):
    for s, knz, idx in built_streams.values():
        assert len(idx["blocks"]) == s.nblocks() and idx["blockSize"] == s.bs and idx["checksum"] == s.checksum, s.name
        assert idx["inputSize"] == s.n, s.name
        assert oracle.decompress(knz, s.n + 16) == s.original(), s.name
    # prefixes that straddle a byte boundary, payloads at every bit phase but perhaps one or two
    pre = [p for s, knz, idx in built_streams.values() for p, off, w in knzrange.fields(knz, idx)]
    assert sum(1 for p in pre if p % 8 > 3) >= 10                                      # a 5-bit field from bit 4 or later crosses a byte
    assert len({off % 8 for s, knz, idx in built_streams.values() for off, _ in idx["blocks"]}) >= 7
    for s, knz, idx in built_streams.values():
        for p, off, w in knzrange.fields(knz, idx):
            assert off - p - 5 == knzrange.lw(w)


def test_chunk_seams_fall_inside_bytes(built_streams):
    """with KZ_STREAM_CHUNK = CHUNK the walk's and the decoder's chunks of the seam ranges start at odd bits"""
    ch, odd = knzrange.CHUNK, 0
    for s, knz, idx in built_streams.values():
        f = knzrange.fields(knz, idx)
        odd += sum(1 for k in (ch, 2 * ch, 1 + ch, ch - 1 + ch) if f[k][0] % 8)
    assert odd >= 12, odd


def test_reassembly_reproduces_the_stream(built_streams):
    for s, knz, idx in built_streams.values():
        nb = s.nblocks()
        assert knzrange.reassemble(knz, idx, 0, nb) == knz, s.name
        assert knzrange.reassemble(knz, idx, 0, nb + 4) == knz, s.name
        part = knzrange.reassemble(knz, idx, 2, 3)
        pidx = kz.knz_index(part)
        assert [w for _, w in pidx["blocks"]] == [w for _, w in idx["blocks"][2:5]], s.name
        assert {k: v for k, v in pidx.items() if k != "blocks"} == {k: v for k, v in idx.items() if k != "blocks"}, s.name
        for (off, w), (o2, _) in zip(idx["blocks"][2:5], pidx["blocks"]):
            assert kz.extract_bits(knz, off, w) == kz.extract_bits(part, o2, w), s.name
        if not s.lens:
            lens = s.block_lengths()[2:5]
            assert oracle.decompress(part, sum(lens) + 16) == s.original()[2 * s.bs:2 * s.bs + sum(lens)], s.name
        empty = knzrange.reassemble(knz, idx, nb, 3)
        assert kz.knz_index(empty)["blocks"] == [] and len(empty) == knzrange.header_bits(knz) // 8 + 1, s.name


def test_damage_by_kind(built_streams):
    for s, knz, idx in built_streams.values():
        if s.lens:
            continue
        cases = knzrange.damaged(knz, idx, 3, 3)
        assert [k for k, _, _ in cases] == ["payload-front", "payload-inside", "payload-behind", "header-front", "prefix-front", "truncated-inside"]
        f = knzrange.fields(knz, idx)
        for kind, bad, truth in cases:
            if kind == "truncated-inside":
                p, off, w = f[5]
                assert off + 64 < 8 * len(bad) < off + w and truth[0] == "cut", (s.name, kind)
                continue
            assert len(bad) == len(knz), (s.name, kind)
            (at,) = [i for i in range(len(knz)) if bad[i] != knz[i]]
            bits = [8 * at + k for k in range(8) if (bad[at] ^ knz[at]) & (0x80 >> k)]
            assert len(bits) == 1
            bit = bits[0]
            where = {"payload-front": 2, "payload-inside": 4, "payload-behind": 6}.get(kind)
            if where is not None:
                p, off, w = f[where]
                hdr = 8 * (7 + 8)                                                      # block header and checksum at their longest
                assert off + hdr <= bit < off + w, (s.name, kind)
                assert kz.knz_index(bad) == idx, (s.name, kind)                        # the chain of prefixes is whole
            elif kind == "header-front":
                assert f[2][1] <= bit < f[2][1] + 8 and kz.knz_index(bad) == idx, (s.name, kind)
            else:
                assert f[0][0] + 5 <= bit < f[0][1], (s.name, kind)                    # inside block 0's length field


def test_index_check_model(built_streams):
    for name, (s, knz, idx) in list(built_streams.items()) + [("synthetic", (None, knzrange.synthetic(), None))]:
        idx = kz.knz_index(knz)
        assert all(knzrange.check_entry(knz, off, w) for off, w in idx["blocks"]), name
        muts = knzrange.index_mutants(knz, idx)
        assert {"off+1", "off-1", "w+1", "w-1", "off-in-header", "end-past-stream"} <= {m[0] for m in muts}
        for mname, i, offs, ws in muts:
            verdicts = [knzrange.check_entry(knz, o, w) for o, w in zip(offs, ws)]
            assert verdicts == [k != i for k in range(len(offs))], (name, mname)
    # a prefix written with more bits than its length needs is still a prefix (the reader takes any lr): lr = 12 for W = 100
    hb = knzrange.header_bits(knzrange.synthetic())
    knz = bytearray(knzrange.synthetic()[:hb // 8]) + bytearray(40)
    field = ((12 - 3) << 12) | 100
    knz[hb // 8:hb // 8 + 3] = (field << 7).to_bytes(3, "big")
    assert knzrange.check_entry(bytes(knz), hb + 17, 100) and not knzrange.check_entry(bytes(knz), hb + 17, 101)
