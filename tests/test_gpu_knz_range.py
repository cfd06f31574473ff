"""Seekable .knz streams: kz_decompress_range / kz_decompress_range_device (a block range, the reference's from / to) and
kz_decode_indexed / kz_decode_indexed_device (blocks by a caller's index, no walk) against the calls they restate.  What a range
read of a stream S must give is what kz_decompress gives for the re-assembled stream: the range's block streams behind S's header
(tests/knzrange.py).  Device sources sit at odd addresses, device destinations are poisoned with 0xA5 and framed by guard bytes."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import knzrange
from layouthelp import Frame

pytestmark = pytest.mark.gpu

GUARD = 4096
STREAMS = knzrange.streams()
NAMES = [s.name for s in STREAMS]
WHOLE = [s.name for s in STREAMS if not s.lens]


# ---- the streams, built once by the library -------------------------------------------------------------------------------------
def _compress(ctx):
    def f(chain, ent, bs, data, checksum):
        cap = kz.compress_bound(len(data), bs)
        dst = np.empty(cap, dtype=np.uint8)
        ctx.set_checksum(checksum)
        try:
            rc = ctx.lib.kz_compress(ctx.h, kz.transform_type(chain), kz.ENTROPY_IDS[ent], bs, data.ctypes.data, len(data), dst.ctypes.data, cap)
        finally:
            ctx.set_checksum(0)
        assert rc > 0, (chain, ent, rc)
        return dst[:rc].tobytes()
    return f


def _encode_block(ctx):
    def f(chain, ent, bs, block, checksum):
        ostride = kz.max_block_stream_bytes(bs)
        src, out = np.zeros(bs, dtype=np.uint8), np.zeros(ostride, dtype=np.uint8)
        src[:len(block)] = block
        ctx.set_block_size(bs)
        ctx.set_checksum(checksum)
        try:
            res = kz.encode_blocks(ctx, chain, ent, src, bs, [len(block)], out, ostride)
        finally:
            ctx.set_checksum(0)
        assert res[0].status == 0
        return out[:(res[0].bits + 7) // 8].tobytes(), int(res[0].bits)
    return f


@pytest.fixture(scope="module")
def made(ctx):
    """name -> (case, stream, index, [block bytes])"""
    out = {}
    for s in STREAMS:
        knz = s.build(_compress(ctx), _encode_block(ctx))
        idx = kz.knz_index(knz)
        assert len(idx["blocks"]) == s.nblocks(), s.name
        out[s.name] = (s, knz, idx, [b.tobytes() for b in s.block_data()])
    return out


# ---- the calls, sources and destinations framed ------------------------------------------------------------------------------------
def up(a, lead=1):
    """bytes -> (tensor that owns the memory, device address `lead` bytes into it)"""
    import torch
    a = np.frombuffer(bytes(a), dtype=np.uint8)
    buf = np.zeros(lead + max(len(a), 1), dtype=np.uint8)
    buf[lead:lead + len(a)] = a
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + lead


def host_decompress(ctx, knz, cap):
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    dst = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    return ctx.lib.kz_decompress(ctx.h, src.ctypes.data, len(knz), dst.ctypes.data, cap), dst


def host_range(ctx, knz, first, count, cap):
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    dst = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    return ctx.lib.kz_decompress_range(ctx.h, src.ctypes.data, len(knz), first, count, dst.ctypes.data, cap), dst


def dev_range(ctx, knz, first, count, cap, lead=1, at=3):
    """src `lead` bytes into its tensor, dst `at` bytes into a poisoned frame whose guard follows dst[cap] directly"""
    t, p = up(knz, lead)
    fr = Frame(at + cap, "a5", device=True, guard=GUARD)
    rc = ctx.lib.kz_decompress_range_device(ctx.h, p, len(knz), first, count, fr.ptr(at), cap)
    a = fr.after()
    assert fr.guards_intact(a) and bytes(a[GUARD:GUARD + at]) == b"\xa5" * at, ("guards", first, count, cap, lead, at)
    return rc, a[GUARD + at:GUARD + at + cap]


def check_range(ctx, knz, first, count, want_stream, cap, tag, delivered=None, **where):
    """the host and the device range read of knz against kz_decompress of want_stream: the code, the bytes produced, and on a fault
    the bytes delivered in front of the failing block -> (code, bytes).  delivered: their number, or the list of the blocks that
    could have been delivered: then it is what kz_decompress delivered of them, in whole blocks"""
    r0, w = host_decompress(ctx, want_stream, cap)
    r1, h = host_range(ctx, knz, first, count, cap)
    r2, d = dev_range(ctx, knz, first, count, cap, **where)
    assert r1 == r0, (tag, "host range", r1, "kz_decompress of the re-assembled stream", r0)
    assert r2 == r0, (tag, "device range", r2, "kz_decompress of the re-assembled stream", r0)
    if isinstance(delivered, list):
        m = 0
        for b in delivered:
            if m + len(b) > cap or w[m:m + len(b)].tobytes() != b:
                break
            m += len(b)
        delivered = m
    m = r0 if r0 >= 0 else (delivered or 0)
    assert h[:m].tobytes() == w[:m].tobytes(), (tag, "host range: bytes")
    assert d[:m].tobytes() == w[:m].tobytes(), (tag, "device range: bytes")
    return r0, w[:m].tobytes()


# ---- 1: every range of every stream ---------------------------------------------------------------------------------------------------
def _all_ranges(ctx, made, name):
    s, knz, idx, blocks = made[name]
    nb = s.nblocks()
    for rname, first, count in knzrange.ranges(nb):
        want = b"".join(blocks[first:first + count])
        r0, got = check_range(ctx, knz, first, count, knzrange.reassemble(knz, idx, first, count), max(count, 0) * s.bs, (name, rname))
        assert r0 == len(want) and got == want, (name, rname, r0, len(want))


@pytest.mark.parametrize("name", NAMES)
def test_every_range_equals_the_reassembled_stream(ctx, made, name):
    _all_ranges(ctx, made, name)


@pytest.mark.parametrize("name", ["bwt-1k-x32", "text-4k-last1", "short-middle"])
def test_ranges_across_chunk_seams(ctx, made, name, monkeypatch):
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(knzrange.CHUNK))
    _all_ranges(ctx, made, name)


@pytest.mark.parametrize("lead", [1, 3, 5])
@pytest.mark.parametrize("at", [1, 3, 5])
def test_range_at_unaligned_addresses(ctx, made, lead, at):
    s, knz, idx, blocks = made["bwt-1k-x32"]
    for first, count in ((0, s.nblocks()), (4, 3), (s.nblocks() - 1, 1)):
        want = b"".join(blocks[first:first + count])
        for cap in (len(want), count * s.bs):                                          # the guard right behind the last byte produced
            r0, got = check_range(ctx, knz, first, count, knzrange.reassemble(knz, idx, first, count), cap, (first, count, cap), lead=lead, at=at)
            assert r0 == len(want) and got == want


def test_range_arguments(ctx, made):
    s, knz, idx, blocks = made["bwt-1k-x32"]
    src = np.frombuffer(knz + b"\0" * 16, dtype=np.uint8)
    dst = np.full(s.bs, 0xA5, dtype=np.uint8)
    t, p = up(knz)
    fr = Frame(s.bs, "a5", device=True, guard=GUARD)
    L = ctx.lib
    for first, count in ((-1, 1), (0, -1), (-5, -5)):
        assert L.kz_decompress_range(ctx.h, src.ctypes.data, len(knz), first, count, dst.ctypes.data, s.bs) == -18
        assert L.kz_decompress_range_device(ctx.h, p, len(knz), first, count, fr.ptr(), s.bs) == -18
    assert L.kz_decompress_range(ctx.h, None, len(knz), 0, 1, dst.ctypes.data, s.bs) == -18
    assert L.kz_decompress_range_device(ctx.h, p, len(knz), 0, 1, None, s.bs) == -18
    assert fr.untouched() and bool((dst == 0xA5).all())
    # the stream header is looked at before the range is: kz_decompress's codes, also for an empty range
    bad = bytearray(knz)
    bad[0] ^= 1
    for first, count in ((0, 0), (2, 1), (50, 1)):
        r0, _ = host_decompress(ctx, bytes(bad), s.bs)
        assert r0 == -15
        assert host_range(ctx, bytes(bad), first, count, s.bs)[0] == r0 and dev_range(ctx, bytes(bad), first, count, s.bs)[0] == r0
    bad = bytearray(knz)
    bad[10] ^= 0x10                                                                    # inside the transform word: the header's checksum
    assert host_range(ctx, bytes(bad), 0, 0, s.bs)[0] == dev_range(ctx, bytes(bad), 0, 0, s.bs)[0] == host_decompress(ctx, bytes(bad), s.bs)[0] == -19
    # an empty range of a stream cut behind its header reads nothing else
    hb = knzrange.header_bits(knz) // 8
    assert host_range(ctx, knz[:hb], 0, 0, s.bs)[0] == dev_range(ctx, knz[:hb], 0, 0, s.bs)[0] == 0
    assert host_range(ctx, knz[:hb], 0, 1, s.bs)[0] == dev_range(ctx, knz[:hb], 0, 1, s.bs)[0] == host_decompress(ctx, knz[:hb], s.bs)[0] == -11


# ---- 2: damage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WHOLE)
def test_damaged_streams(ctx, made, name):
    s, knz, idx, blocks = made[name]
    first, count = 3, 3
    whole = b"".join(blocks[first:first + count])
    cap = count * s.bs
    for kind, bad, truth in knzrange.damaged(knz, idx, first, count):
        tag = (name, kind)
        if truth == "slice":                                                           # damage the read does not look at
            r0, got = check_range(ctx, bad, first, count, knzrange.reassemble(knz, idx, first, count), cap, tag)
            assert r0 == len(whole) and got == whole, tag
        elif truth == "reassembled":                                                   # the range's second block is damaged
            r0, got = check_range(ctx, bad, first, count, knzrange.reassemble(bad, idx, first, count), cap, tag, delivered=s.bs)
            assert r0 < 0 or s.checksum == 0, tag                                      # a checksum catches it whatever the coder does
            if r0 < 0:
                assert got == whole[:s.bs], tag
        elif truth == "whole":                                                         # a fault in front of the range
            r0, _ = host_decompress(ctx, bad, s.nblocks() * s.bs)
            assert r0 < 0, tag
            r1, h = host_range(ctx, bad, first, count, cap)
            r2, d = dev_range(ctx, bad, first, count, cap)
            assert r1 == r0 and r2 == r0, (tag, r1, r2, r0)
            assert bool((h == 0xA5).all()) and bool((d == 0xA5).all()), (tag, "nothing is delivered")
        else:                                                                          # truncated inside the range's last block
            r0, got = check_range(ctx, bad, first, count, knzrange.reassemble(knz, idx, first, count)[:truth[1]], cap, tag, delivered=2 * s.bs)
            assert r0 == -11 and got == whole[:2 * s.bs], tag


# ---- 3: destinations that are too small -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["none-1k-last1", "bwt-1k-x32", "short-middle", "bwt-64k"])
def test_destination_sizes(ctx, made, name):
    s, knz, idx, blocks = made[name]
    nb = s.nblocks()
    for first, count in ((2, 4), (nb - 2, 2), (0, nb)):
        part = blocks[first:first + count]
        size = sum(len(b) for b in part)
        R = knzrange.reassemble(knz, idx, first, count)
        for cap in (size, size - 1, 0, size + 1, size - len(part[-1]), size - len(part[-1]) - 1):
            r0, got = check_range(ctx, knz, first, count, R, cap, (name, first, count, cap), delivered=part)
            if s.lens:
                continue          # kz_decompress counts the blocks that may start in dst per batch of its own: it alone says where the cut is
            fit, k = 0, 0
            while k < len(part) and fit + len(part[k]) <= cap:                         # the blocks that fit whole
                fit += len(part[k])
                k += 1
            if cap >= size:
                assert r0 == size and got == b"".join(part)
            else:
                assert r0 == -12 and got == b"".join(part)[:fit], (name, first, count, cap, r0)


# ---- 4: the indexed form -----------------------------------------------------------------------------------------------------------------
def host_indexed(ctx, knz, offs, ws, stride, rows=None):
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    rows = len(offs) if rows is None else rows
    dst = np.full(max(rows * stride, 1), 0xA5, dtype=np.uint8)
    o, w = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(ws, dtype=np.int64)
    res = (kz.BlockResult * max(len(offs), 1))()
    rc = ctx.lib.kz_decode_indexed(ctx.h, src.ctypes.data, len(knz), o.ctypes.data, w.ctypes.data, len(offs), dst.ctypes.data, stride, ctypes.addressof(res))
    return rc, dst, res


def dev_indexed(ctx, knz, offs, ws, stride, lead=1, at=3):
    t, p = up(knz, lead)
    fr = Frame(at + len(offs) * stride, "a5", device=True, guard=GUARD)
    o, w = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(ws, dtype=np.int64)
    res = (kz.BlockResult * max(len(offs), 1))()
    rc = ctx.lib.kz_decode_indexed_device(ctx.h, p, len(knz), o.ctypes.data, w.ctypes.data, len(offs), fr.ptr(at), stride, ctypes.addressof(res))
    a = fr.after()
    assert fr.guards_intact(a) and bytes(a[GUARD:GUARD + at]) == b"\xa5" * at, ("guards", len(offs), stride)
    return rc, a[GUARD + at:GUARD + at + len(offs) * stride], res, fr


def check_rows(tag, dst, res, stride, bs, want, failed=()):
    """row i holds want[i]; behind a row's first bs bytes nothing is written; rows of failed entries are untouched"""
    for i, b in enumerate(want):
        row = dst[i * stride:(i + 1) * stride]
        if i in failed:
            assert res[i].status < 0 and res[i].length == 0 and bool((row == 0xA5).all()), (tag, i, res[i].status)
            continue
        assert res[i].status == 0 and res[i].length == len(b), (tag, i, res[i].status, res[i].length, len(b))
        assert row[:len(b)].tobytes() == b, (tag, i, "bytes")
        assert bool((row[bs:] == 0xA5).all()), (tag, i, "the gap behind the row")


def _orders(nb):
    return {"full": list(range(nb)), "reversed": list(range(nb))[::-1], "strided": list(range(nb))[1::3], "repeated": [2, 2, nb - 1, 5, 2, 0, nb - 1]}


@pytest.mark.parametrize("name", NAMES)
def test_indexed_rows_equal_the_blocks(ctx, made, name):
    s, knz, idx, blocks = made[name]
    for oname, ids in _orders(s.nblocks()).items():
        offs, ws = [idx["blocks"][i][0] for i in ids], [idx["blocks"][i][1] for i in ids]
        want = [blocks[i] for i in ids]
        for stride in (s.bs, s.bs + 48):
            tag = (name, oname, stride)
            rc, dst, res = host_indexed(ctx, knz, offs, ws, stride)
            assert rc == 0, (tag, "host", rc, ctx.error())
            check_rows(tag + ("host",), dst, res, stride, s.bs, want)
            rc, ddst, dres, _ = dev_indexed(ctx, knz, offs, ws, stride)
            assert rc == 0, (tag, "device", rc, ctx.error())
            check_rows(tag + ("device",), ddst, dres, stride, s.bs, want)
            assert [(r.status, r.length, r.bits) for r in res[:len(ids)]] == [(r.status, r.length, r.bits) for r in dres[:len(ids)]], tag


def test_indexed_in_chunks_and_at_unaligned_addresses(ctx, made, monkeypatch):
    s, knz, idx, blocks = made["bwt-1k-x32"]
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(knzrange.CHUNK))
    ids = list(range(s.nblocks()))[::-1] + [4, 4]
    offs, ws = [idx["blocks"][i][0] for i in ids], [idx["blocks"][i][1] for i in ids]
    want = [blocks[i] for i in ids]
    rc, dst, res = host_indexed(ctx, knz, offs, ws, s.bs)
    assert rc == 0
    check_rows("host", dst, res, s.bs, s.bs, want)
    for lead, at in ((1, 1), (3, 5), (5, 3), (2, 7)):
        rc, dst, res, _ = dev_indexed(ctx, knz, offs, ws, s.bs + 5, lead=lead, at=at)
        assert rc == 0
        check_rows(("device", lead, at), dst, res, s.bs + 5, s.bs, want)
    # no entries: the header is still looked at
    assert host_indexed(ctx, knz, [], [], s.bs)[0] == 0 and dev_indexed(ctx, knz, [], [], s.bs)[0] == 0
    bad = b"X" + knz[1:]
    assert host_indexed(ctx, bad, [], [], s.bs)[0] == dev_indexed(ctx, bad, [], [], s.bs)[0] == -15


# ---- 5: the index is the caller's --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bwt-1k-x32", "lz-4k-x64"])
def test_index_entries_that_do_not_match_the_stream(ctx, made, name):
    s, knz, idx, blocks = made[name]
    for mname, i, offs, ws in knzrange.index_mutants(knz, idx):
        assert [knzrange.check_entry(knz, o, w) for o, w in zip(offs, ws)] == [k != i for k in range(len(offs))], mname
        rc, dst, res = host_indexed(ctx, knz, offs, ws, s.bs)
        assert rc == -18 and "index entry %d does not match the stream" % i in ctx.error(), (name, mname, "host", rc, ctx.error())
        assert bool((dst == 0xA5).all()), (name, mname, "host dst")
        rc, dst, res, fr = dev_indexed(ctx, knz, offs, ws, s.bs)
        assert rc == -18 and "index entry %d does not match the stream" % i in ctx.error(), (name, mname, "device", rc, ctx.error())
        assert fr.untouched(), (name, mname, "device dst")


def test_index_mismatch_in_a_later_chunk_leaves_dst_untouched(ctx, made, monkeypatch):
    s, knz, idx, blocks = made["bwt-1k-x32"]
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(knzrange.CHUNK))
    offs, ws = [o for o, _ in idx["blocks"]], [w for _, w in idx["blocks"]]
    offs[7] += 1                                                                       # the third chunk
    rc, dst, res = host_indexed(ctx, knz, offs, ws, s.bs)
    assert rc == -18 and "index entry 7 " in ctx.error() and bool((dst == 0xA5).all())
    rc, dst, res, fr = dev_indexed(ctx, knz, offs, ws, s.bs)
    assert rc == -18 and "index entry 7 " in ctx.error() and fr.untouched()


def test_a_damaged_block_header_fails_its_entry_alone(ctx, made):
    s, knz, idx, blocks = made["bwt-1k-x32"]
    bad = bytearray(knz)
    bit = idx["blocks"][2][0] + 3                                                      # block 2's mode byte
    bad[bit >> 3] ^= 0x80 >> (bit & 7)
    bad = bytes(bad)
    code, _ = host_decompress(ctx, bad, s.nblocks() * s.bs)                            # the first failing block is block 2
    assert code < 0
    ids = [1, 2, 3, 2, 0]
    offs, ws = [idx["blocks"][i][0] for i in ids], [idx["blocks"][i][1] for i in ids]
    want = [blocks[i] for i in ids]
    rc, dst, res = host_indexed(ctx, bad, offs, ws, s.bs)
    assert rc == 0 and res[1].status == res[3].status == code
    check_rows("host", dst, res, s.bs, s.bs, want, failed=(1, 3))
    rc, dst, res, _ = dev_indexed(ctx, bad, offs, ws, s.bs + 48)
    assert rc == 0 and res[1].status == res[3].status == code
    check_rows("device", dst, res, s.bs + 48, s.bs, want, failed=(1, 3))
    # a damaged payload is its block's fault as well (the stream carries checksums)
    bad = bytearray(knz)
    bit = idx["blocks"][2][0] + idx["blocks"][2][1] // 2
    bad[bit >> 3] ^= 0x80 >> (bit & 7)
    for rc, res in (host_indexed(ctx, bytes(bad), offs, ws, s.bs)[::2], dev_indexed(ctx, bytes(bad), offs, ws, s.bs)[:3:2]):
        assert rc == 0 and res[1].status < 0 and res[3].status < 0 and [res[k].status for k in (0, 2, 4)] == [0, 0, 0]


def test_a_stride_below_the_block_size_is_refused(ctx, made):
    s, knz, idx, blocks = made["lz-4k-x64"]
    offs, ws = [o for o, _ in idx["blocks"]], [w for _, w in idx["blocks"]]
    for stride in (s.bs - 1, 1024, 0, -s.bs):
        src = np.frombuffer(knz + b"\0" * 16, dtype=np.uint8)
        dst = np.full(len(offs) * s.bs, 0xA5, dtype=np.uint8)
        o, w = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(ws, dtype=np.int64)
        res = (kz.BlockResult * len(offs))()
        assert ctx.lib.kz_decode_indexed(ctx.h, src.ctypes.data, len(knz), o.ctypes.data, w.ctypes.data, len(offs), dst.ctypes.data, stride, ctypes.addressof(res)) == -18
        assert bool((dst == 0xA5).all())
        t, p = up(knz)
        fr = Frame(len(offs) * s.bs, "a5", device=True, guard=GUARD)
        assert ctx.lib.kz_decode_indexed_device(ctx.h, p, len(knz), o.ctypes.data, w.ctypes.data, len(offs), fr.ptr(), stride, ctypes.addressof(res)) == -18
        assert fr.untouched()


# ---- 6: it ran where it says ---------------------------------------------------------------------------------------------------------------
def test_the_check_kernel_ran_and_the_walk_did_not(ctx, made):
    s, knz, idx, blocks = made["bwt-64k"]
    ids = [5, 1, 7]
    offs, ws = [idx["blocks"][i][0] for i in ids], [idx["blocks"][i][1] for i in ids]
    L = ctx.lib
    fwd0, inv0 = L.kz_host_stage_blocks(0, 0), L.kz_host_stage_blocks(1, 0)
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        rc, dst, res, _ = dev_indexed(ctx, knz, offs, ws, s.bs)
        times = ctx.kernel_times()
        ctx.reset_kernel_timing()
        r2, d2 = dev_range(ctx, knz, 5, 2, 2 * s.bs)
        times_range = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    assert rc == 0
    check_rows("timed", dst, res, s.bs, s.bs, [blocks[i] for i in ids])
    for name in ("k_knz_check", "k_knz_unpack"):
        assert times.get(name, {}).get("launches", 0) > 0, (name, sorted(times))
    assert "k_knz_walk" not in times, sorted(times)
    assert (L.kz_host_stage_blocks(0, 0), L.kz_host_stage_blocks(1, 0)) == (fwd0, inv0)   # no TEXT / UTF in the chain: no block on the host
    # the range form walks: once over the blocks in front (one chunk), once over the range
    assert r2 == 2 * s.bs and d2.tobytes() == blocks[5] + blocks[6]
    assert times_range.get("k_knz_walk", {}).get("launches", 0) == 2 and "k_knz_check" not in times_range, times_range


# ---- 7: the Python readers -------------------------------------------------------------------------------------------------------------------
def test_reader_read_at(ctx, made):
    import torch
    s, knz, idx, blocks = made["bwt-1k-x32"]
    data, bs, n = b"".join(blocks), s.bs, s.n
    t, p = up(knz, 1)
    readers = [kz.KnzReader(ctx, knz), kz.KnzReader(ctx, t[1:1 + len(knz)])]
    assert readers[0].blocks == readers[1].blocks == idx["blocks"] and readers[1].device and not readers[0].device
    for offset in (0, 1, bs - 1, bs, bs + 1, 3 * bs - 5, 10 * bs, n - 1, n, n + 10):
        for size in (0, 1, 2, bs, bs + 7, 2 * bs + 7, n):                              # bs + 7 from 3 bs - 5: a span across three blocks
            want = data[offset:offset + size]
            got = readers[0].read_at(offset, size)
            assert isinstance(got, bytes) and got == want, ("bytes", offset, size, len(got))
            got = readers[1].read_at(offset, size)
            assert got.is_cuda and got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want, ("tensor", offset, size)
    assert readers[0].read_blocks([9, 0, 9, 10]) == [blocks[9], blocks[0], blocks[9], blocks[10]]
    assert [b.cpu().numpy().tobytes() for b in readers[1].read_blocks([10, 3])] == [blocks[10], blocks[3]]
    assert readers[0].read_blocks([]) == []
    with pytest.raises(IndexError):
        readers[0].read_blocks([11])
    with pytest.raises(ValueError):
        readers[0].read_at(-1, 4)


def test_reader_refuses_byte_addresses_behind_a_short_block(ctx, made):
    s, knz, idx, blocks = made["short-middle"]
    rd = kz.KnzReader(ctx, knz)
    assert rd.read_blocks(range(s.nblocks())) == blocks                               # blocks can be read
    assert rd.read_at(0, 1024) == blocks[0] and rd.read_at(7 * 1024, 100) == blocks[7]   # a whole block in front; the stream's last
    for offset, size in ((0, 1025), (1024, 10), (3 * 1024 + 5, 1), (2 * 1024, 3 * 1024)):
        with pytest.raises(kz.KanziError):
            rd.read_at(offset, size)


def test_input_stream_from_to(ctx, made):
    s, knz, idx, blocks = made["text-4k-last1"]
    nb = s.nblocks()
    for first, count in ((0, nb), (2, 3), (nb - 1, 1), (nb - 1, 4), (nb, 2), (4, 0)):
        want = b"".join(blocks[first:first + count])
        assert kz.decompress_range(ctx, knz, first, count) == want, (first, count)
        assert kz.CompressedInputStream(ctx, knz, from_block=first + 1, to_block=first + 1 + count).read() == want, (first, count)
    assert kz.CompressedInputStream(ctx, knz, from_block=3).read() == b"".join(blocks[2:])
    assert kz.CompressedInputStream(ctx, knz, to_block=3).read() == b"".join(blocks[:2])
    assert kz.CompressedInputStream(ctx, knz).read() == b"".join(blocks)
    t, p = up(knz)
    fr = Frame(3 * s.bs, "a5", device=True, guard=GUARD)
    assert kz.decompress_range_device(ctx, p, len(knz), 2, 3, fr.ptr(), 3 * s.bs) == 3 * s.bs
    assert fr.after()[GUARD:GUARD + 3 * s.bs].tobytes() == b"".join(blocks[2:5])
    out, res = kz.decode_indexed(ctx, knz, [idx["blocks"][4][0]], [idx["blocks"][4][1]])
    assert out.shape == (1, s.bs) and out[0, :res[0].length].tobytes() == blocks[4]
    with pytest.raises(kz.KanziError) as e:
        kz.decode_indexed(ctx, knz, [idx["blocks"][4][0] + 1], [idx["blocks"][4][1]])
    assert e.value.code == 18 and "index entry 0" in str(e.value)
    with pytest.raises(ValueError):
        kz.CompressedInputStream(ctx, knz, from_block=0)
