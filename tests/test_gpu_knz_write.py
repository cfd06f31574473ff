"""Byte-addressed writes of .knz streams: kz_write_bytes / kz_write_bytes_device against kz_compress of the plainly patched data
(tests/knzwrite.py: apply), with and without a table of block starts, across chunk seams, at odd addresses, on damaged streams and
with a caller's index that does not match.  The host form is the device form's reference: same bytes, same index, same codes.
Device buffers sit at odd addresses inside poisoned frames: the stream and the new bytes must come back untouched, and so must the
guards around the destination and the bytes in front of it."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import knzrange
import knzwrite
from layouthelp import Frame

pytestmark = pytest.mark.gpu

GUARD = 4096
STREAMS = knzwrite.streams()
NAMES = [s.name for s in STREAMS]
WRITTEN = [s.name for s in STREAMS if not s.lens]          # the streams kz_compress wrote
INVALID_PARAM, WRITE_FILE, INVALID_FILE = -18, -12, -15


# ---- the streams, built once by the library -------------------------------------------------------------------------------------
def compress(ctx, s, data):
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = kz.compress_bound(len(data), s.bs)
    dst = np.empty(cap, dtype=np.uint8)
    ctx.set_checksum(s.checksum)
    try:
        rc = ctx.lib.kz_compress(ctx.h, kz.transform_type(s.chain), kz.ENTROPY_IDS[s.ent], s.bs, data.ctypes.data, len(data), dst.ctypes.data, cap)
    finally:
        ctx.set_checksum(0)
    assert rc > 0, (s.name, rc)
    return dst[:rc].tobytes()


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


class Made:
    def __init__(self, ctx, s):
        self.s = s
        self.knz = s.build(lambda chain, ent, bs, data, checksum: compress(ctx, s, data), _encode_block(ctx))
        self.idx = kz.knz_index(self.knz)
        assert len(self.idx["blocks"]) == s.nblocks(), s.name
        self.data = s.original()
        self.B = knzwrite.starts(s.block_lengths())
        self.table = self.B if s.lens else None               # a stream with short middle blocks has byte addresses with its table only
        self.cases = dict(knzwrite.cases(s.block_lengths()))


@pytest.fixture(scope="module")
def made(ctx):
    return {s.name: Made(ctx, s) for s in STREAMS}


def applied(m, writes):
    return knzwrite.apply(m.data, [(o, len(p)) for o, p in writes], [p for _, p in writes])


# ---- the calls -----------------------------------------------------------------------------------------------------------------------
def _arrays(blocks, writes, table):
    off = np.ascontiguousarray([b[0] for b in blocks], dtype=np.int64)
    w = np.ascontiguousarray([b[1] for b in blocks], dtype=np.int64)
    ro = np.ascontiguousarray([o for o, _ in writes], dtype=np.int64)
    rl = np.ascontiguousarray([len(p) for _, p in writes], dtype=np.int64)
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.int64)
    new_off, new_w = np.full(max(len(off), 1), 777, dtype=np.int64), np.full(max(len(off), 1), 777, dtype=np.int64)
    return off, w, tab, ro, rl, b"".join(p for _, p in writes), new_off, new_w


def _p(a):
    return None if a is None or len(a) == 0 else a.ctypes.data


def bound(m, blocks=None):
    return kz.write_bytes_bound([min(max(w, 0), (1 << 34) - 1) for _, w in (blocks or m.idx["blocks"])], m.s.bs)


def host_write(ctx, m, writes, table=None, cap=None, knz=None, blocks=None):
    """-> (return value, dst[0 .. cap) poisoned before the call, the new index)"""
    knz = m.knz if knz is None else knz
    blocks = m.idx["blocks"] if blocks is None else blocks
    off, w, tab, ro, rl, new, new_off, new_w = _arrays(blocks, writes, table)
    cap = bound(m, blocks) if cap is None else cap
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    data = np.frombuffer(new + b"\0", dtype=np.uint8)
    dst = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    rc = ctx.lib.kz_write_bytes(ctx.h, src.ctypes.data, len(knz), _p(off), _p(w), _p(tab), len(off), _p(ro), _p(rl), len(ro), data.ctypes.data, len(new),
                                dst.ctypes.data, cap, new_off.ctypes.data, new_w.ctypes.data)
    return rc, dst[:cap], list(zip(new_off[:len(off)].tolist(), new_w[:len(off)].tolist()))


def dev_write(ctx, m, writes, table=None, cap=None, knz=None, blocks=None, leads=(1, 3, 5)):
    """the stream, the new bytes and the destination `leads` bytes into poisoned frames whose guards follow them directly
    -> (return value, dst[0 .. cap), the new index, the destination's frame)"""
    knz = m.knz if knz is None else knz
    blocks = m.idx["blocks"] if blocks is None else blocks
    off, w, tab, ro, rl, new, new_off, new_w = _arrays(blocks, writes, table)
    cap = bound(m, blocks) if cap is None else cap
    ls, ld, lo = leads
    fs, fd, fo = Frame(ls + len(knz), "a5", device=True, guard=GUARD), Frame(ld + max(len(new), 1), "a5", device=True, guard=GUARD), Frame(lo + cap, "a5", device=True, guard=GUARD)
    fs.put(ls, knz)
    fd.put(ld, new)
    rc = ctx.lib.kz_write_bytes_device(ctx.h, fs.ptr(ls), len(knz), _p(off), _p(w), _p(tab), len(off), _p(ro), _p(rl), len(ro), fd.ptr(ld), len(new),
                                       fo.ptr(lo), cap, new_off.ctypes.data, new_w.ctypes.data)
    a = fo.after()
    assert fs.untouched() and fd.untouched(), ("the stream or the new bytes were written", leads)
    assert fo.guards_intact(a) and bytes(a[GUARD:GUARD + lo]) == b"\xa5" * lo, ("guards", len(writes), cap, leads)
    return rc, a[GUARD + lo:GUARD + lo + cap], list(zip(new_off[:len(off)].tolist(), new_w[:len(off)].tolist())), fo


def both(ctx, tag, m, writes, want, table=None, **kw):
    """host and device form against the stream `want`: its bytes, its index, and nothing behind it on the host -> the host's index"""
    idx = kz.knz_index(want)["blocks"]
    rc, dst, new = host_write(ctx, m, writes, table, **{k: v for k, v in kw.items() if k != "leads"})
    assert rc == len(want), (tag, "host", rc, len(want), ctx.error())
    assert dst[:rc].tobytes() == want and bool((dst[rc:] == 0xA5).all()), (tag, "host bytes")
    assert new == idx, (tag, "host index")
    rc, dst, new, _ = dev_write(ctx, m, writes, table, **kw)
    assert rc == len(want), (tag, "device", rc, len(want), ctx.error())
    assert dst[:rc].tobytes() == want, (tag, "device bytes")
    assert new == idx, (tag, "device index")
    return idx


def decompress(ctx, knz, n):
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    out = np.zeros(n + 1, dtype=np.uint8)
    rc = ctx.lib.kz_decompress(ctx.h, src.ctypes.data, len(knz), out.ctypes.data, n + 1)
    return rc, out[:max(rc, 0)].tobytes()


def timed(ctx, fn):
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        out = fn()
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    return out, times


# ---- 1: against kz_compress of the patched data ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WRITTEN)
def test_the_result_is_kz_compress_of_the_patched_data(ctx, made, name):
    m = made[name]
    for case, writes in m.cases.items():
        want = compress(ctx, m.s, applied(m, writes))
        assert len(want) <= bound(m), (name, case)                                      # kz_write_bytes_bound suffices
        both(ctx, (name, case), m, writes, want)
        if case in ("corners", "whole", "whole-first", "first-and-last"):              # with a table: wholly covered blocks are not decoded
            both(ctx, (name, case, "table"), m, writes, want, table=m.B)


def test_short_middle_blocks(ctx, made):
    m = made["short-middle"]
    nb = m.s.nblocks()
    for case, writes in m.cases.items():
        rngs = [(o, len(p)) for o, p in writes]
        patched = applied(m, writes)
        rc, dst, new = host_write(ctx, m, writes, m.B)
        assert rc > 0, (case, rc, ctx.error())
        out = dst[:rc].tobytes()
        assert decompress(ctx, out, len(patched)) == (len(patched), patched), case
        assert new == kz.knz_index(out)["blocks"], case
        _, touched, _ = knzwrite.resolve(rngs, m.B)
        for k in range(nb):                                                             # every untouched block's payload bits are the source's
            if k not in touched:
                (o0, w0), (o1, w1) = m.idx["blocks"][k], new[k]
                assert w0 == w1 and kz.extract_bits(m.knz, o0, w0) == kz.extract_bits(out, o1, w1), (case, k)
        rc2, dst2, new2, _ = dev_write(ctx, m, writes, m.B)
        assert rc2 == rc and dst2[:rc].tobytes() == out and new2 == new, (case, "device")
        parts, got = kz.read_bytes(ctx, out, new, [o for o, _ in rngs], [n for _, n in rngs], byte_offsets=m.B)
        assert got == [n for _, n in rngs] and parts == [patched[o:o + n] for o, n in rngs], case


@pytest.mark.parametrize("name", NAMES)
def test_writing_what_is_there_returns_the_stream(ctx, made, name):
    m = made[name]
    same = [(o, m.data[o:o + len(p)]) for o, p in m.cases["corners"]]
    for tag, writes in (("same bytes", same), ("no ranges", []), ("zero lengths", m.cases["zero-lengths"])):
        both(ctx, (name, tag), m, writes, m.knz, table=m.table)
    if not m.s.lens:
        both(ctx, (name, "same bytes", "table"), m, same, m.knz, table=m.B)


# ---- 2: chunk seams, addresses, batches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bwt-1k-x32", "text-4k-last1", "short-middle"])
def test_chunk_seams(ctx, made, name, monkeypatch):
    m = made[name]
    cases = ("corners", "across-seam", "kept-run", "whole-first")
    whole = {c: host_write(ctx, m, m.cases[c], m.table) for c in cases}
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(knzwrite.CHUNK))
    for c in cases:
        rc, dst, new = whole[c]
        assert rc > 0, (name, c, rc)
        both(ctx, (name, c, "chunked"), m, m.cases[c], dst[:rc].tobytes(), table=m.table)
    rngs = [(o, len(p)) for o, p in m.cases["across-seam"]]
    touched = knzwrite.resolve(rngs, m.B)[1]
    assert touched == [1, 2, 3, 4, 5]
    (rc, _, _, _), times = timed(ctx, lambda: dev_write(ctx, m, m.cases["across-seam"], m.table))
    assert rc == whole["across-seam"][0]
    assert times.get("k_knz_write", {}).get("launches", 0) == 3 and "k_knz_gather" not in times and "k_knz_walk" not in times, sorted(times)


@pytest.mark.parametrize("leads", [(1, 3, 5), (3, 5, 15), (5, 15, 16 + 9), (15, 16 + 9, 1), (16 + 9, 1, 3)])
def test_writes_at_unaligned_addresses(ctx, made, leads):
    for name in ("bwt-1k-x32", "short-middle"):
        m = made[name]
        for case in ("unaligned", "corners"):
            rc, dst, new = host_write(ctx, m, m.cases[case], m.table)
            assert rc > 0
            both(ctx, (name, case, leads), m, m.cases[case], dst[:rc].tobytes(), table=m.table, leads=leads)


@pytest.fixture(scope="module")
def batch_stream(ctx):
    return Made(ctx, knzwrite.BATCH)


@pytest.mark.parametrize("overlap", [True, False])
def test_a_batch_of_4096_records(ctx, batch_stream, overlap):
    m = batch_stream
    writes = knzwrite.batch(m.s.n, overlap)
    assert len(writes) == 4096
    want = compress(ctx, m.s, applied(m, writes))
    rc, dst, new = host_write(ctx, m, writes)
    assert rc == len(want) and dst[:rc].tobytes() == want, ("host", rc, len(want))
    (rc, dst, new2, _), times = timed(ctx, lambda: dev_write(ctx, m, writes, leads=(3, 5, 7)))
    assert rc == len(want) and dst[:rc].tobytes() == want and new2 == new == kz.knz_index(want)["blocks"], ("device", rc, len(want))
    assert times.get("k_knz_write", {}).get("launches", 0) == 1 and "k_knz_gather" not in times, sorted(times)   # one launch for the chunk, whatever it holds


def test_the_probes_yardstick_writes_the_same_stream(ctx, made, monkeypatch):
    """KZ_WRITE_GATHER=1 (tools/knz_write_probe.py) sends the same segments through k_knz_gather"""
    m = made["short-middle"]
    rc, dst, new = host_write(ctx, m, m.cases["corners"], m.B)
    monkeypatch.setenv("KZ_WRITE_GATHER", "1")
    (rc2, dst2, new2, _), times = timed(ctx, lambda: dev_write(ctx, m, m.cases["corners"], m.B, leads=(3, 7, 1)))
    assert rc2 == rc > 0 and dst2[:rc].tobytes() == dst[:rc].tobytes() and new2 == new
    assert times.get("k_knz_gather", {}).get("launches", 0) == 1 and "k_knz_write" not in times, sorted(times)


# ---- 3: damage ---------------------------------------------------------------------------------------------------------------------------
def _flip(knz, bit):
    bad = bytearray(knz)
    bad[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(bad)


def _status(ctx, knz, entry, bs):
    """what kz_decode_indexed says of one block"""
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    dst = np.zeros(bs, dtype=np.uint8)
    o, w = np.asarray([entry[0]], dtype=np.int64), np.asarray([entry[1]], dtype=np.int64)
    res = (kz.BlockResult * 1)()
    assert ctx.lib.kz_decode_indexed(ctx.h, src.ctypes.data, len(knz), o.ctypes.data, w.ctypes.data, 1, dst.ctypes.data, bs, ctypes.addressof(res)) == 0
    return res[0].status


@pytest.mark.parametrize("kind", ["payload", "header"])
def test_damage(ctx, made, kind):
    m = made["bwt-1k-x32"]                                                              # blocks carry a checksum: damaged payload bits are noticed
    B, blocks = m.B, m.idx["blocks"]
    o4, w4 = blocks[4]
    bad = _flip(m.knz, o4 + w4 // 2 if kind == "payload" else o4 + 3)                   # the middle of block 4's payload, or its mode byte
    code = _status(ctx, bad, blocks[4], m.s.bs)
    assert code < 0
    # a touched damaged block fails the call with that block's code, and kz_last_error names it; block 2 in front of it is fine
    touching = [(B[2] + 5, b"ab"), (B[4] + 10, b"hello"), (B[6], b"x")]
    for table in (None, B):
        rc, dst, _ = host_write(ctx, m, touching, table, knz=bad)
        assert rc == code and "block 4:" in ctx.error(), (kind, "host", rc, code, ctx.error())
        rc, dst, _, _ = dev_write(ctx, m, touching, table, knz=bad)
        assert rc == code and "block 4:" in ctx.error(), (kind, "device", rc, code, ctx.error())
    # an untouched damaged block is carried over and the call succeeds
    others = [(B[2] + 5, b"ab"), (B[6], b"x")]
    good = host_write(ctx, m, others)
    rc, dst, new = host_write(ctx, m, others, knz=bad)
    assert rc == good[0] > 0 and new == good[2]
    out = dst[:rc].tobytes()
    assert kz.extract_bits(out, *new[4]) == kz.extract_bits(bad, *blocks[4]) != kz.extract_bits(m.knz, *blocks[4])
    for k in range(len(blocks)):
        if k != 4:
            assert kz.extract_bits(out, *new[k]) == kz.extract_bits(good[1][:rc].tobytes(), *new[k]), k
    rc2, dst2, new2, _ = dev_write(ctx, m, others, knz=bad)
    assert rc2 == rc and dst2[:rc].tobytes() == out and new2 == new
    # a damaged block wholly overwritten with a table is repaired; without a table it is decoded, and fails
    over = [(B[4] + 100, b"buried"), (B[4], knzwrite.payload(44, B[5] - B[4])), (B[2] + 5, b"ab")]
    patched = applied(m, over)
    want = compress(ctx, m.s, patched)
    both(ctx, (kind, "repaired"), m, over, want, table=B, knz=bad)
    assert decompress(ctx, want, len(patched)) == (len(patched), patched)
    assert host_write(ctx, m, over, None, knz=bad)[0] == code and dev_write(ctx, m, over, None, knz=bad)[0] == code


def test_index_entries_that_do_not_match_the_stream(ctx, made, monkeypatch):
    m = made["bwt-1k-x32"]
    B = m.B
    writes = [(B[1] + 3, b"abc"), (B[2] - 1, b"zz"), (B[3] + 9, b"q")]                   # touched blocks 1, 2, 3
    for chunk in (None, knzwrite.CHUNK):
        if chunk:
            monkeypatch.setenv("KZ_STREAM_CHUNK", str(chunk))
        for i, d in ((7, 1), (3, 1), (0, -1), (2, 8)):                                   # a kept block's entry behind, a touched one's (a later chunk's), a kept one in front
            index = [list(b) for b in m.idx["blocks"]]
            index[i][0] += d
            rc, dst, _ = host_write(ctx, m, writes, blocks=index)
            assert rc == INVALID_PARAM and "index entry %d does not match the stream" % i in ctx.error() and bool((dst == 0xA5).all()), (chunk, i, rc, ctx.error())
            rc, dst, _, fr = dev_write(ctx, m, writes, blocks=index)
            assert rc == INVALID_PARAM and "index entry %d does not match the stream" % i in ctx.error() and fr.untouched(), (chunk, i, rc, ctx.error())
        # of several bad entries the first in block order is named
        index = [list(b) for b in m.idx["blocks"]]
        index[8][1] += 1
        index[2][0] -= 1
        assert host_write(ctx, m, writes, blocks=index)[0] == INVALID_PARAM and "index entry 2 " in ctx.error()
        assert dev_write(ctx, m, writes, blocks=index)[0] == INVALID_PARAM and "index entry 2 " in ctx.error()
        # the entry of a block that is wholly overwritten with a table is not looked at
        index = [list(b) for b in m.idx["blocks"]]
        index[5] = [123, -9]
        over = writes + [(B[5], knzwrite.payload(45, 1024))]
        want = compress(ctx, m.s, applied(m, over))
        both(ctx, ("covered entry", chunk), m, over, want, table=B, blocks=index, cap=bound(m))
        assert host_write(ctx, m, over, None, blocks=index, cap=bound(m))[0] == INVALID_PARAM and "index entry 5 " in ctx.error()


# ---- 4: refusals, in the order of the contract ---------------------------------------------------------------------------------------------
def test_refusals(ctx, made):
    m = made["bwt-1k-x32"]                                                              # 10 blocks of 1024 bytes and one of 333
    B, n, nb, bs = m.B, m.s.n, m.s.nblocks(), m.s.bs
    writes = [(5, b"x" * 100), (B[3] - 4, b"y" * 50), (0, b"")]
    good = host_write(ctx, m, writes)
    assert good[0] > 0

    def refused(tag, code, text, w, table=None, **kw):
        rc, dst, _ = host_write(ctx, m, w, table, **kw)
        assert rc == code and (text is None or text in ctx.error()) and bool((dst == 0xA5).all()), (tag, "host", rc, ctx.error())
        rc, dst, _, fr = dev_write(ctx, m, w, table, **kw)
        assert rc == code and (text is None or text in ctx.error()) and fr.untouched(), (tag, "device", rc, ctx.error())

    # 1: arguments
    L = ctx.lib
    off, w, tab, ro, rl, new, new_off, new_w = _arrays(m.idx["blocks"], writes, None)
    src = np.frombuffer(m.knz + b"\0" * 16, dtype=np.uint8)
    data = np.frombuffer(new + b"\0", dtype=np.uint8)
    cap = bound(m)
    dst = np.full(cap, 0xA5, dtype=np.uint8)
    fs, fd, fo = Frame(len(m.knz), "a5", device=True, guard=GUARD), Frame(len(new), "a5", device=True, guard=GUARD), Frame(cap, "a5", device=True, guard=GUARD)
    fs.put(0, m.knz)
    fd.put(0, new)
    for fn, sp, pp, dp in ((L.kz_write_bytes, src.ctypes.data, data.ctypes.data, dst.ctypes.data), (L.kz_write_bytes_device, fs.ptr(), fd.ptr(), fo.ptr())):
        ok = [ctx.h, sp, len(m.knz), _p(off), _p(w), None, nb, _p(ro), _p(rl), len(writes), pp, len(new), dp, cap, new_off.ctypes.data, new_w.ctypes.data]
        for k, v in ((1, None), (2, -1), (3, None), (4, None), (6, -1), (7, None), (8, None), (9, -1), (10, None), (11, -1), (11, len(new) - 1), (11, len(new) + 1),
                     (12, None), (13, -1), (14, None), (15, None)):
            args = list(ok)
            args[k] = v
            assert fn(*args) == INVALID_PARAM, (fn, k, v)
        assert bool((dst == 0xA5).all()) if fn is L.kz_write_bytes else fo.untouched()
        args = list(ok)
        args[14] = args[15] = None                                                      # neither newBitOff nor newBits: fine
        assert fn(*args) == good[0]
    refused("negative offset", INVALID_PARAM, None, [(-1, b"abc")])
    # 2: the header's code comes before the table's and the ranges'
    for code, damaged in ((INVALID_FILE, b"X" + m.knz[1:]), (-19, m.knz[:10] + bytes([m.knz[10] ^ 0x10]) + m.knz[11:])):
        refused("header", code, None, [(n, b"zz")], [1] + B[1:], knz=damaged)
    # 3: a bad table; a range behind the data, with and without a table
    refused("table", INVALID_PARAM, "blockByteOff", writes, [1] + B[1:])
    refused("table", INVALID_PARAM, "blockByteOff", writes, B[:3] + [B[3] + 1] + B[4:])
    refused("behind, table", INVALID_PARAM, "range 1 ends behind the data", [(0, b"a"), (n - 2, b"abc")], B)
    refused("behind, table", INVALID_PARAM, "range 0 ends behind the data", [(n + 1, b"")], B)
    refused("behind, no table", INVALID_PARAM, "range 2 ends behind the data", [(0, b"a"), (n, b""), (nb * bs - 1, b"ab")])
    refused("behind, table, the index wrong as well", INVALID_PARAM, "range 0 ends behind the data", [(n - 2, b"abc")], B, blocks=[(o + 1, w_) for o, w_ in m.idx["blocks"]], cap=cap)
    # a range across the end of the short last block, without a table: refused once that block has been decoded
    for w_ in ([(n - 2, b"abcde")], [(3, b"k"), (n + 5, b"z")]):
        rc, _, _ = host_write(ctx, m, w_)
        assert rc == INVALID_PARAM and "range %d ends behind the data" % (len(w_) - 1) in ctx.error(), (rc, ctx.error())
        rc, _, _, _ = dev_write(ctx, m, w_)
        assert rc == INVALID_PARAM and "range %d ends behind the data" % (len(w_) - 1) in ctx.error(), (rc, ctx.error())
    both(ctx, "to the very end", m, [(n - 2, b"ab")], compress(ctx, m.s, applied(m, [(n - 2, b"ab")])))
    # 6: the destination one byte short; the exact size is enough
    for w_, table in ((writes, None), (writes, B), ([], None), ([(B[10], b"tail")], None)):
        size = host_write(ctx, m, w_, table)[0]
        assert size > 0
        for fn in (host_write, dev_write):
            out = fn(ctx, m, w_, table, cap=size - 1)
            assert out[0] == WRITE_FILE and "destination too small" in ctx.error(), (fn, len(w_), out[0])
            assert fn(ctx, m, w_, table, cap=size)[0] == size
    # the context's own settings are restored
    ctx.set_checksum(64)
    try:
        assert host_write(ctx, m, writes)[1].tobytes() == good[1].tobytes() and dev_write(ctx, m, writes)[0] == good[0]
        assert kz.knz_index(compress_with(ctx, m.s, m.data[:2048]))["checksum"] == 64
    finally:
        ctx.set_checksum(0)


def compress_with(ctx, s, data):
    """kz_compress under whatever checksum setting the context has now"""
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = kz.compress_bound(len(data), s.bs)
    dst = np.empty(cap, dtype=np.uint8)
    rc = ctx.lib.kz_compress(ctx.h, kz.transform_type(s.chain), kz.ENTROPY_IDS[s.ent], s.bs, data.ctypes.data, len(data), dst.ctypes.data, cap)
    assert rc > 0
    return dst[:rc].tobytes()


# ---- 5: the Python readers ---------------------------------------------------------------------------------------------------------------
def test_write_many_then_read_many(ctx, made):
    import torch
    for name in ("bwt-1k-x32", "short-middle"):
        m = made[name]
        writes = m.cases["corners"]
        offs, pays = [o for o, _ in writes], [p for _, p in writes]
        patched = applied(m, writes)
        want = [patched[o:o + len(p)] for o, p in writes]                               # "later wins" resolved
        assert want != pays
        t = torch.from_numpy(np.frombuffer(b"\0" + m.knz, dtype=np.uint8).copy()).cuda()
        for rd in (kz.KnzReader(ctx, m.knz, byte_offsets=m.table), kz.KnzReader(ctx, t[1:], byte_offsets=m.table)):
            new = rd.write_many(offs, pays)
            assert isinstance(new, kz.KnzReader) and new.device == rd.device and new.byte_offsets == rd.byte_offsets and len(new.blocks) == len(rd.blocks)
            got = new.read_many(offs, [len(p) for p in pays])
            if rd.device:
                assert all(g.is_cuda for g in got)
                got = [g.cpu().numpy().tobytes() for g in got]
                assert decompress(ctx, new.src.cpu().numpy().tobytes(), len(patched)) == (len(patched), patched)
            else:
                assert decompress(ctx, new.src, len(patched)) == (len(patched), patched)
            assert got == want, name
            old = rd.read_many(offs, [len(p) for p in pays])                            # the reader written from is unchanged
            old = [g.cpu().numpy().tobytes() if rd.device else g for g in old]
            assert old == [m.data[o:o + len(p)] for o, p in writes]
            assert len(rd.write_many([], []).blocks) == len(rd.blocks)
            with pytest.raises(ValueError):
                rd.write_many([-1], [b"a"])
            with pytest.raises(kz.KanziError) as e:
                rd.write_many([m.s.n - 1], [b"ab"])
            assert e.value.code == 18
    m = made["bwt-1k-x32"]
    new, idx = kz.write_bytes(ctx, m.knz, m.idx, [5], [b"hello"])
    assert new == compress(ctx, m.s, m.data[:5] + b"hello" + m.data[10:]) and idx == kz.knz_index(new)["blocks"]
