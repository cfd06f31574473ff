"""Byte-addressed reads of .knz streams: kz_read_bytes / kz_read_bytes_device against plain slicing of the original data (model A,
tests/knzread.py), with and without a table of block starts, across chunk seams, on damaged streams and with a caller's index that
does not match.  Device sources sit at odd addresses; device destinations are poisoned with 0xA5 and framed by guard bytes, so the
tails of cut slots, the gap in front of dst and everything behind it must come back as they were."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import knzrange
import knzread
from layouthelp import Frame

pytestmark = pytest.mark.gpu

GUARD = 4096
STREAMS = knzrange.streams()
NAMES = [s.name for s in STREAMS]
INVALID_PARAM, WRITE_FILE, INVALID_FILE = -18, -12, -15


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
    """name -> (case, stream, index, [block bytes], block starts, ranges, model A with the table, model A without)"""
    out = {}
    for s in STREAMS:
        knz = s.build(_compress(ctx), _encode_block(ctx))
        idx = kz.knz_index(knz)
        assert len(idx["blocks"]) == s.nblocks(), s.name
        blocks = [b.tobytes() for b in s.block_data()]
        B = knzread.starts(s.block_lengths())
        rngs = knzread.ranges(s.block_lengths())
        out[s.name] = (s, knz, idx, blocks, B, rngs, knzread.model_a(blocks, s.bs, rngs, B), knzread.model_a(blocks, s.bs, rngs, None))
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


def _arrays(blocks, rngs, table):
    off = np.ascontiguousarray([b[0] for b in blocks], dtype=np.int64)
    w = np.ascontiguousarray([b[1] for b in blocks], dtype=np.int64)
    ro = np.ascontiguousarray([r[0] for r in rngs], dtype=np.int64)
    rl = np.ascontiguousarray([r[1] for r in rngs], dtype=np.int64)
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.int64)
    got = np.full(max(len(rngs), 1), 777, dtype=np.int64)
    return off, w, tab, ro, rl, got


def _p(a):
    return None if a is None or len(a) == 0 else a.ctypes.data


def host_read(ctx, knz, blocks, rngs, table=None, cap=None):
    """-> (return value, dst[0 .. cap) poisoned before the call, got)"""
    off, w, tab, ro, rl, got = _arrays(blocks, rngs, table)
    cap = int(rl.sum()) if cap is None else cap
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    dst = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    rc = ctx.lib.kz_read_bytes(ctx.h, src.ctypes.data, len(knz), _p(off), _p(w), _p(tab), len(off), _p(ro), _p(rl), len(ro), dst.ctypes.data, cap, got.ctypes.data)
    return rc, dst[:cap], [int(g) for g in got[:len(rngs)]]


def dev_read(ctx, knz, blocks, rngs, table=None, cap=None, lead=1, at=3):
    """src `lead` bytes into its tensor, dst `at` bytes into a poisoned frame whose guard follows dst[cap] directly
    -> (return value, dst[0 .. cap), got, frame)"""
    off, w, tab, ro, rl, got = _arrays(blocks, rngs, table)
    cap = int(rl.sum()) if cap is None else cap
    t, p = up(knz, lead)
    fr = Frame(at + cap, "a5", device=True, guard=GUARD)
    rc = ctx.lib.kz_read_bytes_device(ctx.h, p, len(knz), _p(off), _p(w), _p(tab), len(off), _p(ro), _p(rl), len(ro), fr.ptr(at), cap, got.ctypes.data)
    a = fr.after()
    assert fr.guards_intact(a) and bytes(a[GUARD:GUARD + at]) == b"\xa5" * at, ("guards", len(rngs), cap, lead, at)
    return rc, a[GUARD + at:GUARD + at + cap], [int(g) for g in got[:len(rngs)]], fr


def check_slots(tag, rc, dst, got, rngs, want):
    """want[i] = (got, bytes) of model A: the first got bytes of slot i are the range's, the rest of a cut slot is still 0xA5; a
    failed range carries its code (its slot is unspecified)"""
    total = sum(s for _, s in rngs)
    assert rc == total, (tag, "return value", rc, total)
    at = 0
    for i, ((o, s), (g, b)) in enumerate(zip(rngs, want)):
        assert got[i] == g, (tag, "got", i, (o, s), got[i], g)
        if g >= 0:
            assert b is None or dst[at:at + g].tobytes() == b, (tag, "bytes", i, (o, s))
            assert bool((dst[at + g:at + s] == 0xA5).all()), (tag, "the tail of a cut slot", i, (o, s))
        at += s


def both(ctx, tag, knz, blocks, rngs, want, table=None, **where):
    rc, dst, got = host_read(ctx, knz, blocks, rngs, table)
    check_slots(tag + ("host",), rc, dst, got, rngs, want)
    rc, dst, got, _ = dev_read(ctx, knz, blocks, rngs, table, **where)
    check_slots(tag + ("device",), rc, dst, got, rngs, want)


# ---- 1: model A -------------------------------------------------------------------------------------------------------------------------
def _model_a(ctx, made, name):
    s, knz, idx, blocks, B, rngs, with_table, without = made[name]
    both(ctx, (name, "table"), knz, idx["blocks"], rngs, with_table, table=B)
    both(ctx, (name, "no table"), knz, idx["blocks"], rngs, without)
    if s.lens:                                                                         # short blocks in the middle: addresses need the table
        codes = [g for g, _ in without]
        assert INVALID_FILE in codes and any(g > 0 for g in codes) and all(g >= 0 for g, _ in with_table), name
    else:
        assert with_table == without


@pytest.mark.parametrize("name", NAMES)
def test_every_range_equals_the_slice(ctx, made, name):
    _model_a(ctx, made, name)


@pytest.mark.parametrize("name", ["bwt-1k-x32", "text-4k-last1", "short-middle"])
def test_ranges_across_chunk_seams(ctx, made, name, monkeypatch):
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(knzread.CHUNK))
    _model_a(ctx, made, name)


@pytest.mark.parametrize("lead,at", [(1, 1), (3, 5), (5, 7), (2, 15), (7, 16 + 9)])
def test_reads_at_unaligned_addresses(ctx, made, lead, at):
    s, knz, idx, blocks, B, rngs, with_table, _ = made["short-middle"]
    rc, dst, got, _ = dev_read(ctx, knz, idx["blocks"], rngs, B, lead=lead, at=at)
    check_slots(("short-middle", lead, at), rc, dst, got, rngs, with_table)


# ---- 2: many small records, and one large one -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, knzread.CHUNK])
def test_the_4096_record_batch(ctx, made, chunk, monkeypatch):
    if chunk:
        monkeypatch.setenv("KZ_STREAM_CHUNK", str(chunk))
    s, knz, idx, blocks, B, _, _, _ = made[knzread.BATCH_STREAM]
    rngs = knzread.batch(s.block_lengths())
    assert len(rngs) == 4096 + 16
    want = knzread.model_a(blocks, s.bs, rngs, None)
    rc, dst, got = host_read(ctx, knz, idx["blocks"], rngs)
    check_slots(("batch", "host"), rc, dst, got, rngs, want)
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        rc, dst, got, _ = dev_read(ctx, knz, idx["blocks"], rngs, lead=3, at=5)
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    check_slots(("batch", "device"), rc, dst, got, rngs, want)
    used = len(knzread.segments(B, rngs)[0])                                            # (the last block holds 9 bytes: a record may or may not touch it)
    assert used >= s.nblocks() - 1
    nchunks = -(-used // chunk) if chunk else 1
    assert times.get("k_knz_read", {}).get("launches", 0) == nchunks, times.get("k_knz_read")   # one launch per chunk, whatever it holds
    assert "k_knz_scatter" not in times and "k_knz_walk" not in times and times.get("k_knz_check", {}).get("launches", 0) == nchunks, sorted(times)


def test_the_probes_yardstick_copies_the_same_bytes(ctx, made, monkeypatch):
    """KZ_READ_SCATTER=1 (tools/knz_read_probe.py) sends the same segments through k_knz_scatter"""
    monkeypatch.setenv("KZ_READ_SCATTER", "1")
    s, knz, idx, blocks, B, rngs, with_table, _ = made["short-middle"]
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        rc, dst, got, _ = dev_read(ctx, knz, idx["blocks"], rngs, B, lead=3, at=7)
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    check_slots(("short-middle", "scatter"), rc, dst, got, rngs, with_table)
    assert times.get("k_knz_scatter", {}).get("launches", 0) == 1 and "k_knz_read" not in times, sorted(times)


@pytest.mark.parametrize("name", NAMES)
def test_the_whole_stream_as_one_range_equals_kz_decompress(ctx, made, name):
    s, knz, idx, blocks, B, _, _, _ = made[name]
    src = np.frombuffer(knz + b"\0" * 16, dtype=np.uint8)
    ref = np.zeros(s.n, dtype=np.uint8)
    assert ctx.lib.kz_decompress(ctx.h, src.ctypes.data, len(knz), ref.ctypes.data, s.n) == s.n
    want = [(s.n, ref.tobytes())]
    both(ctx, (name, "whole"), knz, idx["blocks"], [(0, s.n)], want, table=B, lead=5, at=1)
    if not s.lens:
        both(ctx, (name, "whole, no table"), knz, idx["blocks"], [(0, s.n + 100)], want)


# ---- 3: damage -------------------------------------------------------------------------------------------------------------------------------
def _indexed(ctx, knz, offs, ws, bs):
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    dst = np.zeros(max(len(offs), 1) * bs, dtype=np.uint8)
    o, w = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(ws, dtype=np.int64)
    res = (kz.BlockResult * max(len(offs), 1))()
    rc = ctx.lib.kz_decode_indexed(ctx.h, src.ctypes.data, len(knz), o.ctypes.data, w.ctypes.data, len(offs), dst.ctypes.data, bs, ctypes.addressof(res))
    assert rc == 0, rc
    return dst, res


@pytest.mark.parametrize("name", [s.name for s in STREAMS if not s.lens])
def test_a_damaged_block_fails_the_ranges_that_touch_it(ctx, made, name):
    """What kz_decode_indexed says of a block is what the ranges that touch it carry (a block that decodes to another length than
    its address range has no byte addresses: INVALID_FILE); every other range is exact."""
    s, knz, idx, blocks, B, _, _, _ = made[name]
    nb, lens = s.nblocks(), s.block_lengths()
    for kind, bad, _ in knzrange.damaged(knz, idx, 3, 3):
        entry_ok = [knzrange.check_entry(bad, o, w) for o, w in idx["blocks"]]
        use = [k for k in range(nb) if entry_ok[k]]                                     # the read looks at the entries it uses, and at no other
        rows, res = _indexed(ctx, bad, [idx["blocks"][k][0] for k in use], [idx["blocks"][k][1] for k in use], s.bs)
        status, data = {}, {}
        for j, k in enumerate(use):
            status[k] = res[j].status if res[j].status else (0 if res[j].length == lens[k] else INVALID_FILE)
            data[k] = rows[j * s.bs:j * s.bs + lens[k]].tobytes()
        if kind == "payload-inside" and s.checksum:
            assert status[4] < 0, (name, kind)
        if kind == "header-front":
            assert status[2] < 0, (name, kind)
        # a block without a checksum may decode damaged bits to wrong bytes of the right length: its ranges are delivered, their
        # bytes are whatever the decoder made of them
        sure = {k: status[k] == 0 and data[k] == blocks[k] for k in use}
        rngs, want = [], []
        for k in use:
            cand = [(B[k] + min(3, lens[k] - 1), 20, [k])]                              # (the last block may hold a single byte)
            if k + 1 in use:
                cand.append((B[k + 1] - 5, 10, [k, k + 1]))
            for o, n, ks in cand:
                n = min(n, B[ks[-1] + 1] - o)
                failing = [status[x] for x in ks if status[x]]
                rngs.append((o, n))
                if failing:
                    want.append((failing[0], None))
                else:
                    want.append((n, b"".join(blocks[x] for x in ks)[o - B[ks[0]]:o - B[ks[0]] + n] if all(sure[x] for x in ks) else None))
        assert sum(1 for g, b in want if g >= 0 and b is not None) >= len(want) - 6, (name, kind)      # damage stays with its block
        both(ctx, (name, kind), bad, idx["blocks"], rngs, want)
        both(ctx, (name, kind, "table"), bad, idx["blocks"], rngs, want, table=B[:nb] + [B[nb]])


# ---- 4: the index is the caller's ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bwt-1k-x32", "lz-4k-x64"])
def test_index_entries_that_do_not_match_the_stream(ctx, made, name):
    s, knz, idx, blocks, B, _, _, _ = made[name]
    nb = s.nblocks()
    for mname, i, offs, ws in knzrange.index_mutants(knz, idx):
        index = list(zip(offs, ws))
        touching = [(B[i] + 1, 5), (0, 0), (B[(i + 2) % nb], 7)]                         # the second names no block, the third another one
        rc, dst, got = host_read(ctx, knz, index, touching)
        assert rc == INVALID_PARAM and "index entry %d does not match the stream" % i in ctx.error(), (name, mname, "host", rc, ctx.error())
        assert bool((dst == 0xA5).all()), (name, mname, "host dst")
        rc, dst, got, fr = dev_read(ctx, knz, index, touching)
        assert rc == INVALID_PARAM and "index entry %d does not match the stream" % i in ctx.error(), (name, mname, "device", rc, ctx.error())
        assert fr.untouched(), (name, mname, "device dst")
        # the same mutant in an entry no range uses is not looked at
        others = [(B[k] - 3, 9) for k in range(1, nb) if k != i and k - 1 != i] + [(B[k] + 2, 30) for k in range(nb - 1) if k != i]
        want = knzread.model_a(blocks, s.bs, others, None)
        both(ctx, (name, mname, "unused"), knz, index, others, want)


def test_an_index_mismatch_in_a_later_chunk_leaves_dst_untouched(ctx, made, monkeypatch):
    s, knz, idx, blocks, B, rngs, _, _ = made["bwt-1k-x32"]
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(knzread.CHUNK))
    index = [list(b) for b in idx["blocks"]]
    index[7][0] += 1                                                                   # the third chunk
    rc, dst, got = host_read(ctx, knz, index, rngs)
    assert rc == INVALID_PARAM and "index entry 7 " in ctx.error() and bool((dst == 0xA5).all())
    rc, dst, got, fr = dev_read(ctx, knz, index, rngs)
    assert rc == INVALID_PARAM and "index entry 7 " in ctx.error() and fr.untouched()


# ---- 5: arguments -----------------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx, made):
    s, knz, idx, blocks, B, _, _, _ = made["bwt-1k-x32"]
    index, nb = idx["blocks"], s.nblocks()
    rngs = [(5, 100), (B[3] - 4, 50), (0, 0)]
    total = 150
    # the destination: one byte short is refused before anything is written; the exact size is enough
    for table in (None, B):
        rc, dst, got = host_read(ctx, knz, index, rngs, table, cap=total - 1)
        assert rc == WRITE_FILE and bool((dst == 0xA5).all())
        rc, dst, got, fr = dev_read(ctx, knz, index, rngs, table, cap=total - 1)
        assert rc == WRITE_FILE and fr.untouched()
    rc, dst, got, fr = dev_read(ctx, knz, index, rngs, cap=total + 9)
    assert rc == total and got == [100, 50, 0] and bool((dst[total:] == 0xA5).all())
    # ranges
    for bad in ([(-1, 5)], [(5, -1)], [(0, 4), (-(1 << 62), 4)]):
        assert host_read(ctx, knz, index, bad, cap=16)[0] == INVALID_PARAM
        rc, dst, got, fr = dev_read(ctx, knz, index, bad, cap=16)
        assert rc == INVALID_PARAM and fr.untouched()
    # tables
    for tab in ([1] + B[1:], B[:3] + [B[3] + 1] + B[4:], B[:5] + [B[4]] + B[6:], B[:-1] + [B[-2] + s.bs + 1], [0] + [b + 1 for b in B[1:]], [-b for b in B]):
        assert len(tab) == nb + 1
        rc, dst, got = host_read(ctx, knz, index, rngs, tab)
        assert rc == INVALID_PARAM and bool((dst == 0xA5).all()), tab
        rc, dst, got, fr = dev_read(ctx, knz, index, rngs, tab)
        assert rc == INVALID_PARAM and fr.untouched(), tab
    # pointers
    L = ctx.lib
    off, w, tab, ro, rl, got = _arrays(index, rngs, None)
    src = np.frombuffer(knz + b"\0" * 16, dtype=np.uint8)
    dst = np.full(total, 0xA5, dtype=np.uint8)
    t, p = up(knz)
    fr = Frame(total, "a5", device=True, guard=GUARD)
    for fn, sp, dp in ((L.kz_read_bytes, src.ctypes.data, dst.ctypes.data), (L.kz_read_bytes_device, p, fr.ptr())):
        good = [ctx.h, sp, len(knz), _p(off), _p(w), None, nb, _p(ro), _p(rl), len(rngs), dp, total, got.ctypes.data]
        for k, v in ((1, None), (2, -1), (3, None), (4, None), (6, -1), (7, None), (8, None), (9, -1), (10, None), (11, -1), (12, None)):
            args = list(good)
            args[k] = v
            assert fn(*args) == INVALID_PARAM, (fn, k)
        assert fn(*good) == total
    # no ranges: 0, after the header checks
    for k, damaged in ((None, knz), (INVALID_FILE, b"X" + knz[1:]), (-19, knz[:10] + bytes([knz[10] ^ 0x10]) + knz[11:])):
        rc, dst, got = host_read(ctx, damaged, index, [])
        assert rc == (k or 0)
        rc, dst, got, fr = dev_read(ctx, damaged, index, [])
        assert rc == (k or 0) and fr.untouched()
        assert host_read(ctx, damaged, index, rngs)[0] == (k or total)


# ---- 6: the Python readers ---------------------------------------------------------------------------------------------------------------------
def test_read_many_agrees_with_read_at(ctx, made):
    import torch
    for name in ("bwt-1k-x32", "short-middle"):
        s, knz, idx, blocks, B, rngs, with_table, without = made[name]
        rngs = [r for r in rngs if r[0] < (1 << 40)][::3]
        t, p = up(knz, 1)
        for rd in (kz.KnzReader(ctx, knz), kz.KnzReader(ctx, t[1:1 + len(knz)])):
            accepted, single = [], []
            for o, n in rngs:
                try:
                    single.append(rd.read_at(o, n))
                    accepted.append((o, n))
                except kz.KanziError:
                    pass
            assert len(accepted) > 5 and (len(accepted) == len(rngs)) == (not s.lens), (name, len(accepted))
            many = rd.read_many([o for o, _ in accepted], [n for _, n in accepted])
            assert len(many) == len(single)
            for (o, n), a, b in zip(accepted, many, single):
                if rd.device:
                    assert a.is_cuda and a.dtype == torch.uint8
                    a, b = a.cpu().numpy().tobytes(), b.cpu().numpy().tobytes()
                assert isinstance(a, bytes) and a == b, (name, o, n)
            with pytest.raises(ValueError):
                rd.read_many([-1], [4])
            assert rd.read_many([], []) == []
    # with the table of block starts the stream with short middle blocks has byte addresses; without it a range on one of them raises
    s, knz, idx, blocks, B, rngs, with_table, without = made["short-middle"]
    data = b"".join(blocks)
    rngs = [r for r in rngs if r[0] < (1 << 40)]
    assert B == kz.block_byte_offsets(s.block_lengths(), s.bs)
    t, p = up(knz, 1)
    got = kz.KnzReader(ctx, knz, byte_offsets=B).read_many([o for o, _ in rngs], [n for _, n in rngs])
    assert got == [data[o:o + n] for o, n in rngs]
    got = kz.KnzReader(ctx, t[1:1 + len(knz)], byte_offsets=B).read_many([o for o, _ in rngs], [n for _, n in rngs])
    assert [g.cpu().numpy().tobytes() for g in got] == [data[o:o + n] for o, n in rngs]
    with pytest.raises(kz.KanziError) as e:
        kz.KnzReader(ctx, knz).read_many([0, 1024], [10, 10])
    assert e.value.code == 15
    parts, codes = kz.read_bytes(ctx, knz, idx, [0, 1024, 2048], [10, 10, 10])
    assert codes == [10, INVALID_FILE, 10] and parts == [data[:10], None, blocks[2][:10]]
