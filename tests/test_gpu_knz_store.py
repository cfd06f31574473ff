"""The many-stream index and read (kz_knz_index_many_device / kz_read_bytes_many_device) against the single-stream calls they
restate: kz_knz_index_device on each segment alone and the loop of kz_read_bytes_device per stream are the reference throughout and
never the code under test.  The case set is tests/storecases.py: the thirty streams of manycases.buffers and two joined ones with
tables, packed into one buffer at every residue mod 16 with poison between them; the ranges of all streams interleaved; the
destination poisoned with 0xA5, at an odd address and framed by guard bytes."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import knzread
import manycases as mc
import storecases as sc
from layouthelp import Frame

pytestmark = pytest.mark.gpu

GUARD = 4096
INVALID_PARAM, WRITE_FILE, INVALID_FILE = -18, -12, -15
CHAIN_IDS = ["%s&%s" % c for c in mc.CHAINS]
MIXED_BS = 1024
SENT = 777                         # what got[] and streamStatus[] hold before a call


def _p(a):
    return None if a is None or len(a) == 0 else a.ctypes.data


def i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


# ---- the streams, built once by the library ------------------------------------------------------------------------------------------
_MADE = {}


def made(ctx, chain, ent, bs):
    """-> dict(sts: storecases.streams, streams: their .knz bytes, blocks: their decoded blocks, tables, headers)"""
    import torch
    key = (chain, ent, bs)
    if key in _MADE:
        return _MADE[key]
    bufs = mc.buffers(chain, bs)
    src, soff = mc.pack(bufs)
    t = torch.from_numpy(src).cuda()
    caps = [kz.compress_bound(len(b), bs) for b in bufs]
    doff, payload = mc.slots(caps)
    dst = torch.full((payload + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = kz.compress_many_device(ctx, chain, ent, bs, t.data_ptr(), soff, [len(b) for b in bufs], dst.data_ptr(), doff, caps)
    assert all(n > 0 for n in sizes), sizes
    h = dst.cpu().numpy()
    streams = [h[o:o + n].tobytes() for o, n in zip(doff, sizes)]
    blocks = [[b[k:k + bs].tobytes() for k in range(0, len(b), bs)] for b in bufs]
    sts = sc.streams(bs)
    for st in sts[len(bufs):]:
        pieces, isz = kz.splice_concat([kz.knz_index(streams[p]) for p in st.parts])
        streams.append(kz.knz_splice([streams[p] for p in st.parts], pieces, isz))
        blocks.append([b for p in st.parts for b in blocks[p]])
    for st, bl in zip(sts, blocks):
        assert [len(b) for b in bl] == st.lens, st.name
    _MADE[key] = dict(sts=sts, streams=streams, blocks=blocks, tables=[st.table for st in sts], headers=[key] * len(sts), bs=bs,
                      bufs=bufs, dst=dst, doff=doff, sizes=sizes)
    return _MADE[key]


def made_mixed(ctx):
    """stream s under chain s mod 4: four header groups in one call"""
    if "mixed" not in _MADE:
        per = [made(ctx, c, e, MIXED_BS) for c, e in mc.CHAINS]
        n = len(per[0]["sts"])
        _MADE["mixed"] = dict(sts=per[0]["sts"], streams=[per[s % 4]["streams"][s] for s in range(n)], blocks=[per[s % 4]["blocks"][s] for s in range(n)],
                              tables=per[0]["tables"], headers=[mc.CHAINS[s % 4] for s in range(n)], bs=MIXED_BS)
    return _MADE["mixed"]


def case(ctx, which):
    return made_mixed(ctx) if which == "mixed" else made(ctx, *which)


CASES = [(c, e, bs) for bs in mc.BLOCK_SIZES for c, e in mc.CHAINS] + ["mixed"]
CASE_IDS = ["%s&%s-%d" % c if c != "mixed" else c for c in CASES]


class Dev:
    """the streams in one device buffer, as manycases.pack lays them out: every residue mod 16, `fill` between and behind them"""

    def __init__(self, streams, fill=0xA5):
        import torch
        buf, self.off = mc.pack(streams, fill=fill)
        self.len = [len(s) for s in streams]
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr()


# ---- the index: the call under test and the reference ----------------------------------------------------------------------------------
def index_many(ctx, dev, cap=None, null=False):
    """-> (rc, status, indexFirst, header columns, blockBitOff, blockBits) with every array pre-set to a sentinel"""
    n = len(dev.off)
    so, sl = i64(dev.off), i64(dev.len)
    hdr = [np.full(n, 0x77, dtype=np.uint64), np.full(n, 0x77, dtype=np.uint32), np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int32)]
    status, first = np.full(n, 12345, dtype=np.int32), np.full(n + 1, -9, dtype=np.int64)
    cap = sum(x * 8 // 9 + 16 for x in dev.len) if cap is None else cap
    off, bits = np.full(cap + 8, -3, dtype=np.int64), np.full(cap + 8, -3, dtype=np.int64)
    rc = ctx.lib.kz_knz_index_many_device(ctx.h, dev.ptr, _p(so), _p(sl), n, *[a.ctypes.data for a in hdr], status.ctypes.data, first.ctypes.data,
                                          None if null else off.ctypes.data, None if null else bits.ctypes.data, cap)
    return rc, [int(x) for x in status], [int(x) for x in first], [[int(x) for x in a] for a in hdr], off, bits


def index_single(ctx, dev, s):
    """kz_knz_index_device on segment s alone -> (rc, header fields, entries)"""
    tt, et, bs, isz, chk = ctypes.c_uint64(0x77), ctypes.c_uint32(0x77), ctypes.c_int32(-7), ctypes.c_int64(-7), ctypes.c_int32(-7)
    cap = dev.len[s] * 8 // 9 + 16
    off, bits = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
    rc = ctx.lib.kz_knz_index_device(ctx.h, dev.ptr + dev.off[s], dev.len[s], ctypes.addressof(tt), ctypes.addressof(et), ctypes.addressof(bs), ctypes.addressof(isz),
                                     ctypes.addressof(chk), off.ctypes.data, bits.ctypes.data, cap)
    k = max(rc, 0)
    return rc, [tt.value, et.value, bs.value, isz.value, chk.value], list(zip(off[:k].tolist(), bits[:k].tolist()))


def assert_index_parity(ctx, tag, dev):
    """-> (the single calls' codes, the index per stream)"""
    rc, status, first, hdr, off, bits = index_many(ctx, dev)
    ref = [index_single(ctx, dev, s) for s in range(len(dev.off))]
    at, index = 0, []
    for s, (rc0, fields, entries) in enumerate(ref):
        assert status[s] == rc0, (tag, "status", s, status[s], rc0)
        assert [h[s] for h in hdr] == fields, (tag, "header fields", s)
        assert first[s] == at, (tag, "indexFirst", s)
        if rc0 >= 0:
            assert list(zip(off[at:at + rc0].tolist(), bits[at:at + rc0].tolist())) == entries, (tag, "entries", s)
            at += rc0
        index.append(entries if rc0 >= 0 else [])
    assert rc == at == first[-1], (tag, "total", rc, at)
    assert bool((off[at:] == -3).all()) and bool((bits[at:] == -3).all()), (tag, "entries behind the total")
    return [r[0] for r in ref], index


@pytest.mark.parametrize("which", CASES, ids=CASE_IDS)
def test_index_equals_the_single_call_on_every_segment(ctx, which):
    m = case(ctx, which)
    dev = Dev(m["streams"])
    codes, index = assert_index_parity(ctx, which, dev)
    assert codes == [len(st.lens) for st in m["sts"]] and codes[0] == 0                  # the empty buffer's stream has no entries
    total = sum(codes)
    # a cap below the total: the total comes back, indexFirst is complete, only the entries below cap are written
    for cap in (total - 1, total // 2, 1):
        rc, status, first, _, off, bits = index_many(ctx, dev, cap=cap)
        assert rc == total and status == codes and first[-1] == total, (which, cap)
        flat = [e for ix in index for e in ix]
        assert list(zip(off[:cap].tolist(), bits[:cap].tolist())) == flat[:cap], (which, cap)
        assert bool((off[cap:] == -3).all()) and bool((bits[cap:] == -3).all()), (which, cap, "guard values behind cap")
    rc, status, first, _, _, _ = index_many(ctx, dev, cap=0, null=True)
    assert rc == total and status == codes and first[-1] == total


def test_index_of_damaged_streams_next_to_good_ones(ctx):
    """truncated streams, damaged headers and damaged prefixes get the single call's code, never a device fault; their neighbours
    are unchanged"""
    import torch
    data = mc.small_input()
    t = torch.from_numpy(data.copy()).cuda()
    cap = kz.compress_bound(len(data), mc.SMALL_BS)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    n = kz.compress_device(ctx, *mc.SMALL_CHAIN, mc.SMALL_BS, t.data_ptr(), len(data), dst.data_ptr(), cap)
    knz = dst[:n].cpu().numpy().tobytes()
    blocks = kz.knz_index(knz)["blocks"]
    assert len(blocks) == 3
    bad = mc.truncations(knz) + mc.header_faults(knz) + mc.prefix_faults(knz, blocks)
    streams, goods = mc.interleave(bad, knz)
    dev = Dev(streams)
    codes, index = assert_index_parity(ctx, "damaged", dev)
    assert all(codes[i] == 3 and index[i] == blocks for i in goods)
    faults = {codes[i] for i in range(len(streams)) if i not in set(goods)}
    assert INVALID_FILE in faults and len([c for c in faults if c < 0]) >= 4, faults
    index_many(ctx, dev)
    assert "stream 1:" in ctx.error(), ctx.error()                                       # the first failing stream: the cut to 0 bytes


# ---- the read: the call under test and the reference loop --------------------------------------------------------------------------------
def store_arrays(index, tables):
    first = np.zeros(len(index) + 1, dtype=np.int64)
    first[1:] = np.cumsum([len(ix) for ix in index])
    off, w = i64([e[0] for ix in index for e in ix]), i64([e[1] for ix in index for e in ix])
    tfirst, tab = None, None
    if tables is not None and any(t is not None for t in tables):
        tfirst, flat = np.full(len(index), -1, dtype=np.int64), []
        for s, t in enumerate(tables):
            if t is not None:
                tfirst[s] = len(flat)
                flat += list(t)
        tab = i64(flat)
    return first, off, w, tfirst, tab


def many_read(ctx, dev, index, tables, rngs, at=3, cap=None):
    """dst `at` bytes into a poisoned frame whose guard follows dst[cap] directly -> (rc, dst[0 .. cap), got, streamStatus, frame)"""
    first, off, w, tfirst, tab = store_arrays(index, tables)
    rs, ro, rl = np.ascontiguousarray([r[0] for r in rngs], dtype=np.int32), i64([r[1] for r in rngs]), i64([r[2] for r in rngs])
    got, status = np.full(max(len(rngs), 1), SENT, dtype=np.int64), np.full(max(len(index), 1), SENT, dtype=np.int32)
    cap = int(rl.sum()) if cap is None else cap
    fr = Frame(at + cap, "a5", device=True, guard=GUARD)
    so, sl = i64(dev.off), i64(dev.len)
    rc = ctx.lib.kz_read_bytes_many_device(ctx.h, dev.ptr, _p(so), _p(sl), len(dev.off), first.ctypes.data, _p(off), _p(w),
                                           None if tfirst is None else tfirst.ctypes.data, _p(tab), _p(rs), _p(ro), _p(rl), len(rngs), fr.ptr(at), cap,
                                           got.ctypes.data, status.ctypes.data)
    a = fr.after()
    assert fr.guards_intact(a) and bytes(a[GUARD:GUARD + at]) == b"\xa5" * at, ("guards", len(rngs), cap, at)
    return rc, a[GUARD + at:GUARD + at + cap], [int(g) for g in got[:len(rngs)]], [int(c) for c in status[:len(index)]], fr


def loop_read(ctx, dev, index, tables, rngs):
    """kz_read_bytes_device per named stream, asked that stream's ranges in their call order -> ([(got, bytes or None)] in call
    order, {stream: min(the call's return value, 0)})"""
    out, codes = [None] * len(rngs), {}
    for s in sorted({r[0] for r in rngs}):
        mine, idx = sc.of_stream(rngs, s)
        off, w = i64([e[0] for e in index[s]]), i64([e[1] for e in index[s]])
        tab = None if tables is None or tables[s] is None else i64(tables[s])
        ro, rl = i64([r[0] for r in mine]), i64([r[1] for r in mine])
        got = np.full(len(mine), SENT, dtype=np.int64)
        cap = int(rl.sum())
        fr = Frame(5 + cap, "a5", device=True, guard=GUARD)
        rc = ctx.lib.kz_read_bytes_device(ctx.h, dev.ptr + dev.off[s], dev.len[s], _p(off), _p(w), _p(tab), len(off), _p(ro), _p(rl), len(mine), fr.ptr(5), cap, got.ctypes.data)
        codes[s] = min(rc, 0)
        a = fr.after()[GUARD + 5:GUARD + 5 + cap]
        pos = 0
        for i, (o, n), g in zip(idx, mine, got.tolist()):
            out[i] = (rc, None) if rc < 0 else (g, a[pos:pos + g].tobytes() if g >= 0 else None)
            pos += n
    return out, codes


def check_slots(tag, rc, dst, got, rngs, want):
    """want[i] = (got, bytes or None): the first got bytes of slot i are the range's, the rest of a cut slot is still 0xA5; a failed
    range carries its code (its slot is unspecified)"""
    total = sum(n for _, _, n in rngs)
    assert rc == total, (tag, "return value", rc, total)
    at = 0
    for i, ((s, o, n), (g, b)) in enumerate(zip(rngs, want)):
        assert got[i] == g, (tag, "got", i, (s, o, n), got[i], g)
        if g >= 0:
            assert b is None or dst[at:at + g].tobytes() == b, (tag, "bytes", i, (s, o, n))
            assert bool((dst[at + g:at + n] == 0xA5).all()), (tag, "the tail of a cut slot", i, (s, o, n))
        at += n


_REF = {}


def reference(ctx, which):
    """(dev, index, ranges, the loop's results, model A) of a case, computed once"""
    if which not in _REF:
        m = case(ctx, which)
        dev = Dev(m["streams"])
        _, index = assert_index_parity(ctx, which, dev)
        rngs = sc.call(m["sts"])
        loop, codes = loop_read(ctx, dev, index, m["tables"], rngs)
        assert all(c == 0 for c in codes.values()), codes
        model = sc.model_a(m["blocks"], m["bs"], rngs, m["tables"])
        assert loop == model, (which, "the reference loop against plain slicing")
        _REF[which] = (dev, index, rngs, loop)
    return _REF[which]


@pytest.mark.parametrize("which", CASES, ids=CASE_IDS)
def test_read_equals_the_loop_over_the_streams(ctx, which):
    m = case(ctx, which)
    dev, index, rngs, loop = reference(ctx, which)
    assert {r[0] for r in rngs} == set(range(len(m["sts"])))
    if which == "mixed":
        assert len(set(sc.groups_of(m["headers"], rngs).values())) == 4
    rc, dst, got, status, _ = many_read(ctx, dev, index, m["tables"], rngs)               # d_dst at an odd address
    check_slots(which, rc, dst, got, rngs, loop)
    assert status == [0] * len(index)
    # the joined streams without their tables: INVALID_FILE for the ranges on their short blocks, as in the loop
    loop2, codes = loop_read(ctx, dev, index, None, [r for r in rngs if r[0] >= 30])
    assert INVALID_FILE in {g for g, _ in loop2} and all(c == 0 for c in codes.values())
    rc, dst, got, status, _ = many_read(ctx, dev, index, None, [r for r in rngs if r[0] >= 30], at=16 + 9)
    check_slots((which, "no tables"), rc, dst, got, [r for r in rngs if r[0] >= 30], loop2)


@pytest.mark.parametrize("which", [("BWT+RANK+ZRLT", "ANS0", 1024), "mixed"], ids=["bwt-1024", "mixed"])
def test_chunks_of_three_blocks_give_the_same_results(ctx, which, monkeypatch):
    m = case(ctx, which)
    dev, index, rngs, loop = reference(ctx, which)
    rc0, dst0, got0, status0, _ = many_read(ctx, dev, index, m["tables"], rngs)
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(sc.CHUNK))
    ctx.reload_switches()
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        rc, dst, got, status, _ = many_read(ctx, dev, index, m["tables"], rngs)
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
        monkeypatch.delenv("KZ_STREAM_CHUNK")
        ctx.reload_switches()
    check_slots((which, "chunk 3"), rc, dst, got, rngs, loop)
    assert (rc, got, status) == (rc0, got0, status0) and dst.tobytes() == dst0.tobytes()
    _, chunks, _ = sc.merged_plan([st.starts() for st in m["sts"]], sc.groups_of(m["headers"], rngs), rngs, sc.CHUNK)
    assert len(chunks) > 50
    assert times["k_knz_read"]["launches"] == len(chunks) == times["k_knz_unpack_many"]["launches"], (len(chunks), times.get("k_knz_read"))


# ---- isolation ---------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_no_range_names(ctx):
    """other bytes between the segments, and other bytes in every stream that no range names, header included"""
    which = ("BWT+RANK+ZRLT", "ANS0", 1024)
    m = case(ctx, which)
    _, index, _, _ = reference(ctx, which)
    skip = (0, 9, 17, 30)
    rngs = sc.call(m["sts"], skip=skip)
    a = many_read(ctx, Dev(m["streams"], fill=0xA5), index, m["tables"], rngs)
    other = [bytes([0xEE]) * len(s) if i in skip else s for i, s in enumerate(m["streams"])]
    b = many_read(ctx, Dev(other, fill=0x3C), index, m["tables"], rngs)
    assert a[0] == b[0] == sum(r[2] for r in rngs) and a[2] == b[2] and a[3] == b[3] == [0] * len(index)
    assert a[1].tobytes() == b[1].tobytes()
    check_slots("skip", a[0], a[1], a[2], rngs, sc.model_a(m["blocks"], m["bs"], rngs, m["tables"]))


def test_a_fault_of_one_stream_stays_with_that_stream(ctx):
    """an index entry that does not match, a table that is none, and a block whose header precheck fails: each gives its own ranges
    the single call's code, and every other slot is byte-equal to the undamaged call's"""
    which = ("BWT+RANK+ZRLT", "ANS0", 1024)
    m = case(ctx, which)
    dev0, index, rngs, loop = reference(ctx, which)
    rc0, dst0, got0, _, _ = many_read(ctx, dev0, index, m["tables"], rngs)
    A, B, C = 8, 31, 7                                                                   # bad entry, bad table, bad block
    bad_index = [list(ix) for ix in index]
    bad_index[A][2] = (index[A][2][0] + 1, index[A][2][1])
    bad_tables = list(m["tables"])
    bad_tables[B] = [1] + bad_tables[B][1:]
    streams = list(m["streams"])
    streams[C] = mc.block_header_fault(streams[C], index[C], 1, 0)
    dev = Dev(streams)
    want, codes = loop_read(ctx, dev, bad_index, bad_tables, rngs)
    assert codes[A] == INVALID_PARAM and codes[B] == INVALID_PARAM and codes[C] == 0
    assert any(g < 0 for (s, _, _), (g, _) in zip(rngs, want) if s == C) and any(g > 0 for (s, _, _), (g, _) in zip(rngs, want) if s == C)
    rc, dst, got, status, _ = many_read(ctx, dev, bad_index, bad_tables, rngs)
    assert "stream %d:" % C not in ctx.error() and "stream %d: index entry 2 does not match the stream" % A in ctx.error(), ctx.error()
    check_slots("faults", rc, dst, got, rngs, want)
    assert status == [codes.get(s, 0) for s in range(len(index))]
    at = 0
    for i, (s, o, n) in enumerate(rngs):
        if s not in (A, B, C):
            assert got[i] == got0[i] and dst[at:at + n].tobytes() == dst0[at:at + n].tobytes(), ("a neighbour's slot", i, (s, o, n))
        elif s in (A, B):
            assert got[i] == INVALID_PARAM and bool((dst[at:at + n] == 0xA5).all()), ("a failed stream's slot", i, (s, o, n))
        at += n


# ---- refusals and empties ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls(ctx):
    which = ("BWT+RANK+ZRLT", "ANS0", 1024)
    m = case(ctx, which)
    L = ctx.lib
    streams = m["streams"][6:9]
    dev = Dev(streams)
    _, index = assert_index_parity(ctx, "three", dev)
    first, off, w, _, _ = store_arrays(index, None)
    rngs = [(0, 5, 100), (2, 1000, 50), (1, 0, 0), (1, 3, 9)]
    total = 159
    rs, ro, rl = np.ascontiguousarray([r[0] for r in rngs], dtype=np.int32), i64([r[1] for r in rngs]), i64([r[2] for r in rngs])
    so, sl = i64(dev.off), i64(dev.len)
    got, status = np.full(4, SENT, dtype=np.int64), np.full(3, SENT, dtype=np.int32)
    tfirst, tab = i64([-1, 0, -1]), i64(knzread.starts(sc.block_lengths(3 * 1024, 1024)))
    fr = Frame(total, "a5", device=True, guard=GUARD)

    def good():
        return [ctx.h, dev.ptr, so.ctypes.data, sl.ctypes.data, 3, first.ctypes.data, off.ctypes.data, w.ctypes.data, None, None,
                rs.ctypes.data, ro.ctypes.data, rl.ctypes.data, 4, fr.ptr(), total, got.ctypes.data, status.ctypes.data]

    def call(**kw):
        args = good()
        names = ["ctx", "src", "so", "sl", "ns", "first", "off", "w", "tfirst", "tab", "rs", "ro", "rl", "nr", "dst", "cap", "got", "status"]
        for k, v in kw.items():
            args[names.index(k)] = v.ctypes.data if isinstance(v, np.ndarray) else v
        return L.kz_read_bytes_many_device(*args)

    for k in ("ctx", "src", "so", "sl", "first", "off", "w", "rs", "ro", "rl", "dst", "got"):
        assert call(**{k: None}) == INVALID_PARAM, k
    assert call(ns=-1) == INVALID_PARAM and call(nr=-1) == INVALID_PARAM and call(cap=-1) == INVALID_PARAM
    assert call(tfirst=tfirst) == INVALID_PARAM                                          # a table is named and blockByteOff is null
    assert call(tfirst=i64([-1, -2, -1]), tab=tab) == INVALID_PARAM
    for bad in ([0, 3, 1, 1], [0, -1, 1, 1]):
        assert call(rs=np.ascontiguousarray(bad, dtype=np.int32)) == INVALID_PARAM, bad
    dec = first.copy()
    dec[1], dec[2] = first[2], first[1]
    assert first[1] < first[2] and call(first=dec) == INVALID_PARAM                      # an indexFirst that descends
    neg = first.copy()
    neg[0] = -1
    assert call(first=neg) == INVALID_PARAM
    for name, arr in (("so", so), ("sl", sl), ("ro", ro), ("rl", rl)):
        bad = arr.copy()
        bad[1] = -1
        assert call(**{name: bad}) == INVALID_PARAM, name
    assert call(cap=total - 1) == WRITE_FILE and "destination too small" in ctx.error()
    assert fr.untouched() and list(got) == [SENT] * 4 and list(status) == [SENT] * 3     # decided before anything is written
    assert call(nr=0) == 0 and call(nr=0, rs=None, ro=None, rl=None, dst=None, got=None, status=None) == 0
    assert L.kz_read_bytes_many_device(ctx.h, None, None, None, 0, None, None, None, None, None, None, None, None, 0, None, 0, None, None) == 0
    assert fr.untouched()
    assert call() == total and list(got) == [100, 50, 0, 9] and list(status) == [0, 0, 0]
    assert call(tfirst=tfirst, tab=tab) == total and list(got) == [100, 50, 0, 9]
    assert call(status=None) == total
    # the index call
    hdr = [None] * 5
    st, fi = np.full(3, SENT, dtype=np.int32), np.full(4, SENT, dtype=np.int64)
    eo, eb = np.full(16, SENT, dtype=np.int64), np.full(16, SENT, dtype=np.int64)

    def idx(ctxh=ctx.h, src=dev.ptr, so_=so, sl_=sl, ns=3, st_=st, fi_=fi, eo_=eo, eb_=eb, cap=16):
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.kz_knz_index_many_device(ctxh, src, ptr(so_), ptr(sl_), ns, *hdr, ptr(st_), ptr(fi_), ptr(eo_), ptr(eb_), cap)

    assert idx(ns=0) == 0 and L.kz_knz_index_many_device(ctx.h, None, None, None, 0, *hdr, None, None, None, None, 0) == 0
    assert list(st) == [SENT] * 3 and list(fi) == [SENT] * 4 and list(eo) == [SENT] * 16   # nStreams == 0 touches nothing
    assert idx(ctxh=None) == INVALID_PARAM and idx(ns=-1) == INVALID_PARAM and idx(cap=-1) == INVALID_PARAM
    for k in ("src", "so_", "sl_", "st_", "fi_", "eo_", "eb_"):
        assert idx(**{k: None}) == INVALID_PARAM, k
    for k, arr in (("so_", so), ("sl_", sl)):
        bad = arr.copy()
        bad[2] = -1
        assert idx(**{k: bad}) == INVALID_PARAM, k
    assert list(st) == [SENT] * 3
    assert idx() == 2 + 3 + 4 and list(st) == [2, 3, 4] and list(fi) == [0, 2, 5, 9] and list(eo[9:]) == [SENT] * 7   # all header out-pointers null


# ---- launches ----------------------------------------------------------------------------------------------------------------------------
COUNTED = ("k_knz_heads", "k_knz_check_rows", "k_knz_unpack_many", "k_knz_read")


def _counted(ctx, dev, index, rngs):
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        rc, dst, got, status, _ = many_read(ctx, dev, index, None, rngs)
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    assert rc == sum(r[2] for r in rngs) and all(g >= 0 for g in got)
    assert "k_knz_unpack" not in times and "k_knz_check" not in times and "k_knz_walk" not in times and "k_knz_scatter" not in times, sorted(times)
    return {k: times.get(k, {}).get("launches", 0) for k in COUNTED}, dst, got                   # (kernel_times reads kz_get_kernel_launches)


def test_launches_do_not_grow_with_the_streams(ctx, monkeypatch):
    """thirty streams cost the launches of one stream that holds as many touched blocks, and sixty streams of half the ranges each
    cost what the thirty do"""
    chain, ent, bs = which = ("BWT+RANK+ZRLT", "ANS0", 1024)
    m = case(ctx, which)
    _, index, _, _ = reference(ctx, which)
    thirty = list(range(30))
    rngs = sc.call(m["sts"], only=thirty)
    touched = sum(len(m["sts"][s].lens) for s in thirty)
    assert touched == 165
    # one stream of 165 blocks, every block touched
    data = np.ascontiguousarray(np.tile(mc.data_for(chain, bs), 5)[:touched * bs - 7])
    cap = kz.compress_bound(len(data), bs)
    one = np.empty(cap, dtype=np.uint8)
    n = ctx.lib.kz_compress(ctx.h, kz.transform_type(chain), kz.ENTROPY_IDS[ent], bs, data.ctypes.data, len(data), one.ctypes.data, cap)
    assert n > 0
    one = one[:n].tobytes()
    one_index = [kz.knz_index(one)["blocks"]]
    assert len(one_index[0]) == touched
    one_rngs = [(0, k * bs + 1, 5) for k in range(touched)] + [(0, 3 * bs - 2, 2 * bs)]
    dev30, dev1 = Dev(m["streams"][:30]), Dev([one])
    # sixty streams: every stream twice, its ranges dealt out to the two copies in turn
    turn, rngs60 = {}, []
    for s, o, z in rngs:
        turn[s] = turn.get(s, 0) + 1
        rngs60.append((s + 30 * (turn[s] % 2), o, z))
    dev60 = Dev(m["streams"][:30] + m["streams"][:30])
    for chunk in (None, 64):
        if chunk:
            monkeypatch.setenv("KZ_STREAM_CHUNK", str(chunk))
            ctx.reload_switches()
        a, dst30, got30 = _counted(ctx, dev30, index[:30], rngs)
        b, dst1, _ = _counted(ctx, dev1, one_index, one_rngs)
        nchunks = -(-touched // chunk) if chunk else 1
        assert a == b == {"k_knz_heads": 1, "k_knz_check_rows": 1, "k_knz_unpack_many": nchunks, "k_knz_read": nchunks}, (chunk, a, b)
        assert dst1[:5].tobytes() == data[1:6].tobytes() and dst1[-2 * bs:].tobytes() == data[3 * bs - 2:5 * bs - 2].tobytes()
        if not chunk:
            c, dst60, got60 = _counted(ctx, dev60, index[:30] + index[:30], rngs60)
            assert c == a, (c, a)
            assert got60 == got30 and dst60.tobytes() == dst30.tobytes()
    monkeypatch.delenv("KZ_STREAM_CHUNK")
    ctx.reload_switches()


# ---- the Python store -------------------------------------------------------------------------------------------------------------------
def test_knz_store(ctx):
    import torch
    which = ("BWT+RANK+ZRLT", "ANS0", 1024)
    m = case(ctx, which)
    store = kz.KnzStore.from_compress_many(ctx, m["dst"], m["doff"], m["sizes"])
    assert len(store) == 30 and store.status == [len(st.lens) for st in m["sts"][:30]]
    assert [ix["blocks"] for ix in store.index] == [kz.knz_index(s)["blocks"] for s in m["streams"][:30]]
    assert all(ix["blockSize"] == 1024 and ix["inputSize"] == len(b) for ix, b in zip(store.index, m["bufs"]))
    rngs = [r for r in sc.call(m["sts"], only=range(30)) if r[1] < (1 << 40)]
    packed, got = store.read_many([r[0] for r in rngs], [r[1] for r in rngs], [r[2] for r in rngs])
    assert packed.is_cuda and packed.dtype == torch.uint8 and packed.numel() == sum(r[2] for r in rngs)
    h, at = packed.cpu().numpy(), 0
    for (s, o, n), g in zip(rngs, got):
        want = m["bufs"][s][o:o + n].tobytes()
        assert g == len(want) and h[at:at + g].tobytes() == want, (s, o, n)
        at += n
    out = torch.full((at + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    packed2, got2 = store.read_many([r[0] for r in rngs], [r[1] for r in rngs], [r[2] for r in rngs], out=out)
    assert got2 == got and packed2.data_ptr() == out.data_ptr() and bool((out[at:] == 0xA5).all())
    one = store.read(9, 5 * 1024 - 3, 10)
    assert one.cpu().numpy().tobytes() == m["bufs"][9][5 * 1024 - 3:5 * 1024 + 7].tobytes()
    assert store.read(9, len(m["bufs"][9]) - 4, 100).numel() == 4 and store.read(0, 0, 10).numel() == 0
    assert store.read_many([], [], [])[1] == []
    with pytest.raises(ValueError):
        store.read_many([0], [-1], [4])
    with pytest.raises(IndexError):
        store.read_many([30], [0], [4])
    # with tables: the two joined streams appended behind the thirty
    n = len(m["streams"])
    dev = Dev(m["streams"])
    store = kz.KnzStore(ctx, dev.t, dev.off, dev.len, byte_offsets=m["tables"])
    data = [b"".join(bl) for bl in m["blocks"]]
    rngs = [r for r in sc.call(m["sts"]) if r[1] < (1 << 40)]
    packed, got = store.read_many([r[0] for r in rngs], [r[1] for r in rngs], [r[2] for r in rngs])
    h, at = packed.cpu().numpy(), 0
    for (s, o, z), g in zip(rngs, got):
        assert h[at:at + g].tobytes() == data[s][o:o + z], (s, o, z)
        at += z
    assert len(store) == n
    with pytest.raises(kz.KanziError) as e:
        kz.KnzStore(ctx, dev.t, dev.off, dev.len).read(30, 1024, 10)                      # a short middle block, no table
    assert e.value.code == 15
