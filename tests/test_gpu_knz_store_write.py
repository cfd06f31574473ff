"""The many-stream write (kz_write_bytes_many_device) against the single-stream call it restates: kz_write_bytes_device on each
stream alone, with that stream's ranges in their call order, is the reference throughout and never the code under test.  The case
set is tests/storewritecases.py: fifteen streams of 1 KiB blocks, two of them joined ones with tables, packed into one buffer at
every residue mod 16; the ranges of all streams interleaved; the destination poisoned, its slots at odd offsets so that neighbours
share 16-byte units; KZ_STREAM_CHUNK = 3 cuts every header group."""
import numpy as np
import pytest

import kanzi_amd as kz
import knzwrite
import manycases as mc
import storecases as sc
import storewritecases as wc

pytestmark = pytest.mark.gpu

INVALID_PARAM, WRITE_FILE = -18, -12
POISON = wc.POISON
SENT = -777                        # what dstLen[] and the new index hold before a call
BS = wc.BS


def _p(a):
    return None if a is None or len(a) == 0 else a.ctypes.data


def i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


# ---- the streams, built once by the library -------------------------------------------------------------------------------------------
_MADE = {}


def _compress(ctx, chain, ent, bufs):
    """kz_compress_many_device over the buffers -> their .knz bytes"""
    import torch
    src, soff = mc.pack(bufs)
    t = torch.from_numpy(src).cuda()
    caps = [kz.compress_bound(len(b), BS) for b in bufs]
    doff, payload = mc.slots(caps)
    dst = torch.full((payload + 64,), POISON, dtype=torch.uint8, device="cuda")
    sizes = kz.compress_many_device(ctx, chain, ent, BS, t.data_ptr(), soff, [len(b) for b in bufs], dst.data_ptr(), doff, caps)
    assert all(n > 0 for n in sizes), sizes
    h = dst.cpu().numpy()
    return [h[o:o + n].tobytes() for o, n in zip(doff, sizes)]


def _compressed(ctx, chain, ent):
    """the streams of LENGTHS (and the one of seven blocks) under one chain -> (.knz bytes, input bytes) per stream"""
    key = (chain, ent)
    if key not in _MADE:
        d = mc.data_for(chain, BS)
        lens = wc.LENGTHS + [7 * BS]
        bufs = [np.ascontiguousarray(d[(i * BS) % (len(d) - n):][:n]) for i, n in enumerate(lens)]
        _MADE[key] = (_compress(ctx, chain, ent, bufs), [b.tobytes() for b in bufs])
    return _MADE[key]


def made(ctx, four):
    """-> dict(sts, streams: .knz bytes, data: the original bytes, tables, index) of the call's fifteen streams"""
    key = ("call", four)
    if key in _MADE:
        return _MADE[key]
    sts = wc.streams()
    streams, data = [], []
    for s, st in enumerate(sts):
        knz, raw = _compressed(ctx, *wc.chain_of(s, four))
        if st.parts is None:
            j = s if s < 12 else 12
            streams.append(knz[j])
            data.append(raw[j])
        else:
            pieces, isz = kz.splice_concat([kz.knz_index(knz[p]) for p in st.parts])
            streams.append(kz.knz_splice([knz[p] for p in st.parts], pieces, isz))
            data.append(b"".join(raw[p] for p in st.parts))
        assert len(data[-1]) == st.n
    index = [kz.knz_index(k)["blocks"] for k in streams]
    assert [len(ix) for ix in index] == [len(st.lens) for st in sts]
    _MADE[key] = dict(sts=sts, streams=streams, data=data, tables=[st.table for st in sts], index=index)
    return _MADE[key]


class Dev:
    """the streams in one device buffer, as manycases.pack lays them out: every residue mod 16, poison between and behind them"""

    def __init__(self, streams):
        import torch
        buf, self.off = mc.pack(streams, fill=POISON)
        self.len = [len(s) for s in streams]
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr()


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


def slot_caps(index):
    caps = [kz.write_bytes_bound([w for _, w in ix], BS) for ix in index]
    return [c + (c & 1) for c in caps]                                                   # even: every slot starts at an odd offset


def many_write(ctx, dev, index, tables, rngs, new, caps, lead=mc.SLOT_LEAD, want_index=True):
    """-> (rc, dstLen, the destination buffer, slot offsets, newBitOff, newBits, indexFirst)"""
    import torch
    first, off, w, tfirst, tab = store_arrays(index, tables)
    rs, ro, rl = np.ascontiguousarray([r[0] for r in rngs], dtype=np.int32), i64([r[1] for r in rngs]), i64([r[2] for r in rngs])
    data = torch.from_numpy(np.frombuffer(b"\0" + bytes(new) + b"\0" * 3, dtype=np.uint8).copy()).cuda()      # the new bytes at an odd address
    doff, payload = mc.slots(caps, lead=lead)
    dst = torch.full((payload + 64,), POISON, dtype=torch.uint8, device="cuda")
    dl = np.full(max(len(index), 1), SENT, dtype=np.int64)
    nbo, nbw = np.full(max(len(off), 1), SENT, dtype=np.int64), np.full(max(len(off), 1), SENT, dtype=np.int64)
    so, sl, do, dc = i64(dev.off), i64(dev.len), i64(doff), i64(caps)
    torch.cuda.synchronize()
    rc = ctx.lib.kz_write_bytes_many_device(ctx.h, dev.ptr, _p(so), _p(sl), len(dev.off), first.ctypes.data, _p(off), _p(w),
                                            None if tfirst is None else tfirst.ctypes.data, _p(tab), _p(rs), _p(ro), _p(rl), len(rngs),
                                            data.data_ptr() + 1, len(new), dst.data_ptr(), _p(do), _p(dc), dl.ctypes.data,
                                            nbo.ctypes.data if want_index else None, nbw.ctypes.data if want_index else None)
    return rc, [int(x) for x in dl[:len(index)]], dst.cpu().numpy(), doff, nbo, nbw, first


def single_write(ctx, dev, s, ix, table, mine, new, cap):
    """kz_write_bytes_device on stream s alone -> (rc, the new stream's bytes or None, new index or None)"""
    import torch
    off, w = i64([e[0] for e in ix]), i64([e[1] for e in ix])
    tab = None if table is None else i64(table)
    ro, rl = i64([r[0] for r in mine]), i64([r[1] for r in mine])
    data = torch.from_numpy(np.frombuffer(bytes(new) + b"\0", dtype=np.uint8).copy()).cuda()
    dst = torch.full((cap + 16,), POISON, dtype=torch.uint8, device="cuda")
    nbo, nbw = np.full(max(len(ix), 1), SENT, dtype=np.int64), np.full(max(len(ix), 1), SENT, dtype=np.int64)
    torch.cuda.synchronize()
    rc = ctx.lib.kz_write_bytes_device(ctx.h, dev.ptr + dev.off[s], dev.len[s], _p(off), _p(w), _p(tab), len(ix), _p(ro), _p(rl), len(mine),
                                       data.data_ptr(), len(new), dst.data_ptr(), cap, nbo.ctypes.data, nbw.ctypes.data)
    if rc < 0:
        return rc, None, None
    return rc, dst[:rc].cpu().numpy().tobytes(), list(zip(nbo[:len(ix)].tolist(), nbw[:len(ix)].tolist()))


def assert_parity(ctx, tag, dev, index, tables, rngs, pay, caps, res=None):
    """the many call against the loop of single calls -> (dstLen, {stream: new stream bytes})"""
    new = b"".join(pay)
    res = many_write(ctx, dev, index, tables, rngs, new, caps) if res is None else res
    rc, dl, dst, doff, nbo, nbw, first = res
    assert rc == 0, (tag, rc, ctx.error())
    named = sorted({r[0] for r in rngs})
    out = {}
    for s in range(len(index)):
        a, b = int(first[s]), int(first[s + 1])
        slot = dst[doff[s]:doff[s] + caps[s]]
        if s not in named:
            assert dl[s] == 0 and bool((slot == POISON).all()), (tag, s, "an unnamed stream")
            assert bool((nbo[a:b] == SENT).all()) and bool((nbw[a:b] == SENT).all()), (tag, s)
            continue
        mine, idx = sc.of_stream(rngs, s)
        rc1, want, want_index = single_write(ctx, dev, s, index[s], None if tables is None else tables[s], mine, b"".join(pay[i] for i in idx), caps[s])
        assert dl[s] == rc1, (tag, s, "dstLen", dl[s], rc1, ctx.error())
        if rc1 < 0:
            continue
        assert slot[:rc1].tobytes() == want, (tag, s, "the slot's bytes")
        assert list(zip(nbo[a:b].tolist(), nbw[a:b].tolist())) == want_index, (tag, s, "the new index")
        out[s] = want
    outside = mc.outside_slots(len(dst), doff, caps)
    assert bool((dst[outside] == POISON).all()), (tag, "a byte outside the slots was written")
    return dl, out


def decode_many(ctx, streams):
    """kz_decompress_many_device over the new streams -> their data"""
    import torch
    buf, off = mc.pack(streams, fill=POISON)
    t = torch.from_numpy(buf).cuda()
    caps = [kz.knz_index(k)["inputSize"] + 16 for k in streams]
    doff, payload = mc.slots(caps)
    dst = torch.zeros(payload + 64, dtype=torch.uint8, device="cuda")
    sizes = kz.decompress_many_device(ctx, t.data_ptr(), off, [len(k) for k in streams], dst.data_ptr(), doff, caps)
    h = dst.cpu().numpy()
    return [h[o:o + n].tobytes() if n >= 0 else n for o, n in zip(doff, sizes)]


@pytest.fixture
def chunked(ctx, monkeypatch):
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(wc.CHUNK))
    ctx.reload_switches()
    yield
    monkeypatch.delenv("KZ_STREAM_CHUNK")
    monkeypatch.delenv("KZ_WRITE_GATHER", raising=False)
    ctx.reload_switches()


PARITY = [(False, True, False), (False, False, False), (True, True, False), (True, False, False), (True, True, True)]


@pytest.mark.parametrize("four,tables,gather", PARITY, ids=["%s-%s%s" % ("four" if f else "one", "tables" if t else "notables", "-gather" if g else "") for f, t, g in PARITY])
def test_every_named_stream_equals_its_single_call(ctx, chunked, monkeypatch, four, tables, gather):
    if gather:
        monkeypatch.setenv("KZ_WRITE_GATHER", "1")
        ctx.reload_switches()
    m = made(ctx, four)
    sts = m["sts"]
    rngs = wc.call(sts)
    pay = wc.payloads(rngs)
    dev = Dev(m["streams"])
    caps = slot_caps(m["index"])
    tag = (four, tables, gather)
    dl, new = assert_parity(ctx, tag, dev, m["index"], m["tables"] if tables else None, rngs, pay, caps)
    assert dl[wc.UNNAMED] == 0
    D = wc.data_places(rngs)
    joined = b"".join(pay)
    if tables:
        assert sorted(new) == sorted({r[0] for r in rngs}), (tag, dl)
    else:                                                                                # a short middle block and no table: the single call's refusal
        assert sorted(set(r[0] for r in rngs) - set(new)) == [12, 13] and dl[12] < 0 and dl[13] < 0, (tag, dl)
    ids = sorted(new)
    back = decode_many(ctx, [new[s] for s in ids])
    for s, got in zip(ids, back):
        mine, idx = sc.of_stream(rngs, s)
        assert got == knzwrite.apply(m["data"][s], mine, [joined[D[i]:D[i + 1]] for i in idx]), (tag, s, "the decoded new stream")
    if not four:                                                                         # NONE&NONE: the layout the CPU tests count on is the real one
        group = sc.groups_of([wc.chain_of(s, four) for s in range(len(sts))], rngs)
        P = wc.merged_plan(sts, rngs, group, wc.CHUNK, use=ids)
        _, sizes = wc.none_layout(P, sts, wc.CHUNK)
        assert {s: dl[s] for s in ids} == sizes
        assert all(m["index"][s] and [w for _, w in m["index"][s]] == [wc.none_bits(l) for l in sts[s].lens] for s in ids if sts[s].lens)


def test_slots_that_end_where_their_streams_end(ctx, chunked):
    """the NONE&NONE call into slots of exactly the new streams' sizes (rounded up to even), gaps of 0, 2 and 38 bytes between them:
    neighbouring spans of one launch share 16-byte units, and not a byte between the slots is written"""
    m = made(ctx, False)
    sts = m["sts"]
    rngs = wc.call(sts)
    group = sc.groups_of([wc.chain_of(s, False) for s in range(len(sts))], rngs)
    _, sizes = wc.none_layout(wc.merged_plan(sts, rngs, group, wc.CHUNK), sts, wc.CHUNK)
    caps = wc.tight_caps(sizes, len(sts))
    dl, new = assert_parity(ctx, "tight", Dev(m["streams"]), m["index"], m["tables"], rngs, wc.payloads(rngs), caps)
    assert {s: dl[s] for s in sizes} == sizes and all(0 <= caps[s] - dl[s] <= 1 for s in sizes)


# ---- faults stay with their stream ------------------------------------------------------------------------------------------------------
def _small(ctx):
    import torch
    if "small" not in _MADE:
        data = mc.small_input()
        t = torch.from_numpy(data.copy()).cuda()
        cap = kz.compress_bound(len(data), mc.SMALL_BS)
        dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        n = kz.compress_device(ctx, *mc.SMALL_CHAIN, mc.SMALL_BS, t.data_ptr(), len(data), dst.data_ptr(), cap)
        knz = dst[:n].cpu().numpy().tobytes()
        _MADE["small"] = (knz, kz.knz_index(knz)["blocks"], data.tobytes())
    return _MADE["small"]


SMALL_RANGES = [(0, 5, 7), (1, 1030, 20), (2, 2040, 16), (1, 1040, 3), (0, 3071, 1), (2, 0, 0), (1, 100, 4)]   # stream 1's ranges: numbers 1, 3 and 6 of the call
FAULTS = ["header", "table", "behind", "entry", "block", "slot"]


@pytest.mark.parametrize("what", FAULTS)
def test_a_fault_stays_with_its_stream(ctx, chunked, what):
    knz, blocks, data = _small(ctx)
    assert len(blocks) == 3
    streams, index, tables = [knz, knz, knz], [list(blocks), list(blocks), list(blocks)], [None, None, None]
    rngs = list(SMALL_RANGES)
    caps = slot_caps(index)
    text = None
    if what == "header":
        bad = bytearray(knz)
        bad[0] ^= 0x40
        streams[1] = bytes(bad)
    elif what == "table":
        tables = [None, [0, 1024, 1000, 3072], None]
        text = "blockByteOff is not a table of block starts"
    elif what == "behind":
        rngs[3] = (1, 3070, 3)
        text = "range 3 ends behind the data"
    elif what == "entry":
        index[1][1] = (blocks[1][0] + 1, blocks[1][1])
        text = "index entry 1 does not match the stream"
    elif what == "block":
        streams[1] = mc.block_header_fault(knz, blocks, k=1)
        text = "block 1:"
    elif what == "slot":
        good = single_write(ctx, Dev(streams), 1, index[1], None, [r[1:] for r in rngs if r[0] == 1], b"".join(p for p, r in zip(wc.payloads(rngs), rngs) if r[0] == 1), caps[1])
        assert good[0] > 0
        caps[1] = good[0] - 1
        text = "destination too small"
    pay = wc.payloads(rngs)
    dev = Dev(streams)
    dl, new = assert_parity(ctx, what, dev, index, tables, rngs, pay, caps)              # the failing stream's dstLen is the single call's code; nothing outside the slots
    assert dl[1] < 0 and dl[0] > 0 and dl[2] > 0, (what, dl)
    if what in ("table", "behind", "entry"):
        assert dl[1] == INVALID_PARAM
    if what == "slot":
        assert dl[1] == WRITE_FILE
    many_write(ctx, dev, index, tables, rngs, b"".join(pay), caps)
    assert "stream 1:" in ctx.error() and (text is None or text in ctx.error()), ctx.error()
    # every other stream comes out as if the failing one were not in the call
    keep = [i for i, r in enumerate(rngs) if r[0] != 1]
    alone = [(0 if rngs[i][0] == 0 else 1, rngs[i][1], rngs[i][2]) for i in keep]
    dev2 = Dev([knz, knz])
    dl2, new2 = assert_parity(ctx, what + " without", dev2, [list(blocks), list(blocks)], None, alone, [pay[i] for i in keep], [caps[0], caps[2]])
    assert [new2[0], new2[1]] == [new[0], new[2]] and [dl2[0], dl2[1]] == [dl[0], dl[2]]


def test_a_damaged_block_that_is_wholly_overwritten_with_a_table_is_repaired(ctx, chunked):
    knz, blocks, data = _small(ctx)
    bad = mc.block_header_fault(knz, blocks, k=1)
    table = [0, 1024, 2048, 3072]
    rngs = [(0, 3, 4), (1, 1024, 1000), (1, 2000, 48), (0, 1024, 1024)]
    pay = wc.payloads(rngs)
    dev = Dev([knz, bad])
    index = [list(blocks), list(blocks)]
    dl, new = assert_parity(ctx, "repair", dev, index, [table, table], rngs, pay, slot_caps(index))
    assert dl[0] > 0 and dl[1] > 0
    back = decode_many(ctx, [new[0], new[1]])
    assert back[1] == data[:1024] + pay[1][:976] + pay[2] + data[2048:]
    assert back[0] == knzwrite.apply(data, [(3, 4), (1024, 1024)], [pay[0], pay[3]])
    # without the table the block is decoded, and its damage fails its stream alone
    dl, new = assert_parity(ctx, "no repair", dev, index, None, rngs, pay, slot_caps(index))
    assert dl[0] > 0 and dl[1] < 0


# ---- faults of the call itself -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_destination_untouched(ctx):
    import torch
    knz, blocks, data = _small(ctx)
    dev = Dev([knz, knz])
    n = len(blocks)
    first, off, w = i64([0, n, 2 * n]), i64([b[0] for b in blocks] * 2), i64([b[1] for b in blocks] * 2)
    so, sl = i64(dev.off), i64(dev.len)
    caps = i64(slot_caps([blocks, blocks]))
    doff = i64(mc.slots(caps.tolist())[0])
    dst = torch.full((int(doff[-1] + caps[-1]) + 64,), POISON, dtype=torch.uint8, device="cuda")
    new = torch.zeros(64, dtype=torch.uint8, device="cuda")
    good = dict(src=dev.ptr, so=so, sl=sl, ns=2, first=first, off=off, w=w, tfirst=None, tab=None, rs=np.asarray([0, 1], dtype=np.int32), ro=i64([5, 9]),
                rl=i64([7, 3]), nr=2, data=new.data_ptr(), dlen=10, dst=dst.data_ptr(), doff=doff, caps=caps, dl=np.full(2, SENT, dtype=np.int64),
                nbo=np.full(2 * n, SENT, dtype=np.int64), nbw=np.full(2 * n, SENT, dtype=np.int64))

    def call(**kw):
        a = dict(good, **kw)
        good["dl"][:] = SENT
        ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
        return ctx.lib.kz_write_bytes_many_device(ctx.h, a["src"], ptr(a["so"]), ptr(a["sl"]), a["ns"], ptr(a["first"]), ptr(a["off"]), ptr(a["w"]), ptr(a["tfirst"]),
                                                  ptr(a["tab"]), ptr(a["rs"]), ptr(a["ro"]), ptr(a["rl"]), a["nr"], a["data"], a["dlen"], a["dst"], ptr(a["doff"]),
                                                  ptr(a["caps"]), ptr(a["dl"]), ptr(a["nbo"]), ptr(a["nbw"]))

    bad = [dict(src=None), dict(so=None), dict(sl=None), dict(first=None), dict(off=None), dict(rs=None), dict(ro=None), dict(rl=None), dict(data=None),
           dict(dst=None), dict(doff=None), dict(caps=None), dict(dl=None), dict(ns=-1), dict(nr=-1), dict(dlen=-1),
           dict(so=i64([-1, 5])), dict(sl=i64([-1, 5])), dict(ro=i64([-5, 9])), dict(rl=i64([-7, 3])), dict(caps=i64([-1, 100])), dict(doff=i64([-3, 100])),
           dict(rs=np.asarray([0, 2], dtype=np.int32)), dict(rs=np.asarray([-1, 1], dtype=np.int32)), dict(first=i64([0, n, n - 1])),
           dict(tfirst=i64([-2, -1]), tab=i64([0])), dict(tfirst=i64([0, -1]), tab=None), dict(dlen=11), dict(dlen=9), dict(nbo=None), dict(nbw=None)]
    for kw in bad:
        assert call(**kw) == INVALID_PARAM, kw
    assert bool((dst == POISON).all()), "a refused call wrote to the destination"
    assert list(good["dl"]) == [SENT, SENT] and bool((good["nbo"] == SENT).all())
    # no ranges: 0, every dstLen 0, nothing else touched
    assert call(nr=0, dlen=0, rs=None, ro=None, rl=None, data=None) == 0
    assert list(good["dl"]) == [0, 0] and bool((dst == POISON).all()) and bool((good["nbo"] == SENT).all())
    assert call(nbo=None, nbw=None) == 0 and all(x > 0 for x in good["dl"])                # both NULL: no new index is asked for
    assert call() == 0 and all(x > 0 for x in good["dl"]) and bool((good["nbo"] > 0).all())


# ---- the Python store --------------------------------------------------------------------------------------------------------------------
def test_knz_store_write_many(ctx, chunked):
    import torch
    m = made(ctx, True)
    sts = m["sts"]
    dev = Dev(m["streams"])
    before = dev.t.clone()
    store = kz.KnzStore(ctx, dev.t, dev.off, dev.len, byte_offsets=m["tables"])
    rngs = wc.call(sts)
    pay = wc.payloads(rngs)
    new = store.write_many([r[0] for r in rngs], [r[1] for r in rngs], pay)
    assert isinstance(new, kz.KnzStore) and new is not store and len(new) == len(store) and new.byte_offsets == store.byte_offsets
    assert new.src.data_ptr() != store.src.data_ptr() and bool((dev.t == before).all())
    D = wc.data_places(rngs)
    joined = b"".join(pay)
    want = []
    for s in range(len(sts)):
        mine, idx = sc.of_stream(rngs, s)
        want.append(knzwrite.apply(m["data"][s], mine, [joined[D[i]:D[i + 1]] for i in idx]))
    ask = [(s, 0, sts[s].n) for s in range(len(sts))]
    for st, data in ((new, want), (store, m["data"])):                                   # the old store still reads the old bytes
        packed, got = st.read_many([a[0] for a in ask], [a[1] for a in ask], [a[2] for a in ask])
        h, at = packed.cpu().numpy(), 0
        for (s, _, n), g in zip(ask, got):
            assert g == n and h[at:at + n].tobytes() == data[s], s
            at += n
    u = wc.UNNAMED                                                                       # an unnamed stream is bit-identical
    assert new.src_len[u] == dev.len[u] and new.src[new.src_off[u]:new.src_off[u] + new.src_len[u]].cpu().numpy().tobytes() == m["streams"][u]
    one = store.write(4, 3 * BS + 5, b"record")
    assert one.read(4, 3 * BS + 3, 10).cpu().numpy().tobytes() == m["data"][4][3 * BS + 3:3 * BS + 5] + b"record" + m["data"][4][3 * BS + 11:3 * BS + 13]
    assert one.src_len[:4] + one.src_len[5:] == store.src_len[:4] + store.src_len[5:]
    with pytest.raises(kz.KanziError):
        store.write(4, sts[4].n - 2, b"abc")                                             # behind the data: that stream's fault
    with pytest.raises(IndexError):
        store.write(len(sts), 0, b"a")
    with pytest.raises(ValueError):
        store.write(0, -1, b"a")


# ---- launches ----------------------------------------------------------------------------------------------------------------------------
KNZ = ("k_knz_heads", "k_knz_check_rows", "k_knz_check", "k_knz_unpack_many", "k_knz_unpack", "k_knz_write", "k_knz_splice_many", "k_knz_splice")


def _counted(ctx, fn):
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        out = fn()
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    return out, {k: v["launches"] for k, v in times.items()}


def test_launches_do_not_grow_with_the_streams(ctx):
    """N streams of one header whose touched blocks fit one chunk cost the decode, encode and emit launches of one single-stream call
    over a stream with as many touched blocks; the expected counts are that call's, made here"""
    chain, ent = mc.CHAINS[2]
    blk = mc.data_for(chain, BS)[:BS]                                                    # every block the same bytes, so that both calls code the same blocks
    streams = _compress(ctx, chain, ent, [np.tile(blk, 3)] * 4 + [np.tile(blk, 9)])
    index = [kz.knz_index(k)["blocks"] for k in streams]
    rngs = [(i, BS + 9, 33) for i in range(4)]                                            # four streams, one touched block each
    pay = [knzwrite.payload(1, 33)] * 4
    dev = Dev(streams)
    caps = slot_caps(index)
    res, many = _counted(ctx, lambda: many_write(ctx, dev, index, None, rngs, b"".join(pay), caps))
    dl, _ = assert_parity(ctx, "launches", dev, index, None, rngs, pay, caps, res=res)
    assert all(x > 0 for x in dl[:4]) and dl[4] == 0
    # one stream of nine blocks, four of them touched
    one_rngs = [((2 * k + 1) * BS + 9, 33) for k in range(4)]
    (rc, _, _), single = _counted(ctx, lambda: single_write(ctx, dev, 4, index[4], None, one_rngs, b"".join(pay), caps[4]))
    assert rc > 0
    codec = lambda t: {k: v for k, v in t.items() if not k.startswith("k_knz_")}
    assert codec(many) == codec(single) and codec(many), (many, single)                  # the batched decode and encode: kernel by kernel
    assert many.get("k_knz_unpack_many") == single.get("k_knz_unpack") == 1 and many.get("k_knz_write") == single.get("k_knz_write") == 1
    assert many.get("k_knz_heads") == 1 and many.get("k_knz_check_rows") == single.get("k_knz_check") == 1
    # the emit: the single call copies up to its last touched block and then its tail (two launches); here both ride in one
    assert 1 == many.get("k_knz_splice_many") <= single.get("k_knz_splice") and "k_knz_splice" not in many and "k_knz_splice_many" not in single
    assert set(many) - set(codec(many)) <= set(KNZ)
