"""Many .knz streams in one call (kz_compress_many_device / kz_decompress_many_device) against the single-stream calls they
restate: kz_compress_device / kz_decompress_device on each segment alone are the reference throughout and never the code under
test.  The case set is tests/manycases.py: segments at every residue mod 16 in one source buffer, slots at odd offsets with poison
between them and guards around them."""
import numpy as np
import pytest

import kanzi_amd as kz
import datagen
import manycases as mc
from layouthelp import Frame

pytestmark = pytest.mark.gpu

GUARD = 4096


def up(a, lead=1):
    """bytes / array -> (tensor that owns the memory, device address `lead` bytes into it): an odd address by default"""
    import torch
    a = np.frombuffer(bytes(a), dtype=np.uint8) if not isinstance(a, np.ndarray) else a
    buf = np.zeros(lead + max(len(a), 1), dtype=np.uint8)
    buf[lead:lead + len(a)] = a
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + lead


# ---- the reference: one stream, one call ---------------------------------------------------------------------------------------
def single_compress(ctx, chain, ent, bs, data, cap=None, checksum=0, skip=False):
    """kz_compress_device on the buffer alone -> (rc, the stream)"""
    t, p = up(data)
    cap = kz.compress_bound(len(data), bs) if cap is None else cap
    fr = Frame(3 + cap, "a5", device=True, guard=GUARD)
    ctx.set_checksum(checksum)
    ctx.set_skip_blocks(skip)
    try:
        rc = ctx.lib.kz_compress_device(ctx.h, kz.transform_type(chain), kz.ENTROPY_IDS[ent], bs, p, len(data), fr.ptr(3), cap)
    finally:
        ctx.set_checksum(0)
        ctx.set_skip_blocks(False)
    a = fr.after()
    return rc, a[GUARD + 3:GUARD + 3 + max(rc, 0)].tobytes()


def single_decompress(ctx, knz, cap):
    """kz_decompress_device on the stream alone -> (rc, dst[0 .. cap))"""
    t, p = up(knz)
    fr = Frame(3 + cap, "a5", device=True, guard=GUARD)
    rc = ctx.lib.kz_decompress_device(ctx.h, p, len(knz), fr.ptr(3), cap)
    return rc, fr.after()[GUARD + 3:GUARD + 3 + cap]


_REF = {}


def reference(ctx, chain, ent, bs, checksum=0, skip=False):
    """[(rc, stream)] of kz_compress_device over manycases.buffers, computed once per setting"""
    key = (chain, ent, bs, checksum, skip)
    if key not in _REF:
        _REF[key] = [single_compress(ctx, chain, ent, bs, b, checksum=checksum, skip=skip) for b in mc.buffers(chain, bs)]
    return _REF[key]


# ---- the calls under test, on the set's layout -----------------------------------------------------------------------------------
def many_compress(ctx, chain, ent, bs, bufs, caps=None, checksum=0, skip=False, fill=0xA5):
    """-> (dstLen list, the slots' first dstLen bytes).  Checks the guards and every byte between the slots."""
    import torch
    src, soff = mc.pack(bufs, fill=fill)
    t = torch.from_numpy(src).cuda()
    caps = [kz.compress_bound(len(b), bs) for b in bufs] if caps is None else caps
    doff, payload = mc.slots(caps)
    fr = Frame(payload, "a5", device=True, guard=GUARD)
    got = kz.compress_many_device(ctx, chain, ent, bs, t.data_ptr(), soff, [len(b) for b in bufs], fr.ptr(0), doff, caps,
                                  checksum=checksum, skip_blocks=skip)
    a = fr.after()
    body = a[GUARD:GUARD + payload]
    assert fr.guards_intact(a), ("guards", chain, ent, bs)
    assert bool((body[mc.outside_slots(payload, doff, caps)] == 0xA5).all()), ("bytes between the slots", chain, ent, bs)
    return got, [body[o:o + max(n, 0)].tobytes() for o, n in zip(doff, got)]


def many_decompress(ctx, streams, caps, fill=0xA5):
    """-> (dstLen list, each slot's whole capacity).  Checks the guards and every byte between the slots."""
    import torch
    src, soff = mc.pack(streams, fill=fill)
    t = torch.from_numpy(src).cuda()
    doff, payload = mc.slots(caps)
    fr = Frame(payload, "a5", device=True, guard=GUARD)
    got = kz.decompress_many_device(ctx, t.data_ptr(), soff, [len(s) for s in streams], fr.ptr(0), doff, caps)
    a = fr.after()
    body = a[GUARD:GUARD + payload]
    assert fr.guards_intact(a), "guards"
    assert bool((body[mc.outside_slots(payload, doff, caps)] == 0xA5).all()), "bytes between the slots"
    return got, [body[o:o + c] for o, c in zip(doff, caps)]


def assert_streams(tag, got, out, ref):
    for i, ((rc0, want), rc, have) in enumerate(zip(ref, got, out)):
        assert rc == rc0, (tag, "stream %d" % i, rc, rc0)
        if rc0 >= 0 and have != want:
            k = next(k for k in range(rc0) if have[k] != want[k])
            raise AssertionError("%s: stream %d differs at byte %d of %d: %02x, want %02x" % (tag, i, k, rc0, have[k], want[k]))


# ---- 1: compress parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", mc.BLOCK_SIZES)
@pytest.mark.parametrize("chain,ent", mc.CHAINS, ids=["%s&%s" % c for c in mc.CHAINS])
def test_compress_equals_the_single_call_on_every_segment(ctx, chain, ent, bs):
    bufs = mc.buffers(chain, bs)
    ref = reference(ctx, chain, ent, bs)
    assert all(rc > 0 for rc, _ in ref)
    got, out = many_compress(ctx, chain, ent, bs, bufs)
    assert_streams((chain, ent, bs), got, out, ref)
    # slots that are too small, next to slots that are not: the single call's code, the neighbours unchanged
    caps = [kz.compress_bound(len(b), bs) for b in bufs]
    short = [(ref[i][0] - 1 if i % 3 == 0 else (18 if i % 3 == 1 else caps[i])) & ~1 for i in range(len(bufs))]
    ref2 = [ref[i] if short[i] == caps[i] else single_compress(ctx, chain, ent, bs, bufs[i], cap=short[i]) for i in range(len(bufs))]
    assert all(ref2[i][0] == -12 for i in range(len(bufs)) if short[i] != caps[i])
    got, out = many_compress(ctx, chain, ent, bs, bufs, caps=short)
    assert_streams((chain, ent, bs, "short slots"), got, out, ref2)


@pytest.mark.parametrize("checksum,skip", [(32, False), (64, True)])
def test_compress_with_checksums_and_skip_blocks(ctx, checksum, skip):
    chain, ent, bs = "BWT+RANK+ZRLT", "ANS0", 1024
    ref = reference(ctx, chain, ent, bs, checksum, skip)
    got, out = many_compress(ctx, chain, ent, bs, mc.buffers(chain, bs), checksum=checksum, skip=skip)
    assert_streams((checksum, skip), got, out, ref)


# ---- 2: round trip and decompress parity -----------------------------------------------------------------------------------------
def _decompress_parity(ctx, tag, streams, caps, inputs=None):
    want = [single_decompress(ctx, s, c) for s, c in zip(streams, caps)]
    got, out = many_decompress(ctx, streams, caps)
    for i, ((rc0, d0), rc, d) in enumerate(zip(want, got, out)):
        assert rc == rc0, (tag, "stream %d" % i, rc, rc0)
        if rc0 >= 0:
            assert d[:rc0].tobytes() == d0[:rc0].tobytes(), (tag, "stream %d" % i, "decoded bytes")
            if inputs is not None:
                assert rc0 == len(inputs[i]) and d[:rc0].tobytes() == inputs[i].tobytes(), (tag, "stream %d" % i, "not the input")
    return want, got, out


@pytest.mark.parametrize("bs", mc.BLOCK_SIZES)
@pytest.mark.parametrize("chain,ent", mc.CHAINS, ids=["%s&%s" % c for c in mc.CHAINS])
def test_round_trip_and_decompress_parity(ctx, chain, ent, bs):
    bufs = mc.buffers(chain, bs)
    streams = [s for _, s in reference(ctx, chain, ent, bs)]
    _decompress_parity(ctx, (chain, ent, bs, "exact"), streams, [len(b) for b in bufs], inputs=bufs)
    # one byte short, one block short, capacity 0: every length of the set meets each over the three passes
    L = len(mc.lengths(bs))
    caps = []
    for i, b in enumerate(bufs):
        kind = (i // L + i % L) % 3
        caps.append(max(len(b) - 1, 0) if kind == 0 else (max(len(b) - bs, 0) if kind == 1 else 0))
    want, _, _ = _decompress_parity(ctx, (chain, ent, bs, "short"), streams, caps)
    assert sum(1 for rc, _ in want if rc == -12) >= 15 and any(rc == 0 for rc, _ in want), [rc for rc, _ in want]


# ---- 3: mixed headers ---------------------------------------------------------------------------------------------------------------
def test_streams_of_different_headers_in_one_call(ctx):
    settings = [("NONE", "NONE", 1024, 0), ("LZ", "HUFFMAN", 65536, 32), ("BWT+RANK+ZRLT", "ANS0", 1024, 64), ("LZ", "HUFFMAN", 1024, 0)]
    streams, inputs = [], []
    for k in range(9):                                                         # every length but the longest, the settings in turn
        for j, (chain, ent, bs, chk) in enumerate(settings):
            if (k + j) % 2:
                continue
            b = mc.buffers(chain, bs)[k]
            rc, s = single_compress(ctx, chain, ent, bs, b, checksum=chk)
            assert rc > 0
            streams.append(s)
            inputs.append(b)
    heads = {(i["transform"], i["entropy"], i["blockSize"], i["checksum"]) for i in map(kz.knz_index, streams)}
    assert len(heads) == 4 and len({h[0] for h in heads}) == 3 and len({h[2] for h in heads}) == 2 and len({h[3] for h in heads}) == 3
    _decompress_parity(ctx, "mixed", streams, [len(b) for b in inputs], inputs=inputs)
    _decompress_parity(ctx, "mixed, a byte short", streams, [max(len(b) - 1, 0) for b in inputs])


# ---- 4: faults --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_stream(ctx):
    data = mc.small_input()
    rc, knz = single_compress(ctx, mc.SMALL_CHAIN[0], mc.SMALL_CHAIN[1], mc.SMALL_BS, data)
    assert 0 < rc < 200, rc
    return data, knz


def _faults_in_one_call(ctx, tag, bad, data, knz):
    streams, goods = mc.interleave(bad, knz)
    caps = [len(data)] * len(streams)
    good_ref = single_decompress(ctx, knz, len(data))
    assert good_ref[0] == len(data)
    want = [good_ref if i in set(goods) else single_decompress(ctx, s, len(data)) for i, s in enumerate(streams)]
    got, out = many_decompress(ctx, streams, caps)
    for i, ((rc0, d0), rc, d) in enumerate(zip(want, got, out)):
        what = "good" if i % 2 == 0 else bad[i // 2][0]
        assert rc == rc0, (tag, what, rc, rc0)
        if rc0 >= 0:
            assert d[:rc0].tobytes() == d0[:rc0].tobytes(), (tag, what, "decoded bytes")
    for i in goods:
        assert got[i] == len(data) and out[i].tobytes() == data.tobytes(), (tag, "good neighbour %d" % i)
    return [rc for i, (rc, _) in enumerate(want) if i % 2]


def test_truncations_in_one_call(ctx, small_stream):
    data, knz = small_stream
    codes = set(_faults_in_one_call(ctx, "cut", mc.truncations(knz), data, knz))
    assert -15 in codes and len([c for c in codes if c < 0]) >= 3, codes


def test_header_faults_in_one_call(ctx, small_stream):
    data, knz = small_stream
    import refinputs
    codes = _faults_in_one_call(ctx, "header", mc.header_faults(knz), data, knz)
    assert codes == [-c for _, _, c in refinputs.header_faults(knz)], codes


def test_prefix_faults_in_one_call(ctx, small_stream):
    data, knz = small_stream
    codes = _faults_in_one_call(ctx, "prefix", mc.prefix_faults(knz, kz.knz_index(knz)["blocks"]), data, knz)
    assert any(c < 0 for c in codes), codes


def test_block_header_fault_delivers_the_blocks_in_front(ctx, small_stream):
    data, knz = small_stream
    blocks = kz.knz_index(knz)["blocks"]
    assert len(blocks) == 3
    bad = [("block 2 header byte %d" % byte, mc.block_header_fault(knz, blocks, 1, byte)) for byte in range(3)]
    streams, goods = mc.interleave(bad, knz)
    caps = [len(data)] * len(streams)
    got, out = many_decompress(ctx, streams, caps)
    for k, (what, s) in enumerate(bad):
        rc0, d0 = single_decompress(ctx, s, len(data))
        assert rc0 < 0 and got[2 * k + 1] == rc0, (what, got[2 * k + 1], rc0)
        bs = mc.SMALL_BS
        assert d0[:bs].tobytes() == data[:bs].tobytes(), (what, "the single call's delivered block")
        assert out[2 * k + 1][:bs].tobytes() == d0[:bs].tobytes(), (what, "blocks in front")
    for i in goods:
        assert got[i] == len(data) and out[i].tobytes() == data.tobytes()


# ---- 5: seams ---------------------------------------------------------------------------------------------------------------------
def test_groups_of_three_blocks_give_the_same_results(ctx, monkeypatch):
    chain, ent, bs = "BWT+RANK+ZRLT", "ANS0", 1024
    bufs = mc.buffers(chain, bs)
    ref = reference(ctx, chain, ent, bs)                                       # (computed with the default chunks)
    plan = mc.writer_groups([len(b) for b in bufs], bs, 3)
    assert any(k == "single" for k, _ in plan) and sum(1 for k, g in plan if k == "group" and len(g) > 1) >= 2, plan
    monkeypatch.setenv("KZ_STREAM_CHUNK", "3")
    ctx.reload_switches()
    got, out = many_compress(ctx, chain, ent, bs, bufs)
    assert_streams("chunk 3", got, out, ref)
    dgot, dout = many_decompress(ctx, [s for _, s in ref], [len(b) for b in bufs])
    monkeypatch.delenv("KZ_STREAM_CHUNK")
    ctx.reload_switches()
    dgot0, dout0 = many_decompress(ctx, [s for _, s in ref], [len(b) for b in bufs])
    assert dgot == dgot0 == [len(b) for b in bufs]
    for b, d, d0 in zip(bufs, dout, dout0):
        assert d.tobytes() == d0.tobytes() == b.tobytes()


# ---- 6: independence ----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_lies_between_the_segments(ctx):
    chain, ent, bs = "BWT+RANK+ZRLT", "ANS0", 1024
    bufs = mc.buffers(chain, bs)
    a = many_compress(ctx, chain, ent, bs, bufs, fill=0xA5)
    b = many_compress(ctx, chain, ent, bs, bufs, fill=0x3C)
    assert a[0] == b[0] and a[1] == b[1]
    caps = [len(x) for x in bufs]
    da = many_decompress(ctx, a[1], caps, fill=0xA5)
    db = many_decompress(ctx, a[1], caps, fill=0x3C)
    assert da[0] == db[0] == caps
    assert all(x.tobytes() == y.tobytes() for x, y in zip(da[1], db[1]))


# ---- 7: launches ------------------------------------------------------------------------------------------------------------------
MANY_KERNELS = ("k_knz_gather", "k_knz_pack_many", "k_knz_heads", "k_knz_walk_many", "k_knz_unpack_many", "k_knz_scatter")


def _round_trip_counted(ctx, n):
    """n streams of 1025 .. 2048 bytes through both calls under kernel timing -> {kernel: launches}"""
    import torch
    bs = 1024
    base = datagen.stream(48, bs)
    lens = [1025 + (i * 37) % 1024 for i in range(n)]
    bufs = []
    for i, ln in enumerate(lens):
        b = base[(i * 131) % (len(base) - 2048):][:ln].copy()
        b[0], b[1] = i & 0xFF, i >> 8
        bufs.append(b)
    src, soff = mc.pack(bufs, gaps=mc.GAPS)
    t = torch.from_numpy(src).cuda()
    caps = [kz.compress_bound(ln, bs) for ln in lens]
    doff, payload = mc.slots(caps)
    dst = torch.full((payload + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    back = torch.full((len(src) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        sizes = kz.compress_many_device(ctx, "LZ", "HUFFMAN", bs, t.data_ptr(), soff, lens, dst.data_ptr(), doff, caps)
        assert all(s > 0 for s in sizes)
        got = kz.decompress_many_device(ctx, dst.data_ptr(), doff, sizes, back.data_ptr(), soff, lens)
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    assert got == lens
    h = back.cpu().numpy()
    for o, b in zip(soff, bufs):                                               # every stream against its input
        assert h[o:o + len(b)].tobytes() == b.tobytes()
    assert bool((h[mc.outside_slots(len(h), soff, lens)] == 0xA5).all())
    assert "k_knz_walk" not in times and "k_knz_pack" not in times and "k_knz_unpack" not in times, sorted(times)
    return {k: times.get(k, {}).get("launches", 0) for k in MANY_KERNELS}


def test_launches_do_not_grow_with_the_streams_of_a_group(ctx, monkeypatch):
    """4 000 streams hold about 8 000 blocks, four of the writer's default groups (2 048 blocks) and four of the reader's: the
    launches of a GROUP cannot grow with its streams, those of a call grow with its groups.  So the comparison with 40 streams is
    made with KZ_STREAM_CHUNK=16384, where both calls are one group, and again with the default chunks, where the 4 000 streams
    must cost exactly their number of groups times what the 40 cost."""
    L = ctx.lib
    fwd0, inv0 = L.kz_host_stage_blocks(0, 0), L.kz_host_stage_blocks(1, 0)
    monkeypatch.setenv("KZ_STREAM_CHUNK", "16384")
    ctx.reload_switches()
    few = _round_trip_counted(ctx, 40)
    many = _round_trip_counted(ctx, 4000)
    assert all(few[k] > 0 for k in MANY_KERNELS), few
    assert many == few, (many, few)
    monkeypatch.delenv("KZ_STREAM_CHUNK")
    ctx.reload_switches()
    many = _round_trip_counted(ctx, 4000)
    groups = len(mc.writer_groups([1025 + (i * 37) % 1024 for i in range(4000)], 1024, 2048))
    assert groups == 4
    # (the reader: 2 blocks a stream, 2 048 blocks a group; its count pass and the header table run once per call)
    want = {"k_knz_gather": groups, "k_knz_pack_many": groups, "k_knz_heads": 1, "k_knz_walk_many": 1 + groups,
            "k_knz_unpack_many": groups, "k_knz_scatter": groups}
    assert few == {k: (2 if k == "k_knz_walk_many" else 1) for k in MANY_KERNELS}, few
    assert many == want, (many, want)
    assert (L.kz_host_stage_blocks(0, 0), L.kz_host_stage_blocks(1, 0)) == (fwd0, inv0)


# ---- 8: refusals and empties --------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls(ctx):
    L = ctx.lib
    fr = Frame(4096, "a5", device=True, guard=GUARD)
    t, p = up(datagen.block(1, 2048))
    i64 = lambda *v: np.array(v, dtype=np.int64)
    so, sl, do, dc, out = i64(0, 1024), i64(1024, 1024), i64(1, 2049), i64(2000, 2000), i64(7, 7)
    tt, et = kz.transform_type("LZ"), kz.ENTROPY_IDS["HUFFMAN"]

    def comp(bs=1024, n=2, src=p, dst=None, so=so, sl=sl, do=do, dc=dc, res=out):
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.kz_compress_many_device(ctx.h, tt, et, bs, src, ptr(so), ptr(sl), n, fr.ptr(0) if dst is None else dst, ptr(do), ptr(dc), ptr(res))

    def dec(n=2, src=p, so=so, sl=sl, do=do, dc=dc, res=out):
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.kz_decompress_many_device(ctx.h, src, ptr(so), ptr(sl), n, fr.ptr(0), ptr(do), ptr(dc), ptr(res))

    assert comp(n=0) == 0 and dec(n=0) == 0
    assert L.kz_compress_many_device(ctx.h, tt, et, 1024, None, None, None, 0, None, None, None, None) == 0
    assert L.kz_decompress_many_device(ctx.h, None, None, None, 0, None, None, None, None) == 0
    for call in (comp, dec):
        assert call(n=-1) == -18
        for name in ("so", "sl", "do", "dc", "res"):
            assert call(**{name: None}) == -18, name
        assert call(src=None) == -18
        for name, arr in (("so", so), ("sl", sl), ("do", do), ("dc", dc)):
            bad = arr.copy()
            bad[1] = -1
            assert call(**{name: bad}) == -18, name
    assert L.kz_compress_many_device(None, tt, et, 1024, p, so.ctypes.data, sl.ctypes.data, 2, fr.ptr(0), do.ctypes.data, dc.ctypes.data, out.ctypes.data) == -18
    for bs in (1000, 512, 1040 + 8, (1 << 30) + 16):
        want = L.kz_compress_device(ctx.h, tt, et, bs, p, 1024, fr.ptr(0), 2000)
        assert want < 0 and comp(bs=bs) == want, (bs, want)
    assert fr.untouched() and list(out) == [7, 7]
    assert kz.compress_many_bound([0, 5, 3000], 1024) == sum(kz.compress_bound(n, 1024) for n in (0, 5, 3000))
    assert kz.compress_many_bound([], 1024) == 0
    assert L.kz_compress_many_bound(None, 1, 1024) == -18 and L.kz_compress_many_bound(i64(-1).ctypes.data, 1, 1024) == -18


# ---- 9: tensor helpers ------------------------------------------------------------------------------------------------------------
def test_tensor_helpers(ctx):
    import torch
    g = torch.Generator().manual_seed(5)
    tensors = [(torch.randn(70001, generator=g) * 4).round().div(4).cuda(),                       # float32
               torch.randint(-3, 4, (333, 77), generator=g, dtype=torch.int16).cuda(),
               torch.empty(0, dtype=torch.float32, device="cuda"),
               torch.from_numpy(datagen.stream(3, 65536)).cuda()[1:],                             # uint8 at storage offset 1
               (torch.randn(4099, generator=g).double() * 2).round().cuda()]
    knz = kz.compress_tensors(ctx, tensors, block_size=65536)
    assert len(knz) == len(tensors) and all(k.dtype == torch.uint8 and k.is_cuda for k in knz)
    store = {k.untyped_storage().data_ptr() for k in knz}
    assert len(store) == 1                                                      # views of one buffer
    for t, k in zip(tensors, knz):
        one = kz.compress_tensor(ctx, t, block_size=65536)
        assert torch.equal(k.cpu(), one.cpu())
    back = kz.decompress_tensors(ctx, [k.clone() for k in knz])
    for t, b in zip(tensors, back):
        assert b.dtype == torch.uint8 and torch.equal(b.cpu(), t.cpu().reshape(-1).view(torch.uint8))
    back = kz.decompress_tensors(ctx, knz, sizes=[t.numel() * t.element_size() for t in tensors])
    for t, b in zip(tensors, back):
        assert torch.equal(b.cpu(), t.cpu().reshape(-1).view(torch.uint8))
    with pytest.raises(kz.KanziError) as e:
        kz.decompress_tensors(ctx, knz, sizes=[t.numel() * t.element_size() - (1 if i == 1 else 0) for i, t in enumerate(tensors)])
    assert "stream 1" in str(e.value)
    with pytest.raises(ValueError):
        kz.compress_tensors(ctx, [torch.zeros(4, 4, device="cuda").t()])
