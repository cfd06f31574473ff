"""kz_knz_splice_device against kz_knz_splice on the case set of tests/knzsplice.py, byte for byte and return value for return
value: the host form is the reference throughout (tests/test_knz_splice_cases.py holds it to the Python model).  Sources are
built by the library and lie at odd addresses, back to back in one device buffer; the destination lies at odd offsets inside a
poisoned frame whose guards, and whose bytes around dst, must stay as they were."""
import numpy as np
import pytest

import kanzi_amd as kz
import knzsplice as ks
from layouthelp import Frame

pytestmark = pytest.mark.gpu

GUARD = 4096
KERNELS_NOT_RUN = ("k_knz_unpack", "k_knz_pack", "k_knz_unpack_many", "k_knz_pack_many")


def _compress(ctx):
    def f(chain, ent, bs, data, checksum):
        cap = kz.compress_bound(len(data), bs)
        dst = np.empty(cap, dtype=np.uint8)
        data = np.ascontiguousarray(data)
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
def cases(ctx):
    return ks.cases(_compress(ctx), _encode_block(ctx))


def host(case, cap, **override):
    """the reference: kz_knz_splice -> (rc, dst[0 .. max(rc, 0)))"""
    src, offs = ks.pack(case.sources)
    dst = np.full(max(cap, 0) + 16, ks.POISON, dtype=np.uint8)
    rc = ks.call(kz.load_library().kz_knz_splice, (), src.ctypes.data, offs, case.lens, case.pieces, case.input_size, dst.ctypes.data, cap, **override)
    return rc, dst[:max(rc, 0)].tobytes()


@pytest.fixture(scope="module")
def reference(cases):
    """name -> (rc, bytes) of the host form with the bound as capacity, computed once"""
    return {c.name: host(c, ks.bound(c)) for c in cases}


def device(ctx, case, cap, at=3, lead=1, gap=0, fill=ks.POISON, tail=0, **override):
    """kz_knz_splice_device with the sources `lead` bytes into one device buffer and dst `at` bytes into a poisoned frame ->
    (rc, dst[0 .. max(rc, 0))).  Checks the guards and every byte of the frame outside dst[0 .. cap); after a refusal, all of it."""
    import torch
    src, offs = ks.pack(case.sources, lead=lead, gap=gap, fill=fill, tail=tail)
    t = torch.from_numpy(src).cuda()
    room = max(cap, 0)
    fr = Frame(at + room + 19, "a5", device=True, guard=GUARD)
    rc = ks.call(ctx.lib.kz_knz_splice_device, (ctx.h,), t.data_ptr(), offs, case.lens, case.pieces, case.input_size, fr.ptr(at), cap, **override)
    a = fr.after()
    assert fr.guards_intact(a), ("guards", case.name)
    body = a[GUARD:GUARD + fr.payload]
    assert bool((body[:at] == ks.POISON).all()) and bool((body[at + room:] == ks.POISON).all()), ("bytes around dst", case.name)
    if rc < 0:
        assert fr.untouched(a), ("dst written by a refused call", case.name, rc)
    assert torch.equal(t.cpu(), torch.from_numpy(src)), ("sources changed", case.name)
    return rc, body[at:at + max(rc, 0)].tobytes()


def test_device_equals_host_on_the_case_set(ctx, cases, reference):
    for i, c in enumerate(cases):
        rc0, want = reference[c.name]
        assert rc0 > 0, c.name
        rc, got = device(ctx, c, ks.bound(c), at=1 + 2 * (i % 8), lead=1 + 2 * (i % 3))
        assert rc == rc0 and got == want, (c.name, rc, rc0)
        # dstCap exact succeeds, one less is refused
        rc, got = device(ctx, c, rc0, at=3)
        assert rc == rc0 and got == want, (c.name, "exact capacity", rc)
        assert device(ctx, c, rc0 - 1, at=5)[0] == host(c, rc0 - 1)[0] == -12, (c.name, "one byte less")
        assert "destination too small" in ctx.error()


def test_every_result_decodes_on_the_device(ctx, cases, reference):
    import torch
    stated = [c for c in cases if c.decoded is not None]
    assert len(stated) >= 25
    for c in stated:
        knz = reference[c.name][1]
        src = torch.from_numpy(np.frombuffer(b"\0" + knz, dtype=np.uint8).copy()).cuda()
        cap = len(c.pieces) * ks.head(knz)["blockSize"] + 16                     # (the reader wants room for every block to start in)
        dst = torch.full((cap + 1,), ks.POISON, dtype=torch.uint8, device="cuda")
        n = kz.decompress_device(ctx, src.data_ptr() + 1, len(knz), dst.data_ptr() + 1, cap)
        assert n == len(c.decoded) and dst[1:1 + n].cpu().numpy().tobytes() == c.decoded, c.name


def test_equal_streams(cases, reference):
    for c in cases:
        if c.equals is not None:
            assert reference[c.name][1] == c.equals, c.name


def test_results_do_not_depend_on_what_lies_outside_the_sources(ctx, cases, reference):
    for c in cases:
        rc, got = device(ctx, c, ks.bound(c), lead=2, gap=7, fill=0x3C, tail=64)
        assert (rc, got) == reference[c.name], c.name


def test_chunks_of_three_pieces_give_the_same_bytes(ctx, cases, reference, monkeypatch):
    cov = ks.coverage(cases)
    assert cov["seam inside a byte"] and cov["seam on a byte"]
    monkeypatch.setenv("KZ_STREAM_CHUNK", str(ks.CHUNK))
    ctx.reload_switches()
    for c in cases:
        rc, got = device(ctx, c, ks.bound(c))
        assert (rc, got) == reference[c.name], c.name
        assert device(ctx, c, rc - 1)[0] == -12, c.name
    refs, base = ks.refusals(_compress(ctx))
    for r in refs:
        if r.text and "piece" in r.text:                                        # the first failing piece, whichever chunk it lies in
            assert device(ctx, r.case, ks.bound(base) if r.cap is None else r.cap, **r.override)[0] == r.code, r.name
            assert r.text in ctx.error(), (r.name, ctx.error())


def test_refusals(ctx):
    refs, base = ks.refusals(_compress(ctx))
    assert device(ctx, base, ks.bound(base))[0] == host(base, ks.bound(base))[0] > 0
    for r in refs:
        cap = ks.bound(base) if r.cap is None else r.cap
        rc0, _ = host(r.case, cap, **r.override)
        rc, _ = device(ctx, r.case, cap, **r.override)                          # (asserts that the frame is untouched)
        assert rc == rc0 == r.code, (r.name, rc, rc0, r.code)
        if r.text:
            assert r.text in ctx.error(), (r.name, ctx.error())
    L = ctx.lib
    assert ks.call(L.kz_knz_splice_device, (None,), 1, [0], [30], [], 0, 1, 64) == -18


def test_joining_the_slots_of_a_many_stream_call(ctx):
    """the streams kz_compress_many_device wrote, joined, are the stream kz_compress_device writes for the joined buffer"""
    import torch
    chain, ent, bs = "BWT+RANK+ZRLT", "ANS0", 1024
    lens = [2 * bs, 3 * bs, bs, bs + 77]
    data = ks._data(bs, sum(lens) // bs, sum(lens) % bs, 90)
    t = torch.from_numpy(np.concatenate([np.zeros(1, dtype=np.uint8), data])).cuda()
    soff = [1 + sum(lens[:i]) for i in range(len(lens))]
    caps = [kz.compress_bound(n, bs) for n in lens]
    doff = [3 + sum(caps[:i]) + 5 * i for i in range(len(caps))]
    slots = torch.full((doff[-1] + caps[-1] + 8,), ks.POISON, dtype=torch.uint8, device="cuda")
    sizes = kz.compress_many_device(ctx, chain, ent, bs, t.data_ptr(), soff, lens, slots.data_ptr(), doff, caps, checksum=32)
    assert all(s > 0 for s in sizes)
    idx = [kz.knz_index_device(ctx, slots.data_ptr() + o, n) for o, n in zip(doff, sizes)]
    pieces, total = kz.splice_concat(idx)
    assert total == len(data) and len(pieces) == 8
    cap = kz.knz_splice_bound([w for _, _, w in pieces])
    out = torch.full((cap + 1,), ks.POISON, dtype=torch.uint8, device="cuda")
    n = kz.knz_splice_device(ctx, slots.data_ptr(), doff, sizes, pieces, total, out.data_ptr() + 1, cap)
    whole = torch.full((kz.compress_bound(len(data), bs),), ks.POISON, dtype=torch.uint8, device="cuda")
    m = kz.compress_device(ctx, chain, ent, bs, t.data_ptr() + 1, len(data), whole.data_ptr(), whole.numel(), checksum=32)
    assert n == m and torch.equal(out[1:1 + n], whole[:m])


def _counted(ctx, npieces):
    """a splice of npieces pieces of one stream under kernel timing -> {kernel: launches}"""
    import torch
    S = _compress(ctx)("LZ", "HUFFMAN", 1024, ks._data(1024, 8, 0, 5), 0)
    blocks = kz.knz_index(S)["blocks"]
    pieces = [(0,) + blocks[(5 * i) % len(blocks)] for i in range(npieces)]
    src = torch.from_numpy(np.frombuffer(S, dtype=np.uint8).copy()).cuda()
    cap = kz.knz_splice_bound([w for _, _, w in pieces])
    dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        n = kz.knz_splice_device(ctx, src.data_ptr(), [0], [len(S)], pieces, 0, dst.data_ptr(), cap)
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    assert dst[:n].cpu().numpy().tobytes() == kz.knz_splice([S], pieces, 0)
    return {k: v["launches"] for k, v in times.items()}


def test_kernels_and_launches(ctx):
    few, many = _counted(ctx, 8), _counted(ctx, 64)
    assert few.get("k_knz_splice", 0) > 0 and few.get("k_knz_check_many", 0) > 0, few
    assert not any(k in few or k in many for k in KERNELS_NOT_RUN), (few, many)
    assert many == few == {"k_knz_heads": 1, "k_knz_check_many": 1, "k_knz_splice": 1}, (few, many)
