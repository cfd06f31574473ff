"""The .knz container on device memory (kz_compress_device / kz_decompress_device / kz_knz_assemble_device / kz_knz_index_device)
against the host calls it restates: kz_compress, kz_decompress, kz_knz_assemble and kz_knz_index are the reference throughout.
Sources sit at odd device addresses, destinations are poisoned with 0xA5 and framed by guard bytes."""
import time

import numpy as np
import pytest

import kanzi_amd as kz
import datagen
import knzcases
import refinputs
import textgen
from layouthelp import Frame

pytestmark = pytest.mark.gpu

CHAINS = [("NONE", "NONE"), ("BWT+RANK+ZRLT", "ANS0"), ("LZ", "HUFFMAN"), ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0"), ("LZP+BWT", "CM")]
ORACLE_CHAINS = CHAINS[:4]
BLOCK_SIZES = [1024, 65536]
GUARD = 4096


def sizes(bs):
    return [0, 1, 15, 16, bs - 1, bs, bs + 1, 3 * bs, 3 * bs + 15, 40 * bs + 777]


_DATA = {}


def data_for(chain, bs):
    """40 blocks and a tail, block classes mixed so that the block streams differ in length (text in every other block for TEXT)"""
    key = ("text" if "TEXT" in chain else "bin", bs)
    if key not in _DATA:
        n = 40 * bs + 777
        parts = []
        text = np.frombuffer(textgen.english(3 * bs, 7), dtype=np.uint8) if key[0] == "text" else None
        for b in range(41):
            if key[0] == "text" and b % 2 == 0:
                at = (b * 7919) % (2 * bs)                                    # another window of the text per block
                parts.append(text[at:at + bs])
            else:
                parts.append(datagen.block(b, bs))
        _DATA[key] = np.ascontiguousarray(np.concatenate(parts)[:n])
    return _DATA[key]


def up(a, lead=1):
    """bytes / array -> (tensor that owns the memory, device address `lead` bytes into it): an odd address by default"""
    import torch
    a = np.frombuffer(bytes(a), dtype=np.uint8) if not isinstance(a, np.ndarray) else a
    buf = np.zeros(lead + max(len(a), 1), dtype=np.uint8)
    buf[lead:lead + len(a)] = a
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + lead


def host_compress(ctx, chain, ent, bs, data, checksum=0, skip=False):
    """kz_compress -> (rc, bytes)"""
    a = np.ascontiguousarray(data, dtype=np.uint8)
    cap = kz.compress_bound(len(a), bs)
    dst = np.empty(cap, dtype=np.uint8)
    ctx.set_checksum(checksum)
    ctx.set_skip_blocks(skip)
    try:
        rc = ctx.lib.kz_compress(ctx.h, kz.transform_type(chain), kz.ENTROPY_IDS[ent], bs, a.ctypes.data if len(a) else dst.ctypes.data, len(a), dst.ctypes.data, cap)
    finally:
        ctx.set_checksum(0)
        ctx.set_skip_blocks(False)
    return rc, dst[:max(rc, 0)].tobytes()


def host_decompress(ctx, knz, cap):
    """kz_decompress -> (rc, the whole destination)"""
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    dst = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    rc = ctx.lib.kz_decompress(ctx.h, src.ctypes.data, len(knz), dst.ctypes.data, cap)
    return rc, dst


def dev_compress(ctx, chain, ent, bs, data, checksum=0, skip=False, cap=None):
    """kz_compress_device, src at an odd address, dst poisoned and framed -> (rc, bytes, frame)"""
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
    assert fr.guards_intact(a) and bytes(a[GUARD:GUARD + 3]) == b"\xa5" * 3, ("guards", chain, ent, bs, len(data))
    return rc, a[GUARD + 3:GUARD + 3 + max(rc, 0)].tobytes(), fr


def dev_decompress(ctx, knz, cap):
    """kz_decompress_device, src at an odd address, dst poisoned, guards right behind cap -> (rc, dst[0 .. cap))"""
    t, p = up(knz)
    fr = Frame(3 + cap, "a5", device=True, guard=GUARD)
    rc = ctx.lib.kz_decompress_device(ctx.h, p, len(knz), fr.ptr(3), cap)
    a = fr.after()
    assert fr.guards_intact(a) and bytes(a[GUARD:GUARD + 3]) == b"\xa5" * 3, ("guards", len(knz), cap)
    return rc, a[GUARD + 3:GUARD + 3 + cap]


# ---- 1, 2: assemble and index ------------------------------------------------------------------------------------------------
CASES = knzcases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_assemble_and_index_equal_the_host_calls(ctx, case):
    want = knzcases.assemble_host(ctx.lib, case)
    size = len(want)
    buf, lead, stride = case.layout(lead=1, odd=True)
    import torch
    t = torch.from_numpy(buf).cuda()                                          # rows at base + 1, an odd stride apart
    bits = np.ascontiguousarray(case.bits, dtype=np.int64)
    for cap, code in ((size, 0), (size - 1, 12), (size + 100, 0)):
        fr = Frame(3 + cap, "a5", device=True, guard=GUARD)
        rc = ctx.lib.kz_knz_assemble_device(ctx.h, 0, 0, knzcases.BLOCK_SIZE, case.input_size, case.checksum, t.data_ptr() + lead, stride,
                                            bits.ctypes.data if len(bits) else None, len(bits), fr.ptr(3), cap)
        a = fr.after()
        assert fr.guards_intact(a) and bytes(a[GUARD:GUARD + 3]) == b"\xa5" * 3, (case.name, cap)
        if code:
            assert rc == -code, (case.name, cap, rc)                          # ERR_WRITE_FILE
            continue
        assert rc == size, (case.name, cap, rc)
        got = a[GUARD + 3:GUARD + 3 + size].tobytes()
        if got != want:
            i = next(k for k in range(size) if got[k] != want[k])
            raise AssertionError("%s: stream differs at byte %d of %d: %02x, want %02x" % (case.name, i, size, got[i], want[i]))
    ts, p = up(want)
    assert kz.knz_index_device(ctx, p, size) == kz.knz_index(want), case.name


def test_assemble_and_index_refuse_what_the_host_calls_refuse(ctx):
    t, p = up(b"\0" * 64)
    L = ctx.lib
    one = np.array([8], dtype=np.int64)
    assert L.kz_knz_assemble_device(ctx.h, 0, 0, 1024, 0, 16, p, 8, one.ctypes.data, 1, p, 64) == -18
    assert L.kz_knz_assemble_device(ctx.h, 0, 0, 1024, 0, 0, p, 8, one.ctypes.data, -1, p, 64) == -18
    assert L.kz_knz_assemble_device(ctx.h, 0, 0, 1024, 0, 0, None, 8, one.ctypes.data, 1, p, 64) == -18
    assert L.kz_knz_index_device(ctx.h, p, 19, None, None, None, None, None, None, None, 0) == -15
    z = np.zeros(64, dtype=np.uint8)
    assert L.kz_knz_index_device(ctx.h, p, 64, None, None, None, None, None, None, None, 0) == L.kz_knz_index(z.ctypes.data, 64, None, None, None, None, None, None, None, 0) == -15


# ---- 3, 5: compress parity, decompress ------------------------------------------------------------------------------------------
def _parity(ctx, chain, ent, bs, ns, checksum=0, skip=False, oracle_too=False):
    data = data_for(chain, bs)
    for n in ns:
        d = data[:n]
        rc0, want = host_compress(ctx, chain, ent, bs, d, checksum, skip)
        rc, got, _ = dev_compress(ctx, chain, ent, bs, d, checksum, skip)
        assert rc == rc0 and rc > 0, (chain, ent, bs, n, rc, rc0)
        assert got == want, (chain, ent, bs, n, "stream differs")
        # and back, into a destination of exactly n bytes
        rd, out = dev_decompress(ctx, got, n)
        assert rd == n and out.tobytes() == d.tobytes(), (chain, ent, bs, n, rd)
        if oracle_too:
            import oracle
            ref = oracle.compress(chain, ent, bs, d, jobs=2, checksum=checksum, skip_blocks=skip)
            rd, out = dev_decompress(ctx, ref, n)
            assert rd == n and out.tobytes() == d.tobytes(), (chain, ent, bs, n, rd, "oracle stream")
        # destinations that are too small: kz_decompress's code, nothing written behind them
        if n in (3 * bs, 3 * bs + 15):
            for cap in (n - 1, n - bs if n % bs == 0 else n - n % bs - 1, bs - 1):
                r0, _ = host_decompress(ctx, got, cap)
                r1, _ = dev_decompress(ctx, got, cap)
                assert r1 == r0 and r1 < 0, (chain, ent, bs, n, cap, r1, r0)
        # a destination too small for the stream: kz_compress's code
        if n in (bs + 1, 3 * bs + 15):
            for cap in (rc - 1, 19, rc - 300):
                if cap < 0:
                    continue
                r1, _, fr = dev_compress(ctx, chain, ent, bs, d, checksum, skip, cap=cap)
                a = np.empty(max(cap, 1), dtype=np.uint8)
                ctx.set_checksum(checksum)
                ctx.set_skip_blocks(skip)
                r0 = ctx.lib.kz_compress(ctx.h, kz.transform_type(chain), kz.ENTROPY_IDS[ent], bs, d.ctypes.data, n, a.ctypes.data, cap)
                ctx.set_checksum(0)
                ctx.set_skip_blocks(False)
                assert r1 == r0 == -12, (chain, ent, bs, n, cap, r1, r0)


@pytest.mark.parametrize("k", range(10), ids=["n0", "n1", "n15", "n16", "bs-1", "bs", "bs+1", "3bs", "3bs+15", "40bs+777"])
@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("chain,ent", CHAINS, ids=["%s&%s" % c for c in CHAINS])
def test_compress_equals_kz_compress_and_decodes_back(ctx, chain, ent, bs, k):
    _parity(ctx, chain, ent, bs, sizes(bs)[k:k + 1], oracle_too=(chain, ent) in ORACLE_CHAINS)


@pytest.mark.parametrize("chain,ent,bs,checksum,skip", [("BWT+RANK+ZRLT", "ANS0", 1024, 32, False), ("LZ", "HUFFMAN", 65536, 64, False),
                                                        ("NONE", "NONE", 1024, 0, True), ("BWT+RANK+ZRLT", "ANS0", 65536, 64, True)])
def test_compress_with_checksums_and_skip_blocks(ctx, chain, ent, bs, checksum, skip):
    _parity(ctx, chain, ent, bs, sizes(bs), checksum=checksum, skip=skip, oracle_too=True)


# ---- 4: chunk seams ----------------------------------------------------------------------------------------------------------------
def test_chunk_seams_fall_inside_bytes(ctx, monkeypatch):
    bs, chain, ent = 1024, "BWT+RANK+ZRLT", "ANS0"
    data = data_for(chain, bs)[:10 * bs + 333]
    rc0, want = host_compress(ctx, chain, ent, bs, data)
    idx = kz.knz_index(want)
    assert len(idx["blocks"]) == 11
    # chunks of 3 blocks: chunk k > 0 starts at the prefix of block 3 k, which is where block 3 k - 1 ends
    seams = [idx["blocks"][3 * k - 1][0] + idx["blocks"][3 * k - 1][1] for k in (1, 2, 3)]
    assert sum(1 for s in seams if s % 8) >= 2, seams                        # (a property of the data, checked on the host's stream)
    monkeypatch.setenv("KZ_STREAM_CHUNK", "3")
    rc, got, _ = dev_compress(ctx, chain, ent, bs, data)
    assert rc == rc0 and got == want
    rd, out = dev_decompress(ctx, got, len(data))                             # the reader's chunks: 3 blocks as well
    assert rd == len(data) and out.tobytes() == data.tobytes()
    monkeypatch.delenv("KZ_STREAM_CHUNK")
    rc, got, _ = dev_compress(ctx, chain, ent, bs, data)
    assert rc == rc0 and got == want


# ---- 6: short blocks in the middle ---------------------------------------------------------------------------------------------------
def test_short_middle_blocks_close_up(ctx):
    bs, chain, ent = 1024, "BWT+RANK+ZRLT", "ANS0"
    lens = [bs, 100, bs, 17, bs - 1, bs]
    src = np.zeros(len(lens) * bs, dtype=np.uint8)
    for i, l in enumerate(lens):
        src[i * bs:i * bs + l] = datagen.block(i, bs, cls=i % 3)[:l]
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros(len(lens) * ostride, dtype=np.uint8)
    ctx.set_block_size(bs)
    res = kz.encode_blocks(ctx, chain, ent, src, bs, lens, out, ostride)
    streams = [out[i * ostride:i * ostride + (res[i].bits + 7) // 8].tobytes() for i in range(len(lens))]
    whole = b"".join(src[i * bs:i * bs + l].tobytes() for i, l in enumerate(lens))
    knz = kz.knz_assemble(chain, ent, bs, len(whole), streams, [r.bits for r in res])
    for cap in (len(lens) * bs, len(whole), len(whole) - 1, len(whole) + 5):
        r0, h = host_decompress(ctx, knz, cap)
        r1, d = dev_decompress(ctx, knz, cap)
        assert r1 == r0, (cap, r1, r0)
        if r0 >= 0:
            assert r0 == len(whole) and d[:r0].tobytes() == whole and h[:r0].tobytes() == whole, cap
    assert host_decompress(ctx, knz, len(lens) * bs)[0] == len(whole)
    # every block short but the last: each moves left over its own row
    lens2 = [bs - 1] * 7 + [bs]
    src2 = np.concatenate([datagen.block(9 + i, bs, cls=1) for i in range(len(lens2))])
    out2 = np.zeros(len(lens2) * ostride, dtype=np.uint8)
    res2 = kz.encode_blocks(ctx, chain, ent, src2, bs, lens2, out2, ostride)
    whole2 = b"".join(src2[i * bs:i * bs + l].tobytes() for i, l in enumerate(lens2))
    knz2 = kz.knz_assemble(chain, ent, bs, len(whole2), [out2[i * ostride:i * ostride + (res2[i].bits + 7) // 8].tobytes() for i in range(len(lens2))],
                           [r.bits for r in res2])
    r1, d = dev_decompress(ctx, knz2, len(lens2) * bs)
    assert r1 == len(whole2) and d[:r1].tobytes() == whole2


# ---- 7: faults ---------------------------------------------------------------------------------------------------------------------
def _same_verdict(ctx, bad, cap, tag, data=None):
    r0, h = host_decompress(ctx, bad, cap)
    r1, d = dev_decompress(ctx, bad, cap)
    assert r1 == r0, (tag, "device", r1, "host", r0)
    if r0 >= 0:
        assert d[:r0].tobytes() == h[:r0].tobytes(), (tag, "decoded bytes")
    return r0, d


@pytest.fixture(scope="module")
def small_stream(ctx):
    """three compressible 1 KiB blocks: a stream of well under 200 bytes"""
    bs = 1024
    data = np.frombuffer(b"ab" * 512 + b"cdc" * 341 + b"c" + b"efgh" * 256, dtype=np.uint8)
    rc, knz = host_compress(ctx, "BWT+RANK+ZRLT", "ANS0", bs, data)
    assert 0 < rc < 200, rc
    return bs, data, knz


def test_stream_header_faults(ctx, small_stream):
    bs, data, knz = small_stream
    for what, bad, code in refinputs.header_faults(knz):
        r0, _ = _same_verdict(ctx, bad, len(data), what)
        assert r0 == -code, (what, r0)


def test_truncation_at_every_byte(ctx, small_stream):
    bs, data, knz = small_stream
    codes = set()
    for cut in range(len(knz)):
        r0, _ = _same_verdict(ctx, knz[:cut], len(data), "cut %d" % cut)
        codes.add(r0)
    assert -15 in codes and len([c for c in codes if c < 0]) >= 3, codes       # no magic; a cut header; a cut prefix or payload


def test_length_prefix_faults(ctx, small_stream):
    bs, data, knz = small_stream
    idx = kz.knz_index(knz)
    for k in (0, 1, 2):
        off, w = idx["blocks"][k]
        pre = off - 5 - knzcases.lw(w)
        flips = [pre + i for i in range(5)] + [pre + 5, pre + 5 + knzcases.lw(w) // 2, off - 1]
        for bit in flips:
            bad = bytearray(knz)
            bad[bit >> 3] ^= 0x80 >> (bit & 7)
            _same_verdict(ctx, bytes(bad), len(data), "block %d bit %d" % (k, bit - pre))
        bad = bytearray(knz)
        refinputs.set_bits(bad, pre, 5, 31)                                    # a 34-bit length: the walk is sent far past the end
        r0, _ = _same_verdict(ctx, bytes(bad), len(data), "block %d lw 34" % k)
        assert r0 < 0
    bad = bytearray(knz)                                                      # no end marker: the last block's bits run to the last byte
    _same_verdict(ctx, bytes(bad[:-1]), len(data), "no end marker")


def test_block_header_fault_delivers_the_blocks_in_front(ctx):
    bs, chain, ent = 1024, "BWT+RANK+ZRLT", "ANS0"
    data = data_for(chain, bs)[:10 * bs + 5]
    rc, knz = host_compress(ctx, chain, ent, bs, data)
    idx = kz.knz_index(knz)
    for k in (0, 4, 9):
        for byte in range(3):                                                  # mode, length, and length or checksum: the shortest header
            off, w = idx["blocks"][k]
            bad = bytearray(knz)
            bit = off + 8 * byte + 3
            bad[bit >> 3] ^= 0x80 >> (bit & 7)
            r0, d = _same_verdict(ctx, bytes(bad), len(data), "block %d header byte %d" % (k, byte))
            assert r0 < 0, (k, byte, r0)
            assert d[:k * bs].tobytes() == data[:k * bs].tobytes(), (k, byte, "blocks in front")


def test_corrupted_streams(ctx):
    bs, chain, ent = 1024, "BWT+RANK+ZRLT", "ANS0"
    data = data_for(chain, bs)[:8 * bs + 100]
    rc, knz = host_compress(ctx, chain, ent, bs, data)
    verdicts = {}
    for kind in range(7):
        for seed in range(40):
            rng = np.random.default_rng(1000 * kind + seed)
            bad = refinputs.corrupt(rng, knz, kind)
            r0, _ = _same_verdict(ctx, bad, len(data) + bs, "kind %d seed %d" % (kind, seed))
            verdicts[min(r0, 0)] = verdicts.get(min(r0, 0), 0) + 1
    assert len(verdicts) >= 4, verdicts                                        # several different faults were met, and accepted streams


# ---- 8: more blocks than one launch of the block kernels takes ------------------------------------------------------------------
def test_66000_blocks(ctx):
    """66 000 blocks of 1 KiB under NONE&NONE, past the 65 535 blocks of one launch's grid.  Measured on an MI355X (one run, the
    calls alone): kz_compress_device 10 ms, kz_decompress_device 132 ms, knz_index_device 143 ms (the serial walk, about 2 us per
    block, and 66 000 Python tuples); kz_compress on the host 228 ms."""
    bs, nblk = 1024, 66000
    data = np.tile(datagen.stream(40, bs), nblk // 40)[:nblk * bs]
    data[::bs] = (np.arange(nblk) & 0xFF).astype(np.uint8)
    data[1::bs] = (np.arange(nblk) >> 8).astype(np.uint8)
    import torch
    clock = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t = time.time()
        r = fn()
        clock[name] = (time.time() - t) * 1e3
        return r

    rc0, want = timed("kz_compress", lambda: host_compress(ctx, "NONE", "NONE", bs, data))
    tsrc, p = up(data)
    cap = kz.compress_bound(len(data), bs)
    dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = timed("kz_compress_device", lambda: kz.compress_device(ctx, "NONE", "NONE", bs, p, len(data), dst.data_ptr() + 3, cap))
    assert rc == rc0 == len(want)
    assert torch.equal(dst[3:3 + rc].cpu(), torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()))
    idx = timed("knz_index_device", lambda: kz.knz_index_device(ctx, dst.data_ptr() + 3, rc))
    assert len(idx["blocks"]) == nblk and idx == kz.knz_index(want)
    back = torch.full((len(data) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rd = timed("kz_decompress_device", lambda: kz.decompress_device(ctx, dst.data_ptr() + 3, rc, back.data_ptr(), len(data)))
    assert rd == len(data)
    assert torch.equal(back[:rd].cpu(), torch.from_numpy(data)) and bool((back[rd:] == 0xA5).all())
    print("66000 blocks: " + ", ".join("%s %.0f ms" % kv for kv in clock.items()))


# ---- 9: it ran where it says -----------------------------------------------------------------------------------------------------------
def test_container_kernels_ran_and_the_host_stages_did_not(ctx):
    bs, chain, ent = 65536, "BWT+RANK+ZRLT", "ANS0"
    data = data_for(chain, bs)[:5 * bs + 9]
    L = ctx.lib
    fwd0, inv0 = L.kz_host_stage_blocks(0, 0), L.kz_host_stage_blocks(1, 0)
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        rc, got, _ = dev_compress(ctx, chain, ent, bs, data)
        rd, out = dev_decompress(ctx, got, len(data))
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    assert rd == len(data) and out.tobytes() == data.tobytes()
    for name in ("k_knz_pack", "k_knz_walk", "k_knz_unpack"):
        assert times.get(name, {}).get("launches", 0) > 0, (name, sorted(times))
    assert (L.kz_host_stage_blocks(0, 0), L.kz_host_stage_blocks(1, 0)) == (fwd0, inv0)


# ---- 10: tensor helpers ------------------------------------------------------------------------------------------------------------
def test_tensor_helpers(ctx):
    import torch
    g = torch.Generator().manual_seed(5)
    t = (torch.randn(300001, generator=g) * 4).round().div(4).cuda()            # float32 with few distinct values: compressible
    knz = kz.compress_tensor(ctx, t, block_size=65536)
    assert knz.dtype == torch.uint8 and knz.is_cuda and knz.numel() < t.numel() * 4
    assert knz.cpu().numpy().tobytes() == host_compress(ctx, "BWT+RANK+ZRLT", "ANS0", 65536, t.cpu().numpy().view(np.uint8))[1]
    back = kz.decompress_tensor(ctx, knz)
    assert back.dtype == torch.uint8 and torch.equal(back.cpu(), t.cpu().view(torch.uint8))
    base = torch.from_numpy(datagen.stream(3, 65536)).cuda()
    v = base[1:]                                                               # a uint8 view at storage offset 1
    assert v.storage_offset() == 1 and v.data_ptr() % 2 == 1
    knz = kz.compress_tensor(ctx, v, transform="LZ", entropy="HUFFMAN", block_size=65536, checksum=32)
    out = torch.empty(v.numel() + 7, dtype=torch.uint8, device="cuda")[7:]
    back = kz.decompress_tensor(ctx, knz.clone(), out=out)
    assert back.data_ptr() == out.data_ptr() and torch.equal(back.cpu(), v.cpu())
    with pytest.raises(ValueError):
        kz.compress_tensor(ctx, torch.zeros(4, 4, device="cuda").t())
