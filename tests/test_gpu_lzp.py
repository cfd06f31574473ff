"""LZP on the device against tests/lzpmodel.py (a restatement of LZCodec.LZPCodec, K/transform/LZCodec.java:973-1287): single blocks,
the seams of the window parse, dstEnd, damaged input, the block classes, batched calls, chains and streams.  Every expected byte
comes from the CPU model (or, for the four hand vectors, from the Java by hand), never from the device."""
import numpy as np
import pytest
import torch

import datagen
import katmodels
import kanzi_amd as kz
import lzpcases
import lzpmodel
import oracle
import refinputs

pytestmark = pytest.mark.gpu

W = 64                                        # positions per speculative window of k_lzp_fwd / k_lzp_inv (LZP_WINDOW, kz_lzp.hip)
FC, FE, FF = lzpcases.FC, lzpcases.FE, lzpcases.FF


@pytest.fixture(scope="module")
def ctx():
    return kz.Context(0)


def dev_forward(ctx, data, dst_len=None):
    dst_len = lzpmodel.max_encoded_length(len(data)) if dst_len is None else dst_len
    t = kz.LZPCodec(ctx)
    src = kz.SliceByteArray(np.frombuffer(data, dtype=np.uint8).copy())
    dst = kz.SliceByteArray(np.zeros(max(dst_len, 1), dtype=np.uint8))
    dst.length = dst_len
    ok = t.forward(src, dst)
    return ok, dst.array[:dst.index].tobytes()


def dev_inverse(ctx, data, dst_len):
    t = kz.LZPCodec(ctx)
    src = kz.SliceByteArray(np.frombuffer(data, dtype=np.uint8).copy())
    dst = kz.SliceByteArray(np.zeros(dst_len, dtype=np.uint8))
    ok = t.inverse(src, dst)
    return ok, dst.array[:dst.index].tobytes()


def check_forward(ctx, data, dst_len=None, tag=None, stats=None):
    data = bytes(data)
    want = lzpmodel.forward(data, dst_len, stats)
    got = dev_forward(ctx, data, dst_len)
    assert got[0] == want[0], (tag, len(data), dst_len, "verdict", got[0], want[0], len(got[1]), len(want[1]))
    if want[0]:
        assert len(got[1]) == len(want[1]) and got[1] == want[1], (tag, len(data), len(got[1]), len(want[1]))
    return want


def check_inverse(ctx, data, dst_len, tag=None, stats=None):
    want = lzpmodel.inverse(bytes(data), dst_len, stats)
    got = dev_inverse(ctx, bytes(data), dst_len)
    assert got[0] == want[0], (tag, len(data), dst_len, "verdict", got[0], want[0])
    if want[0]:
        assert got[1] == want[1], (tag, len(data), dst_len, len(got[1]), len(want[1]))
    return want


def check_both(ctx, data, tag=None, stats=None, istats=None, caps=(-1, 5000)):
    data = bytes(data)
    ok, out = check_forward(ctx, data, None, tag, stats)
    if ok and len(data):
        assert check_inverse(ctx, out, len(data), tag, istats) == (True, data), tag
        for extra in caps:                                       # one byte short fails (:1227-1228), room to spare changes nothing
            check_inverse(ctx, out, len(data) + extra, tag)
    return ok, out


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------
def test_hand_vectors_band_and_collision(ctx):
    for lab, data, want in lzpcases.hand_vectors():
        assert dev_forward(ctx, data) == (True, want), lab
        assert check_both(ctx, data, lab) == (True, want)
    a, b = lzpcases.band_pair()
    assert check_both(ctx, a, "band67")[0] is True and check_both(ctx, b, "band66")[0] is False
    ok, out = check_both(ctx, lzpcases.collision_block(True), "foreign entry")
    assert ok and out[304:306] == FC + FF
    ok, out = check_both(ctx, lzpcases.collision_block(False), "empty slot")
    assert ok and out[304] == 0xFC and out[305] != 0xFF
    # the destination rule (:1034-1035) and the smallest block (:1038-1039)
    for n, cap in ((5000, 5077), (5000, 5078), (1024, 1039), (1024, 1040)):
        check_forward(ctx, bytes(n), cap, ("cap", n, cap))


def test_reference_inputs(ctx):
    counts = []
    for items in (refinputs.transform_inputs(), refinputs.edge_inputs()):
        n_ok = 0
        for i, d in enumerate(items):
            n_ok += check_both(ctx, bytes(d), ("ref", i), caps=(-1, 5000) if len(d) <= (256 << 10) else ())[0] and len(d) > 0
        counts.append(n_ok)
    assert counts == [45, 5]


def test_damaged_input(ctx):
    fails = 0
    for lab, coded, dst_len in lzpcases.damaged_inputs():
        fails += not check_inverse(ctx, coded, dst_len, lab)[0]
    assert fails >= 14
    esc = lzpmodel.forward(FC * 5000)[1]
    for cap in (5000, 4999, 4998, 4997):                         # an escape and a literal at dstEnd (:1187-1188, :1203-1204)
        check_inverse(ctx, esc, cap, ("esc", cap))
    for d in (b"abcdef", b"abcdefg", FC * 9, b"abcd" + FC + FF, b"abcd" + FC + FE, b"abcd" + FC + b"\x00"):
        for cap in (len(d), len(d) + 1, 100):
            check_inverse(ctx, d, cap, (d, cap))


def test_fuzz_blocks(ctx):
    fwd, inv = lzpmodel.new_stats(), lzpmodel.new_stats()
    for seed in range(6):
        assert check_both(ctx, lzpcases.fuzz_block(seed), ("fuzz", seed), fwd, inv)[0]
    assert min(fwd[k] for k in ("matches", "chained", "fc_escaped", "fc_plain", "fc_escaped_near", "fc_plain_near")) >= 20
    assert inv["overlapping"] >= 20 and inv["matches"] > inv["overlapping"]


# ---- sizes and ends ----------------------------------------------------------------------------------------------------------------
def test_sizes(ctx):
    """the tail loop covers the last 64 positions: 128 is the smallest block, 129 the first with a position that may match, 192 / 193
    put one window's end on the seam between the two loops"""
    rng = np.random.default_rng(3)
    applied = 0
    for n in (0, 1, 4, 127, 128, 129, 191, 192, 193):
        small = bytes(rng.choice(np.array([0x41, 0xFC], dtype=np.uint8), n))
        for lab, d in (("zeros", bytes(n)), ("flags", FC * n), ("noise", lzpcases.noise(n, n)), ("two", small), ("abc", (b"abc" * 70)[:n])):
            applied += check_both(ctx, d, (lab, n))[0] and n > 0
            for cap in sorted({n, n + 1, n + 64, max(n - 1, 1)} if n else ()):  # the same bytes as CODED input of that count
                check_inverse(ctx, d, cap, (lab, n, cap))
    assert applied >= 12
    assert dev_inverse(ctx, b"abc", 16)[0] is False and dev_inverse(ctx, b"abcd", 16) == (True, b"abcd")
    assert dev_forward(ctx, b"") == (True, b"") and dev_inverse(ctx, b"", 4) == (True, b"")


def test_match_ends(ctx):
    """findMatch steps 8 bytes while bestLen + 8 <= srcEnd - srcIdx: a match that runs to the block's end is cut to whole steps"""
    sizes = set()
    for n in (1000, 1003):
        for k in range(10):
            ok, out = check_both(ctx, lzpcases.match_to_end(k, n), ("end", n, k))
            assert ok
            sizes.add((n, len(out)))
    assert len(sizes) >= 12


def test_match_lengths(ctx):
    for extra, code in ((0, b"\x00"), (253, b"\xfd"), (254, FE + b"\x00"), (507, FE + b"\xfd"), (508, FE + FE + b"\x00")):
        d = lzpcases.planted(3000, 70 + extra, 2000, 500, 64 + extra)
        ok, out = check_both(ctx, d, ("len", extra))
        assert ok and out == d[:2000] + FC + code + d[2000 + 64 + extra:]
    d = lzpcases.planted(3000, 5, 2000, 500, 63)                 # one byte short of a match: every byte a literal, declined
    assert check_both(ctx, d, "len63")[0] is False


# ---- window seams ------------------------------------------------------------------------------------------------------------------
def test_first_match_at_every_offset(ctx):
    """the first match on every lane of the first two windows (position 4 cannot match: the table is empty there)"""
    for at in range(5, 4 + 2 * W + 1):
        d = lzpcases.match_at(at)
        ok, out = check_both(ctx, d, ("at", at))
        assert ok and out[:at] == d[:at] and out[at] == 0xFC


def test_late_match_on_every_lane(ctx):
    st = lzpmodel.new_stats()
    for off in range(2 * W):
        assert check_both(ctx, lzpcases.late_match(off), ("late", off), st)[0]
        assert check_both(ctx, lzpcases.late_match(off, 6), ("late fc", off), st)[0]
    assert st["matches"] == 4 * W and st["fc_escaped"] >= 2 * W and st["fc_plain"] >= 2 * W


def test_runs_and_periods(ctx):
    st = lzpmodel.new_stats()
    ok, out = check_both(ctx, lzpcases.broken_runs(), "runs", st)
    assert ok and st["matches"] == 1 and st["fc_escaped"] > 500 and st["fc_plain"] > 50
    assert check_both(ctx, lzpcases.broken_runs(False), "runs, declined")[0] is False
    inv = lzpmodel.new_stats()
    for p in (1, 2, 3, 63, 64, 65):
        for flag in (False, True):
            assert check_both(ctx, lzpcases.periodic(p, flag=flag), ("period", p, flag), None, inv)[0]
            assert check_both(ctx, lzpcases.noise(500, p) + lzpcases.periodic(p, 2000 + p, flag), ("period behind noise", p, flag), None, inv)[0]
    assert inv["overlapping"] == inv["matches"] == 24


def test_dst_end(ctx):
    for lab, d in lzpcases.dst_end_cases():
        ok, out = check_forward(ctx, d, None, lab)
        n = len(d)
        assert not ok and len(out) == n - (n >> 6), lab
        assert lab == "literal" or out[-1:] == {"escape": FC, "chain": FE}[lab]     # where the model stopped


# ---- block classes -----------------------------------------------------------------------------------------------------------------
def _classes(n):
    blocks = [(str(c), datagen.block(c, n).tobytes()) for c in range(5)]
    blocks.append(("exe", bytes(datagen.exe_like(n, 1))))
    blocks.append(("sensor", bytes(datagen.sensor_like(n, 1))))
    return blocks


def test_block_classes_256k(ctx):
    got = {}
    for name, b in _classes(256 << 10):
        ok, out = check_both(ctx, b, name)
        got[name] = len(out) if ok else None
    assert got == {"0": None, "1": None, "2": None, "3": None, "4": None, "exe": 144187, "sensor": None}
    assert check_both(ctx, datagen.block(4, 4096).tobytes(), "class 4, 4 KiB")[0] is True
    assert len(check_both(ctx, bytes(datagen.exe_like(64 << 10, 1)), "exe 64 KiB")[1]) == 53342


def test_exe_like_4m(ctx):
    ok, out = check_both(ctx, bytes(datagen.exe_like(4 << 20, 1)), "exe 4 MiB")
    assert ok and len(out) == 3320453


# ---- batched calls -----------------------------------------------------------------------------------------------------------------
def _batch(blocks, bs=None):
    bs = bs or max(len(b) for b in blocks)
    inp = np.zeros((len(blocks), bs), dtype=np.uint8)
    lens = np.zeros(len(blocks), dtype=np.int32)
    for i, b in enumerate(blocks):
        inp[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[i] = len(b)
    return inp, lens, bs


def _forty_blocks(seed):
    """about 40 blocks of one shape (the same lengths for every seed): empty, under 16, under 128, applying and declining"""
    rng = np.random.default_rng(seed)
    lengths = [0, 7, 15, 16, 100, 127, 128, 129, 192, 193, 500, 1000, 4096, 4097, 9000, 20000, 30000]
    blocks = []
    for i in range(40):
        n = lengths[i % len(lengths)] + (i // len(lengths))
        kind = (i // 2 + seed) % 4
        if kind == 0:
            b = lzpcases.noise(n, 100 * seed + i)                                    # declines
        elif kind == 1:
            b = (lzpcases.noise(97, 100 * seed + i, ()) * (n // 97 + 1))[:n]         # periodic: applies from 128 bytes on
        elif kind == 2:
            b = lzpcases.fuzz_block(100 * seed + i, max(n, 8000))[:n]
        else:
            b = np.repeat(rng.choice(np.array([0, 7, 0xFC], dtype=np.uint8), n // 150 + 1), 150)[:n].tobytes()   # runs of 150
        blocks.append(b)
    return blocks


def _model_chain(block, names):
    """(skip flags, bytes behind the last stage) of Sequence.forward over the CPU models; BWT comes from the oracle"""
    n = len(block)
    if n == 0:
        return 0xFF, b""
    if n <= 15:
        return 0x7F, bytes(block)                                # a copy block: the one stage is NONE
    skip, cur = 0xFF, bytes(block)
    for i, name in enumerate(names):
        if name == "LZP":
            ok, out = lzpmodel.forward(cur)
        elif name == "BWT":
            ok, out = oracle.transform_forward("BWT", cur)
        elif name == "RANK":
            ok, out = True, katmodels.sbrt_forward(cur, 2)
        elif name == "ZRLT":
            ok, out = katmodels.zrlt_forward(cur)
        else:
            raise ValueError(name)
        if ok:
            skip &= ~(1 << (7 - i)) & 0xFF
            cur = bytes(out)
    return skip, cur


def _check_lzp_batch(blocks, res, out, bs):
    applied = declined = 0
    for i, b in enumerate(blocks):
        skip, cur = _model_chain(b, ["LZP"])
        assert res[i].status == 0 and res[i].skipFlags == skip and res[i].length == len(cur), (i, len(b), res[i].skipFlags, skip, res[i].length, len(cur))
        if len(b) > 15:
            applied += not (skip & 0x80)
            declined += bool(skip & 0x80)
        if len(b) and res[i].bits == 8 * (res[i].bits // 8) and not (res[i].mode & 0x80):   # entropy NONE: the stage's bytes end the stream
            end = res[i].bits // 8
            assert out[i, end - len(cur):end].tobytes() == cur, (i, len(b))
    return applied, declined


def test_batched_calls(ctx):
    ctx.reset()
    for seed, form in ((1, "sync"), (2, "sync"), (3, "submit"), (1, "submit")):
        blocks = _forty_blocks(seed)
        inp, lens, bs = _batch(blocks, 30002)
        ostride = kz.max_block_stream_bytes(bs)
        out = np.zeros((len(blocks), ostride), dtype=np.uint8)
        if form == "sync":
            res = kz.encode_blocks(ctx, "LZP", "NONE", inp, bs, lens, out, ostride)
        else:
            job = kz.submit_encode_blocks(ctx, "LZP", "NONE", inp, bs, lens, out, ostride)
            res = job.wait()
        applied, declined = _check_lzp_batch(blocks, res, out, bs)
        assert applied >= 8 and declined >= 8, (seed, form, applied, declined)
        bits = np.array([r.bits for r in res], dtype=np.int64)
        dec = np.zeros((len(blocks), bs), dtype=np.uint8)
        if form == "sync":
            res2 = kz.decode_blocks(ctx, "LZP", "NONE", bs, out, ostride, bits, dec, bs)
        else:
            res2 = kz.submit_decode_blocks(ctx, "LZP", "NONE", bs, out, ostride, bits, dec, bs).wait()
        for i, b in enumerate(blocks):
            assert res2[i].status == 0 and res2[i].length == len(b) and dec[i, :len(b)].tobytes() == b, (seed, form, i)
    # device memory
    blocks = _forty_blocks(4)
    inp, lens, bs = _batch(blocks, 30002)
    ostride = kz.max_block_stream_bytes(bs)
    d_in = torch.from_numpy(inp).cuda()
    d_out = torch.zeros((len(blocks), ostride), dtype=torch.uint8, device="cuda")
    res = kz.encode_blocks(ctx, "LZP", "NONE", d_in.data_ptr(), bs, lens, d_out.data_ptr(), ostride, kz.MEM_DEVICE)
    _check_lzp_batch(blocks, res, d_out.cpu().numpy(), bs)


# ---- chains and streams ------------------------------------------------------------------------------------------------------------
def _chain_blocks():
    return [bytes(datagen.exe_like(30000, 1)), lzpcases.fuzz_block(3, 28111), datagen.block(3, 30000).tobytes()[100:], datagen.block(0, 17000).tobytes(),
            b"0123456789abcde", lzpcases.periodic(65, 9000, True), b"xy" * 20, bytes(20000), (b"line of text %d\n" * 900) % tuple(range(900))]


@pytest.mark.parametrize("chain", ["LZP+ZRLT", "BWT+LZP", "LZP+BWT+RANK+ZRLT"])
def test_chains(ctx, chain):
    ctx.reset()
    names = chain.split("+")
    blocks = _chain_blocks()
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, chain, "ANS0", inp, bs, lens, out, ostride)
    k = names.index("LZP")
    lzp_flags = []
    for i, b in enumerate(blocks):
        skip, cur = _model_chain(b, names)
        assert res[i].status == 0 and res[i].skipFlags == skip and res[i].length == len(cur), (chain, i, hex(res[i].skipFlags), hex(skip), res[i].length, len(cur))
        if len(b) > 15:
            lzp_flags.append(bool(skip & (0x80 >> k)))
    assert any(lzp_flags) and not all(lzp_flags)                 # LZP accepted some blocks and declined others
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(blocks), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, chain, "ANS0", bs, out, ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert res2[i].status == 0 and res2[i].length == len(b) and dec[i, :len(b)].tobytes() == b, (chain, i)
    out2 = np.zeros_like(out)
    res3 = kz.submit_encode_blocks(ctx, chain, "ANS0", inp, bs, lens, out2, ostride).wait()
    for i in range(len(blocks)):
        assert res3[i].bits == res[i].bits and out2[i, :(res[i].bits + 7) // 8].tobytes() == out[i, :(res[i].bits + 7) // 8].tobytes(), (chain, i)
    dec2 = np.zeros_like(dec)
    kz.submit_decode_blocks(ctx, chain, "ANS0", bs, out, ostride, bits, dec2, bs).wait()
    assert np.array_equal(dec2, dec)
    # the stream calls: three blocks, the last one short
    sbs = 64 << 10
    data = bytes(datagen.exe_like(sbs, 2)) + datagen.block(3, sbs).tobytes() + lzpcases.fuzz_block(9, 20000)
    cos = kz.CompressedOutputStream(ctx, chain, "ANS0", sbs)
    cos.write(data)
    cos.close()
    idx = kz.knz_index(cos.output)
    assert idx["transform"] == kz.transform_type(chain) and len(idx["blocks"]) == 3
    assert kz.CompressedInputStream(ctx, cos.output).read() == data
    ctx.reset()
    ctx.set_block_size(sbs)
    parts = [data[0:sbs], data[sbs:2 * sbs], data[2 * sbs:]]
    inp, lens, _ = _batch(parts, sbs)
    ostride = kz.max_block_stream_bytes(sbs)
    out = np.zeros((3, ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, chain, "ANS0", inp, sbs, lens, out, ostride)
    for i, (off, nbits) in enumerate(idx["blocks"]):
        assert nbits == res[i].bits and res[i].skipFlags == _model_chain(parts[i], names)[0], (chain, i)
        assert kz.extract_bits(cos.output, off, nbits) == out[i, :(nbits + 7) // 8].tobytes(), (chain, i)
    ctx.reset()


def test_what_stays_refused(ctx):
    ctx.reset()
    blocks = _chain_blocks()[:3]
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    ctx.set_block_size(bs)
    with pytest.raises(kz.KanziError) as e:
        kz.encode_blocks(ctx, "LZP+TEXT", "NONE", inp, bs, lens, out, ostride)
    assert "host stages in front of the GPU stages" in str(e.value)
    with pytest.raises(kz.KanziError) as e:
        kz.level_chain(7)                                        # LZP+TEXT+UTF+BWT+LZP&CM: CM is not built
    assert e.value.code == 3
    ctx.reset()
