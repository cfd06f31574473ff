"""EXE on the device against tests/exemodel.py (a restatement of K/transform/EXECodec.java, bitstream >= 3): the hand vectors, sizes and
data-type tags, events planted at the seams of the stage's passes, runs that chain across them, the verdict's edges, ARM64, every
header builder, damaged input behind a guard, a seeded fuzz, batched calls, chains and streams.  Every expected byte comes from the
CPU model, never from the device."""
import ctypes
import struct

import numpy as np
import pytest

import datagen
import exemodel
import execases
import kanzi_amd as kz
from layouthelp import FILLS, Frame, assert_guards

pytestmark = pytest.mark.gpu

S = 16                                        # bytes per thread strip (EX_PER, kz_exe.hip)
T = 256 * S                                   # bytes per tile (EX_TILE)
ROW = 64 * S                                  # bytes per wave of a tile
DT_NAMES = {v: k for k, v in kz.DATA_TYPES.items()}


@pytest.fixture(scope="module")
def ctx():
    return kz.Context(0)


def dev_forward(ctx, data, data_type="UNDEFINED", dst_len=None):
    dst_len = exemodel.max_encoded_length(len(data)) if dst_len is None else dst_len
    ctx.set_data_type(data_type)
    t = kz.EXECodec(ctx)
    src = kz.SliceByteArray(np.frombuffer(data, dtype=np.uint8).copy())
    dst = kz.SliceByteArray(np.zeros(max(dst_len, 1), dtype=np.uint8))
    dst.length = dst_len
    ok = t.forward(src, dst)
    after = DT_NAMES[ctx.get_data_type()]
    ctx.set_data_type(0)
    return ok, dst.array[:dst.index].tobytes(), after


def dev_inverse(ctx, data, dst_len):
    t = kz.EXECodec(ctx)
    src = kz.SliceByteArray(np.frombuffer(data, dtype=np.uint8).copy())
    dst = kz.SliceByteArray(np.zeros(max(dst_len, 1), dtype=np.uint8)[:dst_len])
    ok = t.inverse(src, dst)
    return ok, dst.array[:dst.index].tobytes()


def check_forward(ctx, data, data_type="UNDEFINED", dst_len=None, tag=None, stats=None):
    data = bytes(data)
    want = exemodel.forward(data, data_type, dst_len, stats)
    got = dev_forward(ctx, data, data_type, dst_len)
    assert got[0] == want[0], (tag, len(data), dst_len, "verdict", got[0], want[0], len(got[1]), len(want[1]))
    assert got[2] == want[2], (tag, "data type", got[2], want[2])
    if want[0]:
        assert got[1][:9] == want[1][:9], (tag, "header", got[1][:9].hex(), want[1][:9].hex())
        if got[1] != want[1]:
            at = next((i for i in range(min(len(got[1]), len(want[1]))) if got[1][i] != want[1][i]), -1)
            assert False, (tag, len(data), len(got[1]), len(want[1]), "first difference", at, got[1][max(at - 4, 0):at + 8].hex(), want[1][max(at - 4, 0):at + 8].hex())
    return want


def check_inverse(ctx, data, dst_len, tag=None, stats=None):
    want = exemodel.inverse(bytes(data), dst_len, stats)
    if dst_len <= 0:
        return want                                              # (the mirror refuses an empty output array before the library sees it)
    got = dev_inverse(ctx, bytes(data), dst_len)
    assert got[0] == want[0], (tag, len(data), dst_len, "verdict", got[0], want[0])
    if want[0] and got[1] != want[1]:
        at = next((i for i in range(min(len(got[1]), len(want[1]))) if got[1][i] != want[1][i]), -1)
        assert False, (tag, len(data), dst_len, len(got[1]), len(want[1]), "first difference", at, got[1][max(at - 4, 0):at + 8].hex(), want[1][max(at - 4, 0):at + 8].hex())
    return want


def check_both(ctx, data, tag=None, stats=None, istats=None, caps=(-1, 5000), data_type="UNDEFINED", round_trip=True):
    """forward against the model; its output through the inverse at len, len - 1 and with room.  inverse(forward(x)) == x is asserted
    where the model's own round trip holds (round_trip=False: ARM64 with an unaligned codeStart)"""
    data = bytes(data)
    ok, out, _ = check_forward(ctx, data, data_type, None, tag, stats)
    if ok and len(data):
        back = check_inverse(ctx, out, len(data), tag, istats)
        if round_trip:
            assert back == (True, data), tag
        for extra in caps:
            check_inverse(ctx, out, len(data) + extra, tag)
    return ok, out


# ---- 1, 2, 3: vectors, sizes, tags ------------------------------------------------------------------------------------------------
def test_hand_vectors(ctx):
    res = {lab: check_both(ctx, blk, lab) for lab, blk in execases.hand_vectors()}
    assert res["hand"][0] and len(res["hand"][1]) == 4105 and res["hand"][1][:9].hex() == "400000000009100000"
    assert res["hand"][1][73:78].hex() == "e8f0f0f0a0" and res["hand"][1][105:110].hex() == "e8f0f0f0b0"
    assert not res["15-calls"][0]
    assert res["boundary"][0] and res["boundary"][1][:9].hex() == "400000000008100000"
    assert res["escapes"][0] and res["escapes"][1][2009:2017].hex() == "9b9b9be800000007"


def test_sizes_and_destination(ctx):
    full = bytes(execases.hand_block(4200, 20))
    assert check_both(ctx, full[:4096], 4096)[0] is True
    assert check_both(ctx, full[:4095], 4095)[0] is False        # :119
    for n in (4096, 4200):
        cap = exemodel.max_encoded_length(n)
        assert check_forward(ctx, full[:n], dst_len=cap, tag=("cap", n))[0] is True
        assert check_forward(ctx, full[:n], dst_len=cap - 1, tag=("cap-1", n))[0] is False       # :127
        assert check_forward(ctx, full[:n], dst_len=cap + 1000, tag=("cap+", n))[0] is True
    assert dev_forward(ctx, b"")[:2] == (True, b"") and dev_inverse(ctx, b"", 4) == (True, b"")
    for n in (1, 8, 9, 100, 4000):
        assert check_forward(ctx, full[:n], tag=n)[0] is False
    assert int(ctx.lib.kz_transform_max_encoded_len(kz.EXE_TYPE, 256)) == 288 and int(ctx.lib.kz_transform_max_encoded_len(kz.EXE_TYPE, 4096)) == 4608


def test_data_type_tags(ctx):
    taken = []
    x = execases.x86_like(4096, 2)
    for name in kz.DATA_TYPES:
        ok, _, after = check_forward(ctx, x, name, tag=name)
        if ok:
            taken.append(name)
            assert after == "EXE"
        else:
            assert after == name
        assert check_forward(ctx, bytes(5000), name, tag=("declined", name))[2] == name          # a declined block leaves the tag alone
    assert sorted(taken) == ["BIN", "EXE", "UNDEFINED"]


# ---- 4: events at the seams of the passes -----------------------------------------------------------------------------------------
def _positions(n, code_end):
    pos = set()
    for c in (T, S, 64):
        pos |= set(range(c - 7, c + 8))
    pos |= set(range(code_end - 7, code_end))
    return sorted(p for p in pos if 0 <= p < n)


@pytest.mark.parametrize("kind", ["call", "jcc", "fp", "9b", "of9b", "of38", "nested", "nested9b"])
def test_planted_events(ctx, kind):
    key = {"call": "calls", "jcc": "jcc", "fp": "false_positive", "9b": "escaped_9b", "of9b": "of_9b", "of38": "of_plain", "nested": "calls",
           "nested9b": "calls"}[kind]
    n = 2 * T
    hits = bounds = 0
    for code_end in (n, T + 1000):
        for p in _positions(n, code_end):
            header = p >= 128                                    # below: no header to overwrite, the heuristic takes the block
            if not header and code_end != n:
                continue
            blk = execases.planted(kind, p, n, 5, None if code_end == n else code_end, header)
            base = execases.planted("none", p, n, 5, None if code_end == n else code_end, header)
            st, st0 = exemodel.new_stats(), exemodel.new_stats()
            exemodel.forward(base, stats=st0)
            ok, _ = check_both(ctx, blk, (kind, p, code_end), st, caps=(-1,))
            assert ok, (kind, p, code_end)
            hits += st[key] > st0[key]                              # the event was parsed as what it is meant to be
            bounds += st["boundary"]
    assert hits >= 30 and (bounds >= 1 or kind == "9b"), (kind, hits, bounds)


# ---- 5: chains of 0F / E8, and the heuristic's threshold --------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0x0F, 0xE8])
def test_runs_across_strip_row_and_tile(ctx, byte):
    n = 2 * T
    verdicts = set()
    for length in range(1, 131):
        b = bytearray(execases.x86_like(n, 6))
        for seam in (40 * S, 2 * ROW, T):                        # a strip's, a wave row's and a tile's first byte
            at = seam - (length + 1) // 2
            b[at:at + length] = bytes([byte]) * length
        for header in (True, False):                             # with a header; through the heuristic (the skip automaton sees the runs)
            blk = execases.elf_block(bytes(b)) if header else bytes(b)
            verdicts.add(check_both(ctx, blk, (byte, length, header), caps=())[0])
    assert True in verdicts


def test_heuristic_threshold(ctx):
    modes = []
    for lab, blk in execases.threshold_blocks():
        mode = exemodel.detect_type(blk)[0]
        ok, out, _ = check_forward(ctx, blk, tag=lab)
        modes.append(mode)
        assert ok == (mode == exemodel.X86), (lab, ok, hex(mode))     # (at the threshold the block has well over 16 matches)
    assert modes[0] == exemodel.X86 and modes[1] & exemodel.NOT_EXE
    for n in (4096, 65536):
        assert check_forward(ctx, bytes(datagen.exe_like(n, 1)), tag=("exe_like", n))[0] is False
    # filters one at a time (:751, :760).  Too few FF bytes and too few zeros keep the table of all byte values, so the block is still
    # BIN and the histogram filter is what declines it; with one byte value missing (the random bytes alone hold all 256: taking the
    # table away would not do) detectSimpleType says UNDEFINED
    x = execases.x86_like(8192, 4)
    BIN, UNDEF = exemodel.DT_ORDINAL["BIN"], exemodel.DT_ORDINAL["UNDEFINED"]
    for lab, blk, dt in (("few-ff", x[:-256].replace(b"\xff", b"\xfe") + x[-256:], BIN), ("few-zeros", x[:-256].replace(b"\x00", b"\x21") + x[-256:], BIN),
                         ("no-77", x.replace(b"\x77", b"\x78"), UNDEF)):
        assert exemodel.detect_type(blk)[0] == exemodel.NOT_EXE | dt, lab
        assert check_forward(ctx, blk, tag=lab)[0] is False


# ---- 6: the verdict's edges ---------------------------------------------------------------------------------------------------------
def test_match_count_and_expansion_edges(ctx):
    for calls, want in ((15, False), (16, True), (17, True)):
        assert check_both(ctx, bytes(execases.hand_block(4096, calls)), ("calls", calls))[0] is want
    for k, want in ((71, True), (72, True), (73, False), (74, False)):       # 9 + 4096 + k against 4096 + 81
        assert check_both(ctx, execases.expansion_block(k), ("expansion", k))[0] is want


# ---- 7: ARM64 -----------------------------------------------------------------------------------------------------------------------
def test_arm64(ctx):
    st, ist = exemodel.new_stats(), exemodel.new_stats()
    for n in (4096, 4099, 3 * T + 5):
        assert check_both(ctx, execases.arm64_like(n, 1), ("arm64_like", n), st, ist)[0]
    assert st["arm_bl"] >= 100 and st["arm_escape"] >= 20 and ist["inv_arm_escape"] == st["arm_escape"]
    # escapes at the tile seams: the words around them aim at address 0 and below
    n = 3 * T
    b = bytearray(execases.arm64_like(n, 2))
    for p in (T - 8, T - 4, T, T + 4, 2 * T - 4, 2 * T, ROW - 4, ROW, S * 9, S * 9 + 4):
        b[p:p + 4] = struct.pack("<I", 0x94000000 | ((-(p // 4) - (p // 8 % 2)) & 0x3FFFFFF))
    st2 = exemodel.new_stats()
    assert check_both(ctx, bytes(b), "seam escapes", st2)[0] and st2["arm_escape"] >= 10
    # codeStart and codeEnd from an ELF header: aligned, unaligned (the reference's own round trip does not hold there), the last
    # word cut by codeEnd
    arm = execases.arm64_like(2 * T, 3)
    for start, size, rt in ((0x400, 0x1800, True), (0x400, 0x17FE, True), (0x400, 0x1801, True), (0x402, 0x1BFD, False), (0x401, 0x1B03, False), (0x403, 0x1B01, False)):
        shifted = arm[:start] + arm[start & ~3:len(arm) - (start & 3)]
        blk = execases.elf_block(shifted, 64, False, [(1, start, size)], machine=0xB7)
        ok, out = check_both(ctx, blk, ("elf arm64", start, size), round_trip=rt)
        assert ok and struct.unpack("<i", out[1:5])[0] == start
        assert exemodel.inverse(out, len(blk)) == (True, blk) if rt else exemodel.inverse(out, len(blk))[1] != blk


# ---- 8: headers -----------------------------------------------------------------------------------------------------------------------
def test_header_builders(ctx):
    taken = 0
    for lab, blk, want in execases.header_cases():
        mode, cs, ce, _ = exemodel.detect_type(blk)
        if want is not None:
            assert (mode, cs, ce) == want, lab
        ok, out = check_both(ctx, blk, lab, caps=(-1,), round_trip="unaligned" not in lab)
        if ok:
            taken += 1
            assert out[0] == mode and struct.unpack("<i", out[1:5])[0] == cs, lab
            assert 9 + cs <= struct.unpack("<i", out[5:9])[0] <= len(out), lab
    assert taken >= 30


# ---- 9: damaged input ---------------------------------------------------------------------------------------------------------------
def test_damaged_inputs_stay_inside_dst(ctx):
    fails = total = 0
    for i, (lab, coded, dst_len) in enumerate(execases.damaged_inputs()):
        want = exemodel.inverse(coded, dst_len)
        if len(coded) == 0:
            continue
        total += 1
        fails += not want[0]
        src = np.frombuffer(coded, dtype=np.uint8).copy()
        dst = Frame(dst_len, FILLS[i % 3], False, guard=4096)
        p = ctypes.c_int32(0)
        rc = ctx.lib.kz_transform_inverse(ctx.h, kz.EXE_TYPE, src.ctypes.data, len(coded), dst.ptr(0), dst_len, ctypes.addressof(p))
        assert rc == (1 if want[0] else 0), (lab, rc, want[0], ctx.error())
        assert_guards(dst, lab)
        if want[0]:
            assert bytes(dst.rows(0, dst_len, 1, dst_len)[0][:p.value]) == want[1], lab
    assert 3 * fails >= total and fails < total, (fails, total)


# ---- 10: fuzz -------------------------------------------------------------------------------------------------------------------------
def test_fuzz_blocks(ctx):
    fwd, inv = exemodel.new_stats(), exemodel.new_stats()
    sizes = (4096, 5000, T + 1, 2 * T - 1, 30011, 65536)
    for seed, n in enumerate(sizes):
        assert check_both(ctx, execases.x86_like(n, 20 + seed), ("x86_like", seed, n), fwd, inv)[0]
    assert min(fwd[k] for k in ("calls", "jcc", "false_positive", "escaped_9b", "of_plain")) >= 20, fwd
    assert inv["inv_calls"] == fwd["calls"] + fwd["jcc"] and inv["inv_escapes"] == fwd["false_positive"] + fwd["escaped_9b"] + fwd["of_9b"]
    for seed, n in enumerate((4096, 2 * T + 3, 65536)):
        assert check_both(ctx, execases.arm64_like(n, 30 + seed), ("arm64_like", seed, n), fwd, inv)[0]
    assert fwd["arm_bl"] >= 100 and fwd["arm_escape"] >= 20


# ---- batched calls, chains, streams ---------------------------------------------------------------------------------------------------
def _batch(blocks, bs=None):
    bs = max(len(b) for b in blocks) if bs is None else bs
    inp = np.zeros((len(blocks), bs), dtype=np.uint8)
    lens = np.zeros(len(blocks), dtype=np.int32)
    for i, b in enumerate(blocks):
        inp[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[i] = len(b)
    return inp, lens, bs


def _writer_tag(block):
    """the writer's per-block tag from the first four bytes (none of these blocks starts like a compressed or multimedia file)"""
    return "EXE" if exemodel.magic_type(block) else "UNDEFINED"


def _mixed_blocks():
    hdr = [blk for lab, blk, _ in execases.header_cases() if lab in ("elf64le-3", "pe-good", "macho64", "elf-arm64", "elf-unknown-machine")]
    return [execases.x86_like(4096, 1), bytes(datagen.exe_like(30000, 1)), execases.arm64_like(20000, 2), b"", b"0123456789abcde", bytes(20000),
            execases.x86_like(30001, 3), bytes(execases.hand_block()), bytes(execases.hand_block(4096, 15)), execases.x86_like(4095, 4),
            (b"line of text %d\n" * 900) % tuple(range(900)), execases.arm64_like(4096, 5)] + hdr


def test_batched_calls(ctx):
    ctx.reset()
    blocks = _mixed_blocks()
    inp, lens, bs = _batch(blocks, 30002)
    ostride = kz.max_block_stream_bytes(bs)
    for form in ("sync", "submit"):
        out = np.zeros((len(blocks), ostride), dtype=np.uint8)
        if form == "sync":
            res = kz.encode_blocks(ctx, "EXE", "NONE", inp, bs, lens, out, ostride)
        else:
            res = kz.submit_encode_blocks(ctx, "EXE", "NONE", inp, bs, lens, out, ostride).wait()
        applied = declined = 0
        for i, b in enumerate(blocks):
            ok, cur, _ = exemodel.forward(b, _writer_tag(b)) if len(b) > 15 else (False, b, None)
            cur = cur if ok else b
            skip = 0xFF if len(b) == 0 else (0x7F if (ok or len(b) <= 15) else 0xFF)
            assert res[i].status == 0 and res[i].skipFlags == skip and res[i].length == len(cur), (form, i, len(b), hex(res[i].skipFlags), hex(skip), res[i].length, len(cur))
            applied += ok
            declined += (not ok) and len(b) > 15
            if len(b) and res[i].bits % 8 == 0 and not (res[i].mode & 0x80):
                end = res[i].bits // 8
                assert out[i, end - len(cur):end].tobytes() == cur, (form, i, len(b))
        assert applied >= 8 and declined >= 4, (applied, declined)
        bits = np.array([r.bits for r in res], dtype=np.int64)
        dec = np.zeros((len(blocks), bs), dtype=np.uint8)
        if form == "sync":
            res2 = kz.decode_blocks(ctx, "EXE", "NONE", bs, out, ostride, bits, dec, bs)
        else:
            res2 = kz.submit_decode_blocks(ctx, "EXE", "NONE", bs, out, ostride, bits, dec, bs).wait()
        for i, b in enumerate(blocks):
            assert res2[i].status == 0 and res2[i].length == len(b) and dec[i, :len(b)].tobytes() == b, (form, i)


@pytest.mark.parametrize("chain,ent", [("EXE+LZX", "HUFFMAN"), ("EXE+BWT+RANK+ZRLT", "ANS0"), ("TEXT+UTF+EXE+PACK+MM+LZX", "HUFFMAN")])
def test_chains_and_streams(ctx, chain, ent):
    ctx.reset()
    k = chain.split("+").index("EXE")
    blocks = _mixed_blocks()
    inp, lens, bs = _batch(blocks, 30016)                         # (a block size is a multiple of 16)
    ctx.set_block_size(bs)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, chain, ent, inp, bs, lens, out, ostride)
    flags = []
    for i, b in enumerate(blocks):
        assert res[i].status == 0, (chain, i)
        if len(b) > 15 and k == 0:                               # EXE first: it sees the block itself
            want = exemodel.forward(b, _writer_tag(b))[0]
            assert bool(res[i].skipFlags & (0x80 >> k)) == (not want), (chain, i, hex(res[i].skipFlags), want)
        if len(b) > 15:
            flags.append(bool(res[i].skipFlags & (0x80 >> k)))
    assert any(flags) and not all(flags)
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(blocks), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, chain, ent, bs, out, ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert res2[i].status == 0 and res2[i].length == len(b) and dec[i, :len(b)].tobytes() == b, (chain, i)
    ctx.reset()
    sbs = 64 << 10
    data = execases.x86_like(sbs, 7) + bytes(datagen.exe_like(sbs, 2)) + execases.arm64_like(20000, 8)
    cos = kz.CompressedOutputStream(ctx, chain, ent, sbs)
    cos.write(data)
    cos.close()
    idx = kz.knz_index(cos.output)
    assert idx["transform"] == kz.transform_type(chain) and len(idx["blocks"]) == 3
    assert kz.CompressedInputStream(ctx, cos.output).read() == data
    ctx.reset()


def test_what_stays_refused(ctx):
    ctx.reset()
    blocks = _mixed_blocks()[:3]
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    ctx.set_block_size(bs)
    with pytest.raises(kz.KanziError) as e:
        kz.encode_blocks(ctx, "EXE+RLT+TEXT+UTF+DNA", "NONE", inp, bs, lens, out, ostride)
    assert "host stages in front of the GPU stages" in str(e.value)
    for level in (4, 8, 9):                                      # ROLZ; TPAQ
        with pytest.raises(kz.KanziError):
            kz.level_chain(level)
    ctx.reset()
