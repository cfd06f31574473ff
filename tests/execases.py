"""Inputs for the EXE tests: seeded, numpy only, nothing read from outside tests/.  The expected bytes of every one of them come from
tests/exemodel.py; tests/test_exe_model.py asserts (without a GPU) that each generator reaches what it is for."""
import functools
import struct

import numpy as np

import exemodel

E8, E9, OF, ESC = 0xE8, 0xE9, 0x0F, 0x9B


def _table():
    return np.arange(256, dtype=np.uint8)                          # every byte value: detectSimpleType says BIN only with all 256 present


@functools.lru_cache(maxsize=64)
def x86_like(n, seed):
    """a stream of short records: ~6 % E8/E9 + rel32 (|rel| < 2^20), ~3 % 0F 8x + rel32 (|rel| < 2^16), the rest runs of 00, FF FF
    pairs and 1-3 random bytes (so 9B, E8, 0F turn up on their own: escapes and false positives); the last 256 bytes are a table of
    all byte values.  Taken as X86 by the heuristic at every size from 4 096 up."""
    rng = np.random.default_rng([seed, 0x86, n])
    m = n
    kind = rng.choice(5, m, p=[0.06, 0.03, 0.32, 0.14, 0.45])      # call, jcc, zeros, FF FF, random bytes
    ln = np.select([kind == 0, kind == 1, kind == 3], [5, 6, 2], rng.integers(1, 4, m)).astype(np.int64)
    off = np.cumsum(ln) - ln
    m = int(np.searchsorted(off, n)) + 1
    kind, ln, off = kind[:m], ln[:m], off[:m]
    rec = np.repeat(np.arange(m), ln)
    j = np.arange(len(rec)) - off[rec]
    k = kind[rec]
    rel = np.where(kind == 0, rng.integers(-(1 << 20), 1 << 20, m), rng.integers(-(1 << 16), 1 << 16, m)).astype(np.int64) & 0xFFFFFFFF
    op = np.where(kind == 0, E8 + rng.integers(0, 2, m), 0x80 + rng.integers(0, 16, m))
    buf = np.where(k == 4, rng.integers(0, 256, len(rec)), np.where(k == 3, 0xFF, 0))
    sh = np.where(k == 0, j - 1, j - 2)
    relb = (rel[rec] >> (8 * np.clip(sh, 0, 3))) & 0xFF
    buf = np.where((k <= 1) & (sh >= 0), relb, buf)
    buf = np.where((k == 0) & (j == 0), op[rec], buf)
    buf = np.where((k == 1) & (j == 0), OF, buf)
    buf = np.where((k == 1) & (j == 1), op[rec], buf)
    out = buf[:n].astype(np.uint8)
    out[n - 256:] = _table()
    return out.tobytes()


@functools.lru_cache(maxsize=64)
def arm64_like(n, seed):
    """aligned 32-bit words: ~4 % B / BL with small signed offsets (one in twelve of them aimed at address 0 or below it: the escape),
    a quarter 0000xxxx, a tenth FFFFxxxx, the rest random words that are no B / BL (far targets below 0 would all be escapes and the
    block would outgrow count / 50); the last 256 bytes are a table of all byte values.  Taken as ARM64 by the heuristic."""
    rng = np.random.default_rng([seed, 0xA64, n])
    m = (n + 3) // 4
    kind = rng.choice(4, m, p=[0.04, 0.25, 0.10, 0.61])
    w = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.int64)
    w = np.where((w & 0x7C000000) == 0x14000000, w ^ 0x08000000, w)
    w = np.where(kind == 1, w & 0xFFFF, np.where(kind == 2, w | 0xFFFF0000, w))
    pos = np.arange(m, dtype=np.int64)                              # word index = byte position / 4
    offs = rng.integers(-(1 << 10), 1 << 10, m)
    esc = rng.integers(0, 12, m)
    offs = np.where(esc == 0, -pos, np.where(esc == 1, -pos - rng.integers(1, 100, m), offs))
    opc = np.where(rng.integers(0, 2, m) == 0, 0x14000000, 0x94000000)
    w = np.where(kind == 0, opc | (offs & 0x3FFFFFF), w)
    out = np.frombuffer((w & 0xFFFFFFFF).astype("<u4").tobytes(), dtype=np.uint8)[:n].copy()
    out[n - 256:] = _table()
    return out.tobytes()


# ---- headers ----------------------------------------------------------------------------------------------------------------------
def elf_block(body, bits=64, big=False, sections=(), machine=0x3E, machine_le=True, shoff=None, shentsize=None, shnum=None):
    """`body` with an ELF header over its first 64 bytes and a section header table at `shoff` (default: 64).  sections: (type,
    offset, size).  machine_le: e_machine written little-endian whatever `big` says, which is how the reference reads it (:932); a
    real big-endian file has it the other way round and falls to the heuristic."""
    e = ">" if big else "<"
    b = bytearray(body)
    h = bytearray(64)
    h[0:4] = b"\x7fELF"
    h[4], h[5], h[6] = (2 if bits == 64 else 1), (2 if big else 1), 1
    h[18:20] = struct.pack("<H" if machine_le else e + "H", machine)
    entsize = (0x40 if bits == 64 else 0x28) if shentsize is None else shentsize
    shoff = 64 if shoff is None else shoff
    nsec = len(sections) if shnum is None else shnum
    if bits == 64:
        h[0x28:0x30] = struct.pack(e + "Q", shoff)
        h[0x3A:0x3C] = struct.pack(e + "H", entsize)
        h[0x3C:0x3E] = struct.pack(e + "H", nsec)
    else:
        h[0x20:0x24] = struct.pack(e + "I", shoff)
        h[0x2E:0x30] = struct.pack(e + "H", entsize)
        h[0x30:0x32] = struct.pack(e + "H", nsec)
    b[0:64] = h
    for i, (typ, off, size) in enumerate(sections):
        at = shoff + i * entsize
        if entsize < (0x40 if bits == 64 else 0x28) or at + entsize > len(b):
            continue
        ent = bytearray(entsize)
        ent[4:8] = struct.pack(e + "I", typ)
        if bits == 64:
            ent[0x18:0x20] = struct.pack(e + "Q", off)
            ent[0x20:0x28] = struct.pack(e + "Q", size)
        else:
            ent[0x10:0x14] = struct.pack(e + "I", off)
            ent[0x14:0x18] = struct.pack(e + "I", size)
        b[at:at + entsize] = ent
    return bytes(b)


def pe_block(body, good=True, machine=0x8664, base_of_code=0x400, size_of_code=0x800, pos_pe=0x80, arch18=0):
    """MZ, e_lfanew at +60, `PE\\0\\0` at pos_pe (good) or something else (bad: arch is then the int32 at +18, :805)"""
    b = bytearray(body)
    b[0:64] = bytes(64)
    b[0:2] = b"MZ"
    b[18:22] = struct.pack("<I", arch18)
    b[60:64] = struct.pack("<I", pos_pe)
    b[pos_pe:pos_pe + 48] = bytes(48)
    b[pos_pe:pos_pe + 4] = b"PE\0\0" if good else b"NE\0\0"
    b[pos_pe + 4:pos_pe + 6] = struct.pack("<H", machine)
    b[pos_pe + 28:pos_pe + 32] = struct.pack("<I", size_of_code)
    b[pos_pe + 44:pos_pe + 48] = struct.pack("<I", base_of_code)
    return bytes(b)


def macho_block(body, bits=64, filetype=2, cpu=0x1000007, text_segment=True, text_section=True, start=0x400, size=0x800, align=0):
    """a little-endian Mach-O (magic bytes CF FA ED FE / CE FA ED FE): one LC_UUID, then one segment command with one section.  The
    reference reads the 64-bit section's offset as a long at +0x30 (offset and alignment together): align != 0 makes the range
    impossible, parseHeader returns false and codeStart stays zeroed.  For a 32-bit section it reads +0x28 as the length and +0x2C as
    the start: the values are written where it reads them."""
    b = bytearray(body)
    is64 = bits == 64
    hdr = 0x20 if is64 else 0x1C
    seg = 0x48 if is64 else 0x38
    sec = 0x50 if is64 else 0x44
    b[0:hdr + 24 + seg + sec] = bytes(hdr + 24 + seg + sec)
    b[0:4] = bytes.fromhex("cffaedfe" if is64 else "cefaedfe")
    b[4:8] = struct.pack("<I", cpu)
    b[12:16] = struct.pack("<I", filetype)
    b[16:20] = struct.pack("<I", 2)
    p = hdr
    b[p:p + 8] = struct.pack("<II", 0x1B, 24)                       # LC_UUID
    p += 24
    b[p:p + 8] = struct.pack("<II", 0x19 if is64 else 0x01, seg + sec)
    b[p + 8:p + 24] = (b"__TEXT" if text_segment else b"__DATA").ljust(16, b"\0")
    q = p + seg
    b[q:q + 16] = (b"__text" if text_section else b"__const").ljust(16, b"\0")
    b[q + 16:q + 32] = b"__TEXT".ljust(16, b"\0")
    if is64:
        b[q + 0x28:q + 0x2C] = struct.pack("<I", size)
        b[q + 0x30:q + 0x38] = struct.pack("<II", start, align)
    else:
        b[q + 0x28:q + 0x2C] = struct.pack("<I", size)
        b[q + 0x2C:q + 0x30] = struct.pack("<I", start)
    return bytes(b)


def header_cases(n=8192, seed=3):
    """(label, block, expected detect_type result or None when the heuristic decides)"""
    x = x86_like(n, seed)
    X, A = exemodel.X86, exemodel.ARM64
    S1 = [(1, 0x400, 0x800)]
    S3 = [(1, 0x400, 0x100), (8, 0x100, 0x4000), (1, 0x800, 0x600)]            # first PROGBITS sets the start, the last one the end
    out = []
    for bits in (32, 64):
        for big in (False, True):
            t = "elf%d%s" % (bits, "be" if big else "le")
            out.append((t + "-0", elf_block(x, bits, big), (X, 0, n)))
            out.append((t + "-1", elf_block(x, bits, big, S1), (X, 0x400, 0xC00)))
            out.append((t + "-3", elf_block(x, bits, big, S3), (X, 0x400, 0xE00)))
    out.append(("elf-short-section", elf_block(x, 64, False, [(1, 0x400, 63)]), (X, 0, n)))         # len < 64: ignored
    out.append(("elf-table-outside", elf_block(x, 64, False, S1, shoff=n - 0x27), None))            # posSection > count - 0x28: false, start zeroed
    out.append(("elf-table-runs-out", elf_block(x, 64, False, S1 * 3, shoff=n - 0x60), None))       # the second entry lies outside: false, range narrowed
    out.append(("elf-entsize-0", elf_block(x, 64, False, S1, shentsize=0), None))
    out.append(("elf-section-outside", elf_block(x, 64, False, [(1, 0x400, n)]), None))             # setCodeRange false
    out.append(("elf-unknown-machine", elf_block(x, 64, False, S1, machine=0x28), None))            # true, arch unknown: heuristic, narrowed range
    out.append(("elf-be-machine", elf_block(x, 64, True, S1, machine=0x3E, machine_le=False), None))
    out.append(("elf-arm64", elf_block(arm64_like(n, seed), 64, False, [(1, 0x400, 0x1800)], machine=0xB7), (A, 0x400, 0x1C00)))
    arm = arm64_like(n, seed)
    out.append(("elf-arm64-unaligned", elf_block(arm[:0x402] + arm[0x400:n - 2], 64, False, [(1, 0x402, 0x1BFD)], machine=0xB7), (A, 0x402, 0x1FFF)))
    out.append(("pe-good", pe_block(x), (X, 0x400, 0xC00)))
    out.append(("pe-arm64", pe_block(arm64_like(n, seed), machine=0xAA64, size_of_code=0x1800), (A, 0x400, 0x1C00)))
    out.append(("pe-bad-signature", pe_block(x, good=False), None))                                  # arch = int32 at +18 = 0: heuristic, whole block
    out.append(("pe-bad-signature-arch18", pe_block(x, good=False, arch18=0x14C), (X, 0, n)))       # the int32 at +18 happens to name x86
    out.append(("pe-range-outside", pe_block(x, size_of_code=n), None))
    for bits in (32, 64):
        t = "macho%d" % bits
        out.append((t, macho_block(x, bits), (X, 0x400, 0xC00)))
        out.append((t + "-dylib", macho_block(x, bits, filetype=6), None))                           # not MH_EXECUTE: false, start zeroed
        out.append((t + "-no-text-segment", macho_block(x, bits, text_segment=False), (X, 0, n)))
        out.append((t + "-no-text-section", macho_block(x, bits, text_section=False), (X, 0, n)))
    out.append(("macho64-arm64", macho_block(arm64_like(n, seed), 64, cpu=0x100000C, size=0x1800), (A, 0x400, 0x1C00)))
    out.append(("macho64-align", macho_block(x, 64, align=4), None))
    return out


# ---- the hand vector (the issue's figures) ----------------------------------------------------------------------------------------
def hand_block(n=4096, calls=16):
    b = bytearray(n)
    b[0:4] = b"\x7fELF"
    b[4], b[5], b[6], b[18], b[0x3A] = 2, 1, 1, 0x3E, 0x40
    for k in range(calls):
        p = 64 + 32 * k
        b[p] = E8
        b[p + 1:p + 5] = struct.pack("<i", 0x10 if k % 2 == 0 else -0x20)
    return b


def hand_vectors():
    """(label, block): the block and its three variants"""
    a = hand_block()
    b = hand_block(); b[64 + 32 * 15] = 0
    c = hand_block(); c[4095] = E8
    d = hand_block(); d[2000], d[2001], d[2005] = ESC, E8, 7
    return [("hand", bytes(a)), ("15-calls", bytes(b)), ("boundary", bytes(c)), ("escapes", bytes(d))]


def expansion_block(k, n=4096):
    """the hand block with k plain 9B bytes: 9 + n + k output bytes against n + n / 50"""
    b = hand_block(n)
    for i in range(k):
        b[1000 + 2 * i] = ESC
    return bytes(b)


# ---- planted events ---------------------------------------------------------------------------------------------------------------
EVENTS = {"none": b"", "call": bytes([E8]) + struct.pack("<i", 0x1234), "jcc": bytes([OF, 0x84]) + struct.pack("<i", -0x321),
          "fp": bytes([E9, 0x11, 0x22, 0x33, 0x55]), "9b": bytes([ESC]), "of9b": bytes([OF, ESC]), "of38": bytes([OF, 0x38, 0x85]),
          "nested": bytes([E8, E8, OF, 0x85, 0x00]), "nested9b": bytes([E8, ESC, E9, 0xFF, 0xFF])}


def planted(kind, p, n=8192, seed=5, code_end=None, header=True):
    """an x86_like block under an ELF header (taken whatever the plant does; with code_end: one section [64, code_end); header=False:
    no header, the heuristic takes it) whose bytes around p are zeroed, then the event written at p (cut at the block's end)"""
    b = bytearray(x86_like(n, seed))
    lo, hi = max(64 if header else 0, p - 6), min(n, p + 12)
    b[lo:hi] = bytes(hi - lo)
    ev = EVENTS[kind][:max(0, n - p)]
    b[p:p + len(ev)] = ev
    if not header:
        return bytes(b)
    return elf_block(bytes(b), 64, False, [] if code_end is None else [(1, 64, code_end - 64)], shoff=n - 0x200)


def run_block(byte, length, at, n=8192, seed=6, header=True):
    """`length` bytes `byte` (0F or E8) from `at` on: whether a byte behind the run starts an instruction depends on the run's first"""
    b = bytearray(x86_like(n, seed))
    b[at:at + length] = bytes([byte]) * length
    return elf_block(bytes(b)) if header else bytes(b)


def threshold_blocks(n=8192):
    """blocks for the heuristic alone (no header) whose x86 jump count is exactly count / 200 and one below it, with 0F skips in
    front of some of the jumps: (label, block)"""
    out = []
    for short in (0, 1):
        rng = np.random.default_rng([7, short])
        b = np.zeros(n, dtype=np.uint8)
        b[1::3] = rng.integers(16, 255, len(b[1::3]))                # two thirds zeros would fail smallVals; one third random
        b[2::3] = 0xFF
        b[b == E8] = 0x11
        b[b == E9] = 0x12
        b[b == OF] = 0x13
        b[n - 256:] = _table()                                       # (its own E8 E9 .. .. EC is no jump: EC is neither 00 nor FF)
        want = n // 200 - short
        have = exemodel.scan_counts(b.tobytes())[1]
        p = 300
        while have < want:
            if have % 3 == 0:
                b[p:p + 5] = [E8, 1, 2, 3, 0]
            elif have % 3 == 1:
                b[p:p + 6] = [OF, 0x38, 0x80, 1, 2, 3]               # 0F 38 8x: skips two, counts one
            else:
                b[p:p + 8] = [OF, OF, 0x84, E8, 0, 0, 0, 0]          # the second 0F is skipped, so is not a prefix; the E8 behind 84 counts
            have = exemodel.scan_counts(b.tobytes())[1]
            p += 24
        out.append(("jumps-%d" % have, b.tobytes()))
    return out


# ---- damaged input for the inverse -----------------------------------------------------------------------------------------------
def damaged_inputs():
    """(label, coded, dst_len)"""
    src = x86_like(4096, 11)
    ok, coded, _ = exemodel.forward(src)
    assert ok
    n = len(src)
    out = [("exact", coded, n), ("one-short", coded, n - 1), ("room", coded, n + 4096)]
    for k in range(13):
        out.append(("cut-%d" % k, coded[:k], n))
    first = coded.index(bytes([E8]), 9)
    for k in (1, 2, 3, 4):
        out.append(("cut-mid-address-%d" % k, coded[:first + k], n))
    ce = struct.unpack("<i", coded[5:9])[0]

    def hdr(cs, cend, mode=0x40):
        return bytes([mode]) + struct.pack("<ii", cs, cend) + coded[9:]
    out += [("codeStart<0", hdr(-1, ce), n), ("codeEnd<9", hdr(0, 8), n), ("codeEnd=9", hdr(0, 9), n), ("codeEnd>end", hdr(0, len(coded) + 1), n),
            ("codeEnd=end", hdr(0, len(coded)), n), ("codeStart>codeEnd-9", hdr(ce - 8, ce), n), ("codeStart=codeEnd-9", hdr(ce - 9, ce), n),
            ("codeStart>dst", hdr(100, ce), 99), ("codeStart=dst", hdr(100, ce), 100), ("mode-00", hdr(0, ce, 0), n), ("mode-60", hdr(0, ce, 0x60), n),
            ("mode-80", hdr(0, ce, 0x80), n)]
    out.append(("arm-mode-on-x86", hdr(0, ce & ~3 | 1, 0x20), n))
    for cut in range(1, 7):                                           # codeEnd moved so that an instruction straddles it
        out.append(("codeEnd-%d" % cut, hdr(0, first + cut), n + 16))
    body = bytearray(coded)
    body[ce - 1] = ESC                                               # 9B as the last code byte
    out.append(("9b-last", bytes(body), n + 8))
    body = bytearray(coded)
    body[ce - 1] = OF                                                # a trailing 0F is accepted
    out.append(("0f-last", bytes(body), n + 8))
    rng = np.random.default_rng(12)
    for i in range(12):
        body = bytearray(coded)
        at = int(rng.integers(9, len(coded)))
        body[at] ^= 1 << int(rng.integers(0, 8))
        out.append(("flip-%d" % at, bytes(body), n + int(rng.integers(-2, 3))))
    asrc = arm64_like(4096, 11)
    ok, acoded, _ = exemodel.forward(asrc)
    assert ok
    out += [("arm-exact", acoded, n), ("arm-one-short", acoded, n - 1), ("arm-room", acoded, n + 100)]
    ace = struct.unpack("<i", acoded[5:9])[0]
    p = 9
    while p < ace:                                                    # the first escape pair: cut behind its first word
        w = struct.unpack("<I", acoded[p:p + 4])[0]
        if (w & 0xFC000000) in (0x14000000, 0x94000000) and (w & 0x3FFFFFF) == 0:
            break
        p += 4
    assert p < ace
    out.append(("arm-escape-cut", acoded[:1] + struct.pack("<ii", 0, p + 4) + acoded[9:], n + 16))
    out.append(("arm-word-cut", acoded[:1] + struct.pack("<ii", 0, ace - 2) + acoded[9:], n + 16))
    for i in range(6):
        body = bytearray(acoded)
        at = int(rng.integers(9, len(acoded)))
        body[at] ^= 1 << int(rng.integers(0, 8))
        out.append(("arm-flip-%d" % at, bytes(body), n + 8))
    return out
