"""CPU model of EXE, the x86 / ARM64 branch-address transform, written from the reference's Java (K/transform/EXECodec.java), not
from the HIP kernels.  Line numbers cite that file.  Bitstream >= 3 only: inverseV2 (:497-559) is not restated.

forward(data, data_type="UNDEFINED", dst_len=None, stats=None) -> (ok, out, data_type_after)
inverse(coded, dst_len, stats=None) -> (ok, out)
max_encoded_length(n)
detect_type(data, stats=None) -> (mode, codeStart, codeEnd, arch)

`ok` is the method's return value, `out` the bytes up to `output.index` (empty where the method returns false).  `dst_len` is
`output.length` with `output.index` 0.  `input.index` and `output.index` are 0 everywhere in this library: forwardX86 starts at
`input.index + codeStart` (:166), which is codeStart here, and the model keeps the index at 0 throughout.  Where the Java would
throw (an array index outside the array) the block has failed: (False, b""); in parseHeader a read past the block makes
parseHeader return false with the range as it stood (no block of 4 096 bytes and more reaches such a read: every offset is checked
against `count` first).

`mode` is X86 (0x40), ARM64 (0x20) or NOT_EXE | Global.DataType ordinal (:676, :752, :761, :771).

`stats`, when given, is a dict whose counters are incremented (new_stats()):
  forward, x86   calls (E8/E9 coded), jcc (0F 8x coded), false_positive (escaped opcode), escaped_9b (a plain 9B doubled),
                 of_9b (0F 9B: the second byte doubled), of_plain (0F + another byte), boundary (one of the three exits)
  forward, arm   arm_bl (B / BL coded), arm_escape (target 0: 8 bytes)
  inverse        inv_calls, inv_escapes (9B dropped), inv_trailing_0f, inv_arm_bl, inv_arm_escape
  detect         header_true, header_false, header_decided (arch known), heuristic, skipped (bytes the 0F arm jumped over)
"""
X86 = 0x40                                                       # :43
ARM64 = 0x20                                                     # :44
NOT_EXE = 0x80                                                   # :42
MIN_BLOCK_SIZE = 4096                                            # :71
MAX_BLOCK_SIZE = (1 << 28) - 1                                   # :72
MASK_ADDRESS = 0xF0F0F0F0                                        # :47
X86_ADDR_MASK = (1 << 24) - 1                                    # :46
ARM_B_ADDR_MASK = (1 << 26) - 1                                  # :48
ARM_B_OPCODE_MASK = 0xFFFFFFFF ^ ARM_B_ADDR_MASK                 # :49
ARM_B_ADDR_SGN_MASK = 1 << 25                                    # :50
ARM_OPCODE_B = 0x14000000                                        # :51
ARM_OPCODE_BL = 0x94000000                                       # :52
ARM_CB_OPCODE_MASK = 0x7F000000                                  # :56
ARM_OPCODE_CBZ = 0x34000000                                      # :57
ARM_OPCODE_CBNZ = 0x3500000                                      # :58 (seven digits: it never matches under the mask)
WIN_PE = 0x00004550
WIN_X86_ARCH, WIN_AMD64_ARCH, WIN_ARM64_ARCH = 0x014C, 0x8664, 0xAA64
ELF_X86_ARCH, ELF_AMD64_ARCH, ELF_ARM64_ARCH = 0x03, 0x3E, 0xB7
MAC_AMD64_ARCH, MAC_ARM64_ARCH = 0x1000007, 0x100000C
MAC_MH_EXECUTE, MAC_LC_SEGMENT, MAC_LC_SEGMENT64 = 0x02, 0x01, 0x19
WIN_MAGIC, ELF_MAGIC = 0x4D5A, 0x7F454C46                        # K/Magic.java
MAC_MAGIC32, MAC_CIGAM32, MAC_MAGIC64, MAC_CIGAM64 = 0xFEEDFACE, 0xCEFAEDFE, 0xFEEDFACF, 0xCFFAEDFE
# Global.DataType ordinals (K/Global.java:40-80) for the NOT_EXE verdicts
DT_ORDINAL = {"UNDEFINED": 0, "TEXT": 1, "MULTIMEDIA": 2, "EXE": 3, "NUMERIC": 4, "BASE64": 5, "DNA": 6, "BIN": 7, "UTF8": 8, "SMALL_ALPHABET": 9}
M32 = 0xFFFFFFFF

STAT_KEYS = ("calls", "jcc", "false_positive", "escaped_9b", "of_9b", "of_plain", "boundary", "arm_bl", "arm_escape",
             "inv_calls", "inv_escapes", "inv_trailing_0f", "inv_arm_bl", "inv_arm_escape",
             "header_true", "header_false", "header_decided", "heuristic", "skipped")


def new_stats():
    return dict.fromkeys(STAT_KEYS, 0)


def _bump(stats, key, by=1):
    if stats is not None:
        stats[key] += by


def _i32(v):
    v &= M32
    return v - (1 << 32) if v & 0x80000000 else v


def _i64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def max_encoded_length(n):                                       # :653-656
    return n + 32 if n <= 256 else n + n // 8


class _PastBlock(Exception):
    pass


class _Reader:
    """reads inside the block; one past it is the Java's ArrayIndexOutOfBoundsException"""
    def __init__(self, src):
        self.s = src

    def get(self, off, k):
        if off < 0 or off + k > len(self.s):
            raise _PastBlock()
        return self.s[off:off + k]

    def le16(self, off):
        return int.from_bytes(self.get(off, 2), "little")

    def le32(self, off):
        return _i32(int.from_bytes(self.get(off, 4), "little"))

    def le64(self, off):
        return _i64(int.from_bytes(self.get(off, 8), "little"))

    def be16(self, off):
        return int.from_bytes(self.get(off, 2), "big")

    def be32(self, off):
        return _i32(int.from_bytes(self.get(off, 4), "big"))

    def be64(self, off):
        return _i64(int.from_bytes(self.get(off, 8), "big"))


def magic_type(src):                                             # K/Magic.java:147-185, only what parseHeader looks at
    if len(src) < 4:
        return 0
    key = int.from_bytes(src[0:4], "big")
    if key in (ELF_MAGIC, MAC_MAGIC32, MAC_CIGAM32, MAC_MAGIC64, MAC_CIGAM64):
        return key
    if (key >> 16) == WIN_MAGIC:
        return WIN_MAGIC
    return 0


class _Range:
    def __init__(self, count):
        self.start, self.end, self.arch = 0, count, 0             # :139-140, :670

    def set_code_range(self, count, range_start, range_length, update_start):   # :784-800 with start = 0
        if range_start < 0 or range_length < 0 or range_start > count or range_length > count - range_start:
            return False
        if update_start or self.start == 0:
            self.start = range_start
        self.end = range_start + range_length
        return True


def _parse_header(src, count, magic, R):                         # :802-1011
    rd = _Reader(src)
    try:
        if magic == WIN_MAGIC:
            if count >= 64:
                R.arch = rd.le32(18)                             # :805: an int32, replaced only under a good signature
                pos_pe = rd.le32(60)
                if 0 < pos_pe <= count - 48 and rd.le32(pos_pe) == WIN_PE:
                    if not R.set_code_range(count, rd.le32(pos_pe + 44), rd.le32(pos_pe + 28), True):
                        return False
                    R.arch = rd.le16(pos_pe + 4)
                return True
        elif magic == ELF_MAGIC:
            little = src[5] == 1                                 # :821
            if count >= 64:
                R.start = 0                                      # :824
                r16, r32, r64 = (rd.le16, rd.le32, rd.le64) if little else (rd.be16, rd.be32, rd.be64)
                if src[4] == 2:                                  # 64 bits: :829-851, :881-903
                    nb, sz, pos, room = r16(0x3C), r16(0x3A), r64(0x28), 0x28
                else:                                            # 32 bits: :854-876, :906-928
                    nb, sz, pos, room = r16(0x30), r16(0x2E), r32(0x20), 0x18
                if sz <= 0 or pos < 0 or pos > count - room:
                    return False
                for i in range(nb):
                    entry = pos + i * sz
                    if entry < 0 or entry > count - room:
                        return False
                    typ = r32(entry + 4)
                    if src[4] == 2:
                        off, ln = r64(entry + 0x18), r64(entry + 0x20)
                    else:
                        off, ln = r32(entry + 0x10), r32(entry + 0x14)
                    if typ == 1 and ln >= 64:
                        if not R.set_code_range(count, off, ln, False):
                            return False
                R.arch = rd.le16(18)                             # :932: little-endian whatever the file says
                R.start = min(R.start, count)
                R.end = min(R.end, count)
                return True
        elif magic in (MAC_MAGIC32, MAC_CIGAM32, MAC_MAGIC64, MAC_CIGAM64):
            is64 = magic in (MAC_MAGIC64, MAC_CIGAM64)
            R.start = 0                                          # :940
            if count >= 64:
                if rd.le32(12) != MAC_MH_EXECUTE:
                    return False
                R.arch = rd.le32(4)
                nb_cmds = rd.le32(0x10)
                pos = 0x20 if is64 else 0x1C
                cmd = 0
                while cmd < nb_cmds:
                    if pos > count - 8:
                        return False
                    ld_cmd, sz_cmd = rd.le32(pos), rd.le32(pos + 4)
                    sz_seg = 0x48 if is64 else 0x38
                    if sz_cmd < 8 or sz_cmd > count - pos:
                        return False
                    if ld_cmd in (MAC_LC_SEGMENT, MAC_LC_SEGMENT64):
                        if pos > count - 14 or pos > count - sz_seg:
                            return False
                        if (rd.be64(pos + 8) & ((1 << 64) - 1)) >> 16 == 0x5F5F54455854:      # "__TEXT"
                            pos_sec = pos + sz_seg
                            if pos_sec > count - (0x38 if is64 else 0x30):
                                return False
                            if (rd.be64(pos_sec) & ((1 << 64) - 1)) >> 16 == 0x5F5F74657874:  # "__text"
                                if is64:
                                    ok = R.set_code_range(count, rd.le64(pos_sec + 0x30), rd.le32(pos_sec + 0x28), True)
                                else:
                                    ok = R.set_code_range(count, rd.le32(pos_sec + 0x2C), rd.le32(pos_sec + 0x28), True)
                                if not ok:
                                    return False
                                break
                    cmd += 1
                    pos = _i32(pos + sz_cmd)
                R.start = min(R.start, count)
                R.end = min(R.end, count)
                return True
    except _PastBlock:
        return False
    return False


def detect_simple_type(count, histo):                            # K/Global.java:556-605
    if count == 0:
        return "UNDEFINED"
    if sum(histo[c] for c in b"acgntuACGNTU") > count - count // 12:
        return "DNA"
    digits = sum(histo[0x30:0x3A])
    if digits + sum(histo[c] for c in b"+-*/=,.:; ") == count:
        return "NUMERIC"
    b64 = digits + sum(histo[0x41:0x5B]) + sum(histo[0x61:0x7B]) + histo[0x2B] + histo[0x2F]
    if b64 + (1 if histo[0x3D] == 1 else 0) == count:
        return "BASE64"
    nsym = sum(1 for f in histo if f > 0)
    if nsym == 256:
        return "BIN"
    if nsym <= 4:
        return "SMALL_ALPHABET"
    return "UNDEFINED"


def scan_counts(src, stats=None):
    """the heuristic's loop (:701-747): the histogram of the VISITED bytes and the two jump counts"""
    end = len(src)
    histo = [0] * 256
    jx = ja = 0
    i = 0
    while i < end:
        b = src[i]
        histo[b] += 1
        if i + 4 < end and (b & 0xFE) == 0xE8:                   # :710: tested first
            if src[i + 4] in (0, 0xFF):
                jx += 1
        elif b == 0x0F and i + 1 < end:                          # :720
            j = i + 1
            if src[j] in (0x38, 0x3A) and j + 1 < end:
                j += 1
            if (src[j] & 0xF0) == 0x80:                          # :728: the offset is not looked at
                jx += 1
            _bump(stats, "skipped", j - i)
            i = j                                                # :730, :732: the bytes up to j are neither counted nor tested
        if (i & 3) == 0 and i + 4 <= end:                        # :737: with the moved i
            instr = int.from_bytes(src[i:i + 4], "little")
            op1, op2 = instr & ARM_B_OPCODE_MASK, instr & ARM_CB_OPCODE_MASK
            if op1 in (ARM_OPCODE_B, ARM_OPCODE_BL) or op2 in (ARM_OPCODE_CBZ, ARM_OPCODE_CBNZ):
                ja += 1
        i += 1
    return histo, jx, ja


def detect_type(data, stats=None):                               # :666-772
    src = bytes(data)
    count = len(src)
    R = _Range(count)
    if _parse_header(src, count, magic_type(src), R):
        _bump(stats, "header_true")
        if R.start < 0 or R.start > count or R.end < R.start or R.end > count:
            return NOT_EXE | DT_ORDINAL["UNDEFINED"], R.start, R.end, R.arch
        if R.arch in (ELF_X86_ARCH, ELF_AMD64_ARCH, WIN_X86_ARCH, WIN_AMD64_ARCH, MAC_AMD64_ARCH):
            _bump(stats, "header_decided")
            return X86, R.start, R.end, R.arch
        if R.arch in (ELF_ARM64_ARCH, WIN_ARM64_ARCH, MAC_ARM64_ARCH):
            _bump(stats, "header_decided")
            return ARM64, R.start, R.end, R.arch
    else:
        _bump(stats, "header_false")
    if R.start < 0 or R.start > count or R.end < R.start or R.end > count:
        return NOT_EXE | DT_ORDINAL["UNDEFINED"], R.start, R.end, R.arch
    if count <= 0:
        return NOT_EXE | DT_ORDINAL["UNDEFINED"], R.start, R.end, R.arch
    _bump(stats, "heuristic")
    histo, jx, ja = scan_counts(src, stats)
    dt = detect_simple_type(count, histo)
    if dt != "BIN":
        return NOT_EXE | DT_ORDINAL[dt], R.start, R.end, R.arch
    if histo[0] < count // 10 or sum(histo[:16]) > count // 2 or histo[255] < count // 100:      # :760
        return NOT_EXE | DT_ORDINAL[dt], R.start, R.end, R.arch
    if jx >= count // 200:                                       # :764: x86 first
        return X86, R.start, R.end, R.arch
    if ja >= count // 200:
        return ARM64, R.start, R.end, R.arch
    return NOT_EXE | DT_ORDINAL[dt], R.start, R.end, R.arch


def _forward_x86(src, code_start, code_end, dst_len, stats):     # :162-265
    count = len(src)
    dst = bytearray(dst_len)
    dst[0] = X86
    s, d = code_start, 9
    dst_end = dst_len - 5
    boundary = False
    matches = 0
    if code_start > dst_len or d + code_start > dst_len:         # :172-173
        return False, b""
    if code_end < code_start or code_end > dst_len:              # :175-176
        return False, b""
    dst[d:d + code_start] = src[:code_start]                     # :178-181
    d += code_start
    while s < code_end and d < dst_end:
        if src[s] == 0x0F:
            if s + 1 >= code_end:                                # :185
                boundary = True
                break
            if (src[s + 1] & 0xF0) == 0x80 and s + 5 >= code_end:    # :190-195: before the 0F is copied
                boundary = True
                break
            dst[d] = src[s]
            d += 1
            s += 1
            if (src[s] & 0xF0) != 0x80:                          # :199-206
                if src[s] == 0x9B:
                    dst[d] = 0x9B
                    d += 1
                    _bump(stats, "of_9b")
                else:
                    _bump(stats, "of_plain")
                dst[d] = src[s]
                d += 1
                s += 1
                continue
            if s + 4 >= code_end:                                # :208 (never true after :191)
                boundary = True
                break
            kind = "jcc"
        elif (src[s] & 0xFE) != 0xE8:                            # :212-218
            if src[s] == 0x9B:
                dst[d] = 0x9B
                d += 1
                _bump(stats, "escaped_9b")
            dst[d] = src[s]
            d += 1
            s += 1
            continue
        elif s + 4 >= code_end:                                  # :219
            boundary = True
            break
        else:
            kind = "calls"
        sgn = src[s + 4]
        offset = _i32(int.from_bytes(src[s + 1:s + 5], "little"))
        if sgn not in (0, 0xFF) or (offset & M32) == 0xFF000000:     # :229-233: only the opcode byte is consumed
            dst[d] = 0x9B
            dst[d + 1] = src[s]
            d += 2
            s += 1
            _bump(stats, "false_positive")
            continue
        addr = _i32(s + (offset if sgn == 0 else -((-offset) & X86_ADDR_MASK)))      # :236
        dst[d] = src[s]
        dst[d + 1:d + 5] = ((addr ^ MASK_ADDRESS) & M32).to_bytes(4, "big")
        s += 5
        d += 5
        matches += 1
        _bump(stats, kind)
    if boundary:
        _bump(stats, "boundary")
    if matches < 16 or (s < code_end and not boundary):          # :246
        return False, b""
    if d + (count - s) > dst_end:                                # :249
        return False, b""
    dst[1:5] = code_start.to_bytes(4, "little")
    dst[5:9] = d.to_bytes(4, "little")                           # counts the 9 header bytes
    dst[d:d + count - s] = src[s:]
    d += count - s
    if d > count + count // 50:                                  # :259
        return False, b""
    return True, bytes(dst[:d])


def _forward_arm(src, code_start, code_end, dst_len, stats):     # :267-364
    count = len(src)
    dst = bytearray(dst_len + 8)                                 # (the Java array is as long as dst_len; the slack is never kept)
    dst[0] = ARM64
    s, d = code_start, 9
    dst_end = dst_len - 8
    matches = 0
    if d + code_start > dst_len:                                 # System.arraycopy would throw
        return False, b""
    dst[d:d + code_start] = src[:code_start]
    d += code_start
    while s + 4 <= code_end and d < dst_end:                     # :281: 4-byte steps from codeStart
        instr = int.from_bytes(src[s:s + 4], "little")
        op1 = instr & ARM_B_OPCODE_MASK
        if op1 not in (ARM_OPCODE_B, ARM_OPCODE_BL):             # isCB is hard-wired false (:286)
            dst[d:d + 4] = src[s:s + 4]
            s += 4
            d += 4
            continue
        offset = instr & ARM_B_ADDR_MASK
        sgn = instr & ARM_B_ADDR_SGN_MASK
        addr = _i32(s + 4 * _i32(offset if sgn == 0 else (ARM_B_OPCODE_MASK | offset)))   # :307
        if addr < 0:
            addr = 0
        val = (op1 | (addr >> 2)) & M32
        dst[d:d + 4] = val.to_bytes(4, "little")
        if addr == 0:                                            # :326-335: the escape, not a match
            dst[d + 4:d + 8] = src[s:s + 4]
            s += 4
            d += 8
            _bump(stats, "arm_escape")
            continue
        s += 4
        d += 4
        matches += 1
        _bump(stats, "arm_bl")
    if matches < 16 or (s + 4 <= code_end and d >= dst_end):     # :345
        return False, b""
    if d + (count - s) > dst_end:
        return False, b""
    dst[1:5] = code_start.to_bytes(4, "little")
    dst[5:9] = d.to_bytes(4, "little")
    dst[d:d + count - s] = src[s:]
    d += count - s
    if d > count + count // 50:
        return False, b""
    return True, bytes(dst[:d])


def forward(data, data_type="UNDEFINED", dst_len=None, stats=None):      # :110-160
    src = bytes(data)
    count = len(src)
    if count == 0:
        return True, b"", data_type
    if count < MIN_BLOCK_SIZE or count > MAX_BLOCK_SIZE:         # :119
        return False, b"", data_type
    if dst_len is None:
        dst_len = max_encoded_length(count)
    if dst_len < max_encoded_length(count):                      # :127
        return False, b"", data_type
    if data_type not in ("UNDEFINED", "EXE", "BIN"):             # :130-137
        return False, b"", data_type
    mode, code_start, code_end, _ = detect_type(src, stats)
    if mode & NOT_EXE:                                           # :143: the detected type is not written to the context
        return False, b"", data_type
    if mode == X86:
        ok, out = _forward_x86(src, code_start, code_end, dst_len, stats)
    else:
        ok, out = _forward_arm(src, code_start, code_end, dst_len, stats)
    return ok, out, ("EXE" if ok else data_type)                 # :156-157


def _inverse_header(src, dst_len):                               # :410-415, :567-572
    end = len(src)
    code_start = _i32(int.from_bytes(src[1:5], "little"))
    code_end = _i32(int.from_bytes(src[5:9], "little"))
    if code_start < 0 or code_end < 9 or code_end > end or code_start > code_end - 9 or code_start > dst_len:
        return None
    return code_start, code_end


def _inverse_x86(src, dst_len, stats):                           # :404-495
    end = len(src)
    hdr = _inverse_header(src, dst_len)
    if hdr is None:
        return False, b""
    code_start, code_end = hdr
    dst = bytearray(dst_len)
    dst[:code_start] = src[9:9 + code_start]
    s, d = 9 + code_start, code_start
    while s < code_end:
        if src[s] == 0x0F:
            if s + 1 >= code_end:                                # :425-433: a trailing 0F (legacy streams)
                if d >= dst_len:
                    return False, b""
                dst[d] = src[s]
                d += 1
                s += 1
                _bump(stats, "inv_trailing_0f")
                break
            if d >= dst_len:
                return False, b""
            dst[d] = src[s]
            d += 1
            s += 1
            if (src[s] & 0xF0) != 0x80:
                if src[s] == 0x9B:                               # :442-447
                    s += 1
                    _bump(stats, "inv_escapes")
                    if s >= code_end:
                        return False, b""
                if d >= dst_len:
                    return False, b""
                dst[d] = src[s]
                d += 1
                s += 1
                continue
        elif (src[s] & 0xFE) != 0xE8:
            if src[s] == 0x9B:                                   # :457-462: the next byte is copied raw, whatever it is
                s += 1
                _bump(stats, "inv_escapes")
                if s >= code_end:
                    return False, b""
            if d >= dst_len:
                return False, b""
            dst[d] = src[s]
            d += 1
            s += 1
            continue
        if s + 4 >= code_end:                                    # :471
            return False, b""
        if d + 5 > dst_len:                                      # :474
            return False, b""
        addr = _i32(int.from_bytes(src[s + 1:s + 5], "big") ^ MASK_ADDRESS)
        offset = addr - d                                        # a long (:479)
        enc = _i32(offset) if offset >= 0 else -((-offset) & X86_ADDR_MASK)       # :480
        dst[d] = src[s]
        dst[d + 1:d + 5] = (enc & M32).to_bytes(4, "little")
        s += 5
        d += 5
        _bump(stats, "inv_calls")
    if d + (end - s) > dst_len:                                  # :487
        return False, b""
    dst[d:d + end - s] = src[s:]
    d += end - s
    return True, bytes(dst[:d])


def _inverse_arm(src, dst_len, stats):                           # :561-644
    end = len(src)
    hdr = _inverse_header(src, dst_len)
    if hdr is None:
        return False, b""
    code_start, code_end = hdr
    dst = bytearray(dst_len)
    dst[:code_start] = src[9:9 + code_start]
    s, d = 9 + code_start, code_start
    while s < code_end:
        if s + 4 > code_end:                                     # :581
            return False, b""
        if d + 4 > dst_len:                                      # :584
            return False, b""
        instr = int.from_bytes(src[s:s + 4], "little")
        op1 = instr & ARM_B_OPCODE_MASK
        if op1 not in (ARM_OPCODE_B, ARM_OPCODE_BL):
            dst[d:d + 4] = src[s:s + 4]
            s += 4
            d += 4
            continue
        addr = _i32((instr & ARM_B_ADDR_MASK) << 2)              # :609
        offset = _i32(addr - d) >> 2                             # :610: an arithmetic shift
        val = (op1 | (offset & ARM_B_ADDR_MASK)) & M32
        if addr == 0:                                            # :618-629
            if s + 8 > code_end:
                return False, b""
            dst[d:d + 4] = src[s + 4:s + 8]
            s += 8
            d += 4
            _bump(stats, "inv_arm_escape")
            continue
        dst[d:d + 4] = val.to_bytes(4, "little")
        s += 4
        d += 4
        _bump(stats, "inv_arm_bl")
    if d + (end - s) > dst_len:
        return False, b""
    dst[d:d + end - s] = src[s:]
    d += end - s
    return True, bytes(dst[:d])


def inverse(coded, dst_len, stats=None):                         # :374-402
    src = bytes(coded)
    if len(src) == 0:
        return True, b""
    if len(src) < 9:                                             # :390
        return False, b""
    if src[0] == X86:
        return _inverse_x86(src, dst_len, stats)
    if src[0] == ARM64:
        return _inverse_arm(src, dst_len, stats)
    return False, b""
