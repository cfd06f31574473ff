"""Case set and Python model for the scan calls (kz_knz_scan on the host, kz_knz_scan_device on the GPU): intact streams, an
incompressible payload, a stream nested in a block, damaged streams and what must come back of each, and the coverage that
tests/test_knz_scan_cases.py computes from the model.  The model is written from the container's rules (the length prefix, the
block header and its checksum byte, the reader's bounds), with numpy over all bit positions at once; it shares no code with the
library.  Nothing here touches the GPU: streams are built by whatever compressor the caller hands in (the oracle, as in knzsplice)."""
import numpy as np

import kanzi_amd as kz
import datagen
import knzrange

END, BROKEN = -1, -2
BWT = knzrange.BWT
MIN_CHAINS = (1, 2, 3, 4)
WIDTH_LENGTHS = (4, 8, 20, 40, 80, 160, 320, 640, 1280, 2560, 5120, 10240, 20480, 40960, 65536)
SEAMS = (256, 1024, 4096, 65536)      # true prefixes lie within 16 bytes of multiples of these, and inside the last 16 bytes


# ---- the model -----------------------------------------------------------------------------------------------------------------
def header(knz):
    """(header bits, nbFunctions, blockSize, checksum bytes per block) from the stream header's fields"""
    v = int.from_bytes(knz[:20], "big")
    field = lambda at, k: (v >> (160 - at - k)) & ((1 << k) - 1)
    chk, tt, bs, mask = field(36, 2), field(43, 48), field(91, 28) << 4, field(119, 2)
    nbf = sum(1 for i in range(8) if (tt >> (42 - 6 * i)) & 0x3F)
    return 160 + 16 * mask, max(nbf, 1), bs, (0, 4, 8)[chk]


def _mix32(c, v):
    h = np.uint64(0x1E35A7BD)
    m = np.uint64(0xFFFFFFFF)
    c = c ^ ((h * (~v & m)) & m)
    c = ((c << np.uint64(13)) | (c >> np.uint64(19))) & m
    return (c * np.uint64(5) + np.uint64(0x52DCE729)) & m


class _Words:
    """the 64 bits from any bit position of `data`, left aligned, zeros behind its end"""

    def __init__(self, data):
        b = np.concatenate([np.frombuffer(data, dtype=np.uint8), np.zeros(24, dtype=np.uint8)])
        self.b = b.astype(np.uint64)
        w = np.zeros(len(b) - 8, dtype=np.uint64)
        for i in range(8):
            w = (w << np.uint64(8)) | self.b[i:len(b) - 8 + i]
        self.w = w

    def at(self, q):
        by, k = q >> 3, (q & 7).astype(np.uint64)
        return (self.w[by] << k) | (self.b[by + 8] >> (np.uint64(8) - k))        # (k = 0: the next byte shifted out whole)


def accepted(knz):
    """[(q, pay, W)] of every bit position behind the stream header at which a reader accepts a block, ascending"""
    n, nbits = len(knz), 8 * len(knz)
    hb, nbf, bs, cks = header(knz)
    words = _Words(knz)
    row = (bs + (bs >> 3) + 1024 + 64 + 255) // 256 * 256 - 64                   # the decoder's staging row holds the block
    max_tl = min(max(bs + bs // 2, 2048), 1 << 30)
    u = np.uint64
    out = []
    for q0 in range(hb, nbits, 1 << 21):
        q = np.arange(q0, min(nbits, q0 + (1 << 21)), dtype=np.int64)
        x = words.at(q)
        lr = (x >> u(59)).astype(np.int64) + 3
        w = ((x << u(5)) >> (u(64) - lr.astype(u))).astype(np.int64)
        pay = q + 5 + lr
        ok = (pay <= nbits) & (w >= 8) & (pay + w <= nbits) & ((w + 7) >> 3 <= row)
        q, pay, w = q[ok], pay[ok], w[ok]
        hd = words.at(pay)
        mode = (hd >> u(56)).astype(np.int64)
        copy, b4 = (mode & 0x80) != 0, (mode & 0x10) != 0
        has_skip = b4 & (~copy | (nbf > 4))
        derived = ((mode << 4) | 0x0F) & 0xFF
        skip = np.where(has_skip, ((hd >> u(48)) & u(0xFF)).astype(np.int64), np.where(copy & ~b4, 0, derived))
        ds = 1 + ((mode >> 5) & 3)
        at = np.where(has_skip, 16, 8)
        hsize = at // 8 + ds + 1
        pre = ((hd << at.astype(u)) >> (u(64) - (8 * ds).astype(u))).astype(np.int64)
        ck = ((hd >> (u(56) - at.astype(u) - (8 * ds).astype(u))) & u(0xFF)).astype(np.int64)
        c = np.full(len(q), (0x1E35A7BD * 0x01030507) & 0xFFFFFFFF, dtype=u)
        for v in (mode, skip, pre, w >> 32, w & 0xFFFFFFFF):
            c = _mix32(c, v.astype(u))
        c = ((c >> u(23)) ^ (c >> u(3))) & u(0xFF)
        ok = (w >= 8 * hsize) & (ck == c.astype(np.int64)) & (pre <= max_tl) & ((w + 7) >> 3 <= pre + hsize + cks)
        out += list(zip(q[ok].tolist(), pay[ok].tolist(), w[ok].tolist()))
    return out


def _bits(knz, at, k):
    return int.from_bytes(kz.extract_bits(knz, at, k), "big") >> ((-k) % 8)


def final(knz, s):
    """the end marker at s, its last bit in the stream's last byte"""
    n = len(knz)
    if s + 5 > 8 * n:
        return False
    lr = _bits(knz, s, 5) + 3
    return s + 5 + lr <= 8 * n and _bits(knz, s + 5, lr) == 0 and (s + 5 + lr + 7) >> 3 == n


def model(knz, min_chain, acc=None):
    """kz_knz_scan's results: dict(prefix, blocks, next, head), from the accepted positions (acc: accepted(knz), to share)"""
    acc = accepted(knz) if acc is None else acc
    hb = header(knz)[0]
    at = {q: i for i, (q, _, _) in enumerate(acc)}
    succ = [at.get(pay + w, -1) for _, pay, w in acc]
    fwd, back, reach = [1] * len(acc), [1] * len(acc), [False] * len(acc)
    for i in range(len(acc) - 1, -1, -1):
        if succ[i] >= 0:
            fwd[i], reach[i] = fwd[succ[i]] + 1, reach[succ[i]]
        else:
            reach[i] = final(knz, acc[i][1] + acc[i][2])
    for i in range(len(acc)):
        if succ[i] >= 0:
            back[succ[i]] = max(back[succ[i]], back[i] + 1)
    keep = [i for i in range(len(acc)) if reach[i] or back[i] + fwd[i] - 1 >= min_chain]
    rank = {i: r for r, i in enumerate(keep)}
    nxt = [rank[succ[i]] if succ[i] >= 0 else (END if final(knz, acc[i][1] + acc[i][2]) else BROKEN) for i in keep]
    head = rank[at[hb]] if at.get(hb, -1) in rank else (END if final(knz, hb) else BROKEN)
    return {"prefix": [acc[i][0] for i in keep], "blocks": [(acc[i][1], acc[i][2]) for i in keep], "next": nxt, "head": head}


def chain(scan, start):
    out = []
    while start >= 0:
        out.append(start)
        start = scan["next"][start]
    return out, start


# ---- the cases -------------------------------------------------------------------------------------------------------------------
class Case:
    """knz: the stream; kind: intact / random / nested / damage / header; blocks: the (bitOff, bits) of the undamaged stream's blocks
    that must come back, by their place in `knz`; info: what the damage tests need"""

    def __init__(self, name, knz, kind, **info):
        self.name, self.knz, self.kind, self.info = name, bytes(knz), kind, info


def _flip(knz, bit):
    bad = bytearray(knz)
    bad[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(bad)


def _assembled(encode_block, chain_, ent, bs, blocks, checksum=0):
    once = {b: encode_block(chain_, ent, bs, np.frombuffer(b, dtype=np.uint8), checksum) for b in set(blocks)}
    coded = [once[b] for b in blocks]
    return kz.knz_assemble(chain_, ent, bs, sum(len(b) for b in blocks), [s for s, _ in coded], [w for _, w in coded], checksum=checksum)


def _seam_stream(encode_block):
    """NONE&NONE blocks of chosen lengths, so that a prefix starts in the 16 bytes in front of a multiple of every seam and the next
    one in the 16 bytes behind it, and the last prefix inside the stream's last 16 bytes"""
    pool = datagen.block(3, 1024).tobytes()
    cost = {}

    def bits(length):                                              # prefix and payload bits of a block of `length` bytes
        if length not in cost:
            w = encode_block("NONE", "NONE", 1024, np.frombuffer(pool[:length], dtype=np.uint8), 0)[1]
            cost[length] = 5 + knzrange.lw(w) + w
        return cost[length]

    lens, pos = [], 192                                            # (the header of a stream with a 32-bit size field)
    for seam in (256, 1024, 4096, 8192, 65536):
        target = 8 * seam
        while True:                                                # a prefix in the 16 bytes in front of the seam, of a block of 4 bytes
            fit = [l for l in range(16, 1025) if target - bits(4) <= pos + bits(l) < target and pos + bits(l) >= target - 128]
            if fit:
                break
            step = 1024 if target - pos > bits(1024) + bits(16) else 400
            lens.append(step)
            pos += bits(step)
            assert pos < target, (seam, pos)
        lens += [fit[0], 4]                                        # ... which lies across the seam: the next prefix starts in the 16 bytes behind it
        pos += bits(fit[0]) + bits(4)
        assert target <= pos < target + 128, (seam, pos)
    lens += [300, 5]                                               # the last prefix inside the last 16 bytes
    return _assembled(encode_block, "NONE", "NONE", 1024, [pool[:l] for l in lens])


def cases(compress, encode_block):
    """compress(chain, ent, bs, data, checksum) -> .knz bytes; encode_block(chain, ent, bs, block, checksum) -> (stream, W)"""
    out = []

    def intact(name, chain_, ent, bs, n, checksum=0):
        out.append(Case(name, compress(chain_, ent, bs, datagen.stream(n // bs + 1, bs)[:n].copy(), checksum), "intact"))

    intact("empty", "NONE", "NONE", 1024, 0)
    intact("one", BWT, "ANS0", 1024, 1000)
    intact("none-1k-3", "NONE", "NONE", 1024, 3 * 1024)
    intact("bwt-1k-x32-4", BWT, "ANS0", 1024, 4 * 1024, 32)
    intact("bwt-1k-5-short-last", BWT, "ANS0", 1024, 4 * 1024 + 333)
    intact("lz-fpaq-4k-x64-copy-last", "LZ", "FPAQ", 4096, 2 * 4096 + 9, 64)                  # 9 bytes: a copy block
    intact("five-functions-4k", "TEXT+UTF+" + BWT, "ANS0", 4096, 5 * 4096 + 77, 32)          # more than 4: the skip-flag byte
    intact("bwt-64k", BWT, "ANS0", 65536, 4 * 65536 + 9)
    pool = [datagen.block(b, 64).tobytes() for b in range(64)]
    out.append(Case("many-64", _assembled(encode_block, "NONE", "NONE", 1024, [pool[(7 * i) % 64] for i in range(20000)]), "intact"))
    out.append(Case("seams", _seam_stream(encode_block), "intact"))
    wide = datagen.block(6, 65536).tobytes()                       # one block per width of the length field, 6 .. 20 bits
    out.append(Case("widths", _assembled(encode_block, "NONE", "NONE", 65536, [wide[:l] for l in WIDTH_LENGTHS]), "intact"))
    # incompressible payload: chance hits at min_chain 1, none at 4
    rnd = np.random.default_rng(20).integers(0, 256, 256 * 1024, dtype=np.uint8)
    out.append(Case("random-256k", compress("NONE", "NONE", 65536, rnd, 0), "random"))
    # a stream stored raw inside a block: a chain of its own, off head
    inner = _assembled(encode_block, "NONE", "NONE", 8192, [datagen.block(b, 300).tobytes() for b in range(6)])
    region = inner[knzrange.header_bits(inner) // 8:]
    out.append(Case("nested", compress("NONE", "NONE", 8192, np.frombuffer(region, dtype=np.uint8), 0), "nested", inner_blocks=6))
    # damage, on a 12-block stream at block 5
    base = compress(BWT, "ANS0", 1024, datagen.stream(12, 1024), 32)
    idx = kz.knz_index(base)
    f = knzrange.fields(base, idx)                                 # (prefix start, payload start, W)
    j = 5
    p5, o5, w5 = f[j]
    lr = o5 - p5 - 5
    mode = base[o5 >> 3] if o5 % 8 == 0 else _bits(base, o5, 8)
    ck_at = o5 + 8 * (1 + (1 if (mode & 0x10) and not (mode & 0x80) else 0) + 1 + ((mode >> 5) & 3))
    out.append(Case("damage-base", base, "intact"))

    def damage(name, knz, lost, shift_from=None, shift=0, **info):
        """lost: blocks of the base that must not come back; the blocks from shift_from on lie `shift` bits further on"""
        where = [(o + (shift if shift_from is not None and k >= shift_from else 0), w) for k, (o, w) in enumerate(idx["blocks"])]
        out.append(Case(name, knz, "damage", base=base, where=where, lost=set(lost), fields=f, **info))

    damage("flip-lr", _flip(base, p5 + 4), [5], broken_after=[4], gaps=[(p5, f[6][0])])
    damage("flip-w", _flip(base, p5 + 5 + lr - 1), [5], broken_after=[4], gaps=[(p5, f[6][0])])
    damage("flip-checksum-byte", _flip(base, ck_at + 7), [5], broken_after=[4], gaps=[(p5, f[6][0])])
    damage("flip-payload", _flip(base, o5 + w5 // 2), [], same_as_base=True, broken_after=[], gaps=[])
    cut = (o5 + w5 // 2) >> 3
    damage("byte-deleted", base[:cut] + base[cut + 1:], [], shift_from=6, shift=-8, broken_after=[5], gaps=[], bad_decode=[5])
    damage("cut", base[:cut], range(5, 12), broken_after=[4], gaps=[(p5, 8 * cut)])
    junk = np.random.default_rng(9).integers(0, 256, 7, dtype=np.uint8).tobytes()
    damage("cut-and-junk", base[:cut] + junk, range(5, 12), broken_after=[4], gaps=[(p5, 8 * (cut + 7))])
    p9, o9, _ = f[9]
    two = _flip(_flip(base, p5 + 5 + lr - 1), p9 + 5 + (o9 - p9 - 5) - 1)
    damage("two-breaks", two, [5, 6, 7, 8, 9], broken_after=[4], gaps=[(p5, f[10][0])], lost3=[5, 9],
           gaps3=[(p5, f[6][0]), (p9, f[10][0])], broken_after3=[4, 8])
    out.append(Case("flip-stream-header", _flip(base, 45), "header"))
    return out

