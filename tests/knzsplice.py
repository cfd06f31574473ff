"""Case set and helpers for the splice calls (kz_knz_splice on the host, kz_knz_splice_device on the GPU): the sources, the plans made
from their indices, what each result must equal or decode to, the refusals, the Python model of a result, and the coverage that
tests/test_knz_splice_cases.py computes from the plans.  Nothing here touches the GPU: a stream is built by whatever compressor
the caller hands in, as in knzrange.Stream.build (the oracle in tests/test_knz_splice_cases.py, the library in
tests/test_gpu_knz_splice.py; the two write the same bytes)."""
import numpy as np

import kanzi_amd as kz
import datagen
import knzrange

CHUNK = 3                     # KZ_STREAM_CHUNK of the seam cases: the pieces go through in steps of three
BWT = knzrange.BWT
SETTINGS = [("NONE", "NONE", 1024, 0), (BWT, "ANS0", 1024, 32), ("LZ", "HUFFMAN", 4096, 64)]
POISON = 0xA5


class Case:
    """pieces [(source, bitOff, bits)] of `sources` (.knz bytes) and the header's size -> a stream that is `equals` byte for byte
    and / or decodes to `decoded` (None: not stated; synthetic sources hold random bits and decode to nothing)"""

    def __init__(self, name, sources, pieces, input_size, equals=None, decoded=None, lens=None):
        self.name, self.sources, self.pieces, self.input_size = name, [bytes(s) for s in sources], list(pieces), int(input_size)
        self.equals, self.decoded = equals, decoded
        self.lens = list(lens) if lens else [len(s) for s in self.sources]       # srcLen (a source may be cut short of its bytes)

    def bits(self):
        return [w for _, _, w in self.pieces]


def head(knz):
    """the header parameters of a stream, as knz_index gives them, of a stream that is cut short as well"""
    return kz.knz_index(knz[:knzrange.header_bits(knz) // 8] + b"\0")


def model(case):
    """the definition of a result: kz_knz_assemble(the sources' header parameters, the pieces' extracted bit strings, their W)"""
    idx = head(case.sources[0])
    rows = [kz.extract_bits(case.sources[s][:case.lens[s]], off, w) for s, off, w in case.pieces]
    return kz.knz_assemble(idx["transform"], idx["entropy"], idx["blockSize"], case.input_size, rows, case.bits(), checksum=idx["checksum"])


def prefix_starts(case):
    """[bit where piece i's prefix starts in the result] + [the end marker's]"""
    pos, out = knzrange.header_bits(model_header(case)), []
    for w in case.bits():
        out.append(pos)
        pos += 5 + knzrange.lw(w) + w
    return out + [pos]


def model_header(case):
    idx = head(case.sources[0])
    return kz.knz_assemble(idx["transform"], idx["entropy"], idx["blockSize"], case.input_size, [], [], checksum=idx["checksum"])


def _data(bs, nblocks, tail, first=0):
    return datagen.stream(nblocks + 1, bs, first)[:nblocks * bs + tail].copy()


def _blocks(data, bs):
    return [data[i:i + bs].tobytes() for i in range(0, len(data), bs)]


def _phase_plan(knz, idx, limit=400):
    """pieces of one source chosen greedily until all 64 pairs (payload phase in the source, payload phase in the result) occur"""
    blocks = idx["blocks"]
    pos, seen, pieces = knzrange.header_bits(knz), set(), []
    while len(seen) < 64 and len(pieces) < limit:
        best = None
        for k, (off, w) in enumerate(blocks):
            pair = (off % 8, (pos + 5 + knzrange.lw(w)) % 8)
            if pair not in seen:
                best = k
                break
        if best is None:
            best = (len(pieces) * 7 + 1) % len(blocks)        # nothing new from here: move on to another phase
        off, w = blocks[best]
        seen.add((off % 8, (pos + 5 + knzrange.lw(w)) % 8))
        pieces.append((0, off, w))
        pos += 5 + knzrange.lw(w) + w
    return pieces


def _packed_plan(knz, idx):
    """block numbers: a few blocks that bring the next payload to the first bits of a 16-byte unit of the result (counted from the
    stream's first byte, size field empty), then three of the shortest blocks, whose payloads and the two prefixes between them lie
    whole inside that unit.  (The shortest block stream, of one data byte, has 32 bits, 43 with its prefix: three whole prefixes
    and payloads, 129 bits, fit in no unit; the synthetic case "micro" has those.)"""
    blocks = idx["blocks"]
    cost = {k: 5 + knzrange.lw(w) + w for k, (_, w) in enumerate(blocks)}
    small = min(cost, key=cost.get)
    w, pw = blocks[small][1], cost[small] - blocks[small][1]
    assert 3 * w + 2 * pw <= 128
    reach = {160 % 128: []}                                   # residue of the next prefix start -> the blocks that lead there
    for _ in range(8):
        for r, path in list(reach.items()):
            for k, c in cost.items():
                reach.setdefault((r + c) % 128, path + [k])
    r = min(x for x in reach if (x + pw) % 128 + 3 * w + 2 * pw <= 128)
    return reach[r] + [small] * 3 + [len(blocks) - 1]


def _micro_source(nb=40, seed=21):
    """a synthetic stream of blocks of 8 to 24 random bits: whole pieces, prefix and payload, three and more to a 16-byte unit"""
    rng = np.random.default_rng(seed)
    ws = [int(w) for w in rng.integers(8, 25, nb)]
    rows = [rng.integers(0, 256, (w + 7) // 8, dtype=np.uint8).tobytes() for w in ws]
    return kz.knz_assemble("NONE", "NONE", 1024, 0, rows, ws)


def _last_bits_source(seed=11):
    """a synthetic stream cut behind a block that ends on a byte boundary: (the cut stream, its blocks)"""
    for s in range(seed, seed + 64):
        knz = knzrange.synthetic(nb=6, seed=s)
        blocks = kz.knz_index(knz)["blocks"]
        for k in range(2, len(blocks)):
            off, w = blocks[k]
            if (off + w) % 8 == 0:
                return knz[:(off + w) // 8], blocks[:k + 1]
    raise AssertionError("no block of the synthetic streams ends on a byte boundary")


def cases(compress, encode_block):
    """compress(chain, ent, bs, data, checksum) -> .knz bytes; encode_block(chain, ent, bs, block, checksum) -> (stream, W)"""
    out = []
    for chain, ent, bs, chk in SETTINGS:
        tag = "%s-%d" % (chain.split("+")[0].lower(), bs)
        D = _data(bs, 6, 333)
        S = compress(chain, ent, bs, D, chk)
        idx = kz.knz_index(S)
        blk = _blocks(D, bs)
        all_pieces = [(0, off, w) for off, w in idx["blocks"]]
        # all blocks of S in order with S's size give S
        out.append(Case(tag + "-identity", [S], all_pieces, idx["inputSize"], equals=S, decoded=D.tobytes()))
        # a block range as a stream of its own: in the middle, and up to the short last block
        for first, count in ((2, 3), (4, 9)):
            p, n = kz.splice_slice(idx, first, count)
            part = D[first * bs:(first + count) * bs]
            out.append(Case("%s-slice-%d+%d" % (tag, first, count), [S], p, n, equals=compress(chain, ent, bs, part, chk), decoded=part.tobytes()))
        # a block replaced after only the new bytes were compressed
        N = datagen.block(40, bs)
        SN = compress(chain, ent, bs, N, chk)
        p, n = kz.splice_replace(idx, 1, 1, kz.knz_index(SN))
        E = np.concatenate([D[:bs], N, D[2 * bs:]])
        out.append(Case(tag + "-replace-1", [S, SN], p, n, equals=compress(chain, ent, bs, E, chk), decoded=E.tobytes()))
        if chk == 32:
            # a block appended to a stream of whole blocks
            W6 = compress(chain, ent, bs, D[:6 * bs], chk)
            T = datagen.block(41, 500)
            ST = compress(chain, ent, bs, T, chk)
            p, n = kz.splice_replace(kz.knz_index(W6), 6, 1, kz.knz_index(ST))
            E = np.concatenate([D[:6 * bs], T])
            out.append(Case(tag + "-append", [W6, ST], p, n, equals=compress(chain, ent, bs, E, chk), decoded=E.tobytes()))
            # streams joined: whole blocks in all but the last give the stream of the joined data; ragged ones decode to it
            for kind, la, lb, lc in (("whole", 2 * bs, 3 * bs, bs + 77), ("ragged", 2 * bs + 5, 700, bs)):
                A, B, C = [_data(bs, n // bs, n % bs, f) for n, f in ((la, 50), (lb, 60), (lc, 70))]
                srcs = [compress(chain, ent, bs, x, chk) for x in (A, B, C)]
                p, n = kz.splice_concat([kz.knz_index(s) for s in srcs])
                J = np.concatenate([A, B, C])
                assert n == len(J)
                out.append(Case("%s-concat-%s" % (tag, kind), srcs, p, n, equals=compress(chain, ent, bs, J, chk) if kind == "whole" else None,
                                decoded=J.tobytes()))
                if kind == "whole":
                    whole = (A, B, C, srcs)
            A, B, C, srcs = whole
            # three sources interleaved (a short block comes to lie in the middle)
            ia, ib, ic = [kz.knz_index(s)["blocks"] for s in srcs]
            order = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (1, 2)]
            ba, bb, bc = _blocks(A, bs), _blocks(B, bs), _blocks(C, bs)
            p = [(s, *(ia, ib, ic)[s][k]) for s, k in order]
            out.append(Case(tag + "-interleave-3", srcs, p, 0, decoded=b"".join((ba, bb, bc)[s][k] for s, k in order)))
        # reverse order, repeats, no pieces
        out.append(Case(tag + "-reverse", [S], all_pieces[::-1], 0, decoded=b"".join(blk[::-1])))
        rep = [0, 0, 3, 3, 3, 6, 5]
        out.append(Case(tag + "-repeats", [S], [all_pieces[k] for k in rep], 0, decoded=b"".join(blk[k] for k in rep)))
        out.append(Case(tag + "-empty", [S], [], 0, decoded=b""))
    # the wide path: payloads of 2^19 bits, units wholly inside one payload, source and result at different phases
    D = _data(65536, 2, 9, 80)
    S = compress("NONE", "NONE", 65536, D, 0)
    idx = kz.knz_index(S)
    p = [(0, off, w) for off, w in idx["blocks"]]
    out.append(Case("wide-identity", [S], p, idx["inputSize"], equals=S, decoded=D.tobytes()))
    out.append(Case("wide-reverse", [S], p[::-1], 0, decoded=b"".join(_blocks(D, 65536)[::-1])))
    # blocks of 1 to 5 data bytes: several whole pieces inside one 16-byte unit of the result
    lens = [1, 2, 1, 3, 1, 1, 2, 5, 4, 1, 2, 1, 1, 3, 5, 1]
    tiny = knzrange.Stream("tiny", "NONE", "NONE", 1024, lens=lens)
    S = tiny.build(compress, encode_block)
    idx = kz.knz_index(S)
    p = [(0, off, w) for off, w in idx["blocks"]]
    tb = [b.tobytes() for b in tiny.block_data()]
    out.append(Case("tiny-identity", [S], p, idx["inputSize"], equals=S, decoded=b"".join(tb)))
    out.append(Case("tiny-reverse", [S], p[::-1], 0, decoded=b"".join(tb[::-1])))
    packed = _packed_plan(S, idx)
    out.append(Case("tiny-packed", [S], [p[k] for k in packed], 0, decoded=b"".join(tb[k] for k in packed)))
    # synthetic blocks (random bits: the container does not look inside): every pair of bit phases; the last bits of a cut source
    S = knzrange.synthetic(nb=64, seed=9)
    out.append(Case("phases", [S], _phase_plan(S, kz.knz_index(S)), 0))
    S = _micro_source()
    out.append(Case("micro", [S], [(0, off, w) for off, w in kz.knz_index(S)["blocks"][::-1]], 0))
    cut, blocks = _last_bits_source()
    out.append(Case("last-bits", [cut], [(0, off, w) for off, w in blocks[::-1]], 0))
    return out


# ---- coverage, computed from the plans ----
def coverage(cs):
    pairs, three, inside, last_bits, big, seam_in, seam_on, three_pay = set(), False, False, False, False, False, False, False
    for c in cs:
        pre = prefix_starts(c)
        pays = []
        for (s, off, w), p in zip(c.pieces, pre):
            pay = p + 5 + knzrange.lw(w)
            pays.append((p, pay, w))
            pairs.add((off % 8, pay % 8))
            last_bits |= off + w == 8 * c.lens[s]
            big |= w >= 1 << 16
            inside |= (pay + 127) // 128 * 128 + 128 <= pay + w                 # an aligned 16-byte unit inside the payload
        ends = [pay + w for _, pay, w in pays]
        for u in range(0, pre[-1], 128):                                        # units counted from the stream's first byte
            three |= sum(1 for (p, _, _), e in zip(pays, ends) if u <= p and e <= u + 128) >= 3
            if c.decoded is not None:                                           # real block streams
                three_pay |= sum(1 for (_, pay, _), e in zip(pays, ends) if u <= pay and e <= u + 128) >= 3
        for k in range(CHUNK, len(c.pieces), CHUNK):
            seam_in |= pre[k] % 8 != 0
            seam_on |= pre[k] % 8 == 0
    return {"phase pairs": len(pairs), "three pieces in a unit": three, "three payloads of real blocks in a unit": three_pay, "unit inside a payload": inside, "last bits of a source": last_bits,
            "W >= 2^16": big, "seam inside a byte": seam_in, "seam on a byte": seam_on}


# ---- the raw calls ----
def pack(sources, lead=0, gap=0, fill=POISON, tail=0):
    """the sources one behind the other (gap bytes of fill between them) behind `lead` bytes -> (buffer, offsets)"""
    offs, pos = [], lead
    for s in sources:
        offs.append(pos)
        pos += len(s) + gap
    buf = np.full(max(pos - gap + tail, 1), fill, dtype=np.uint8)
    for o, s in zip(offs, sources):
        buf[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return buf, offs


ARGS = ("src", "srcOff", "srcLen", "nSrc", "pieceSrc", "pieceBitOff", "pieceBits", "nPieces", "inputSize", "dst", "dstCap")


def call(fn, head, src_ptr, offs, lens, pieces, input_size, dst_ptr, cap, **override):
    """fn(*head, src, srcOff, srcLen, nSrc, pieceSrc, pieceBitOff, pieceBits, nPieces, inputSize, dst, dstCap) with any argument
    replaced by name (None: a null pointer) -> the return value"""
    so, sl = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int64)
    ps = np.ascontiguousarray([p[0] for p in pieces], dtype=np.int32)
    po = np.ascontiguousarray([p[1] for p in pieces], dtype=np.int64)
    pw = np.ascontiguousarray([p[2] for p in pieces], dtype=np.int64)
    ptr = lambda a: a.ctypes.data if len(a) else None
    a = dict(zip(ARGS, (src_ptr, ptr(so), ptr(sl), len(so), ptr(ps), ptr(po), ptr(pw), len(ps), int(input_size), dst_ptr, int(cap))))
    assert set(override) <= set(ARGS), override
    a.update(override)
    return int(fn(*head, *[a[k] for k in ARGS]))


def bound(case):
    return kz.knz_splice_bound(case.bits())


# ---- refusals ----
class Refusal:
    """a call that must be refused with `code` (kz_last_error holds `text` in the device form, which has a context) and leave dst
    untouched.  cap: None = the bound; override: arguments replaced by name"""

    def __init__(self, name, code, sources, pieces, text=None, lens=None, input_size=0, cap=None, **override):
        self.name, self.code, self.text, self.override, self.cap = name, code, text, override, cap
        self.case = Case(name, sources, pieces, input_size, lens=lens)


def refusals(compress):
    chain, ent, bs, chk = SETTINGS[1]
    A = compress(chain, ent, bs, _data(bs, 6, 333), chk)
    B = compress(chain, ent, bs, _data(bs, 2, 50, 30), chk)
    ia, ib = kz.knz_index(A), kz.knz_index(B)
    good = [(0, o, w) for o, w in ia["blocks"][:4]] + [(1, o, w) for o, w in ib["blocks"]] + [(0, o, w) for o, w in ia["blocks"][4:]]
    out = []
    add = lambda *a, **k: out.append(Refusal(*a, **k))
    # bad arguments
    for name in ("src", "srcOff", "srcLen", "pieceSrc", "pieceBitOff", "pieceBits", "dst"):
        add("null " + name, -18, [A, B], good, **{name: None})
    add("nSrc 0", -18, [A, B], good, nSrc=0)
    add("nSrc -1", -18, [A, B], good, nSrc=-1)
    add("nPieces -1", -18, [A, B], good, nPieces=-1)
    add("inputSize -1", -18, [A, B], good, input_size=-1)
    add("dstCap -1", -18, [A, B], good, cap=-1)
    add("srcLen -1", -18, [A, B], good, lens=[len(A), -1])
    for v in (-1, 2, 1 << 30):
        add("pieceSrc %d" % v, -18, [A, B], good[:5] + [(v,) + good[5][1:]] + good[6:])
    # a bad header, in a source that pieces name and in one that none names
    import refinputs
    for what, bad, code in refinputs.header_faults(B):
        add("header of a named source: " + what, -code, [A, bad], good, text="source 1: ")
        add("header of an unnamed source: " + what, -code, [bad, A], [(1, o, w) for o, w in ia["blocks"]], text="source 0: ")
    add("a source of 10 bytes", -2, [A, B], good[:4], lens=[len(A), 10], text="source 1: ")
    # sources that disagree in each of the four
    D = _data(bs, 2, 50, 30)
    for what, (c2, e2, b2, k2) in (("the transform word", ("LZ", ent, bs, chk)), ("the entropy id", (chain, "HUFFMAN", bs, chk)),
                                   ("the block size", (chain, ent, 2 * bs, chk)), ("the checksum kind", (chain, ent, bs, 64))):
        other = compress(c2, e2, b2, D, k2)
        add("sources differ in " + what, -18, [A, B, other], good, text="source 2 differs from source 0 in " + what)
    # pieces that do not match their source: the index mutants of the seekable calls, and a piece named with the other source
    for mname, i, offs, ws in knzrange.index_mutants(A, ia):
        add("piece " + mname, -18, [A, B], [(1, o, w) for o, w in ib["blocks"]] + [(0, o, w) for o, w in zip(offs, ws)],
            text="piece %d does not match its source" % (i + len(ib["blocks"])))
    add("piece of the other source", -18, [A, B], good[:4] + [(0,) + good[4][1:]] + good[5:], text="piece 4 does not match its source")
    add("piece behind a cut", -18, [A, B], good, lens=[ia["blocks"][-1][0] // 8 + 3, len(B)], text="piece %d does not match its source" % (len(good) - 1))
    add("two bad pieces", -18, [A, B], [good[0], (0, 5, 5), good[1], (1, 0, 0)], text="piece 1 does not match its source")
    # a bad piece and no room: the piece comes first
    add("a bad piece and no room", -18, [A, B], good[:3] + [(0, 177, 64)], cap=30, text="piece 3 does not match its source")
    # no room
    add("no room: 0 bytes", -12, [A, B], good, cap=0)
    add("no room: the header alone", -12, [A, B], good, cap=22)
    add("no room for the end marker of no pieces", -12, [A, B], [], cap=20)
    return out, Case("refusal-base", [A, B], good, 0)
