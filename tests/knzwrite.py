"""Case set and model for the byte-addressed writes (kz_write_bytes / kz_write_bytes_device): the ranges written to a stream of
known block lengths, `apply` (the plain sequential definition: the ranges one after the other in argument order, the later one
wins) and `resolve` (what the plan must make of them: disjoint surviving segments, the touched blocks, the wholly covered ones),
both per byte and in plain Python so that they share nothing with knz_write_plan's sort and sweep.  The streams are knzread's (that
is knzrange.streams()) at block sizes of 1 KiB and 4 KiB, and one longer stream for the 4096-record batch.  Nothing here touches
the GPU."""
import numpy as np

import knzrange
import knzread

CHUNK = 2                     # KZ_STREAM_CHUNK of the seam cases: touched blocks go in steps of two
STREAM_NAMES = ["none-1k-last1", "bwt-1k-x32", "lz-4k-x64", "text-4k-last1", "short-middle"]
RECORD, RECORDS, SLOT = 64, 4096, 80
# the batch: 4096 records of 64 bytes without an overlap need 256 KiB of data; slots of 80 bytes leave room for odd offsets
BATCH = knzrange.Stream("lz-4k-batch", "LZ", "HUFFMAN", 4096, RECORDS * SLOT + 77, checksum=32)

starts = knzread.starts


def streams():
    return [s for s in knzrange.streams() if s.name in STREAM_NAMES]


def payload(seed, n):
    return np.random.default_rng(1000 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _fill(name, rngs):
    seed = sum(ord(c) for c in name) * 131
    return [(int(o), payload(seed + i, int(n))) for i, (o, n) in enumerate(rngs)]


def corners(lens):
    """[(offset, size)]: every seam of the plan in one call, for blocks of the given lengths (at least 8)"""
    B, n, nb = starts(lens), sum(lens), len(lens)
    out = [(7, 1)]                                                                       # a 1-byte segment
    out += [(B[1], 3), (B[2] - 2, 2)]                                                    # a block's first byte, a block's last byte
    out += [(B[2] + 5, B[4] - B[2] - 1)]                                                 # three blocks, the middle one wholly covered
    out += [(B[5], 0), (n, 0)]                                                           # zero length
    out += [(B[k] - 2, min(4, n - B[k] + 2)) for k in range(nb - 1, 4, -1)]              # descending, across block edges
    out += [(B[1] + 40, 30)] * 2                                                         # the same range twice (with different bytes)
    out += [(B[5] + 100, 200), (B[5] + 150, 20)]                                         # nested: the earlier survives as two pieces
    out += [(B[6] + 10 + 15 * i, 20) for i in range(6)]                                  # a chain of partial overlaps
    out += [(B[6] + 300, 16), (B[6] + 290, 40)]                                          # buried: none of the first one's bytes survives
    out += [(B[7], lens[7] // 2), (B[7] + lens[7] // 2, lens[7] - lens[7] // 2)]         # a block covered only by a union
    out += [(n - 3, 3)]                                                                  # ends exactly at the end of data
    return out


def cases(lens):
    """[(name, [(offset, payload)])] for a stream whose blocks have the given lengths, each one call"""
    B, n, nb = starts(lens), sum(lens), len(lens)
    c = corners(lens)
    out = [("corners", c),
           ("whole", [(0, n)]),                                                          # one range equal to the whole data
           ("whole-first", [(0, n)] + c),                                                # everything else lies on it
           ("whole-last", c + [(0, n)]),                                                 # it buries everything
           ("one-byte", [(B[3] + 1, 1)]),
           ("kept-run", [(B[1] + 9, 11), (B[nb - 2] + 3, 5)]),                           # touched blocks far apart: kept runs in front, between and behind
           ("first-and-last", [(0, 16), (n - 1, 1)]),
           ("across-seam", [(B[1] + 5, 3), (B[3] - 10, 20), (B[5] - 1, 2)]),             # with KZ_STREAM_CHUNK = 2: touched blocks 1 2 | 3 4 | 5, ranges across both seams
           ("empty", []),
           ("zero-lengths", [(0, 0), (B[2], 0), (n, 0)]),
           ("unaligned", [(B[1] + p, 16 + p) for p in range(1, 20, 3)] + [(B[2] + 33, 100), (B[3] + 15, 17)])]
    return [(name, _fill(name, r)) for name, r in out]


def batch(n, overlap, seed=5):
    """the 4096-record batch for n bytes of data -> [(offset, payload)]: records of 64 bytes at seeded offsets; overlap=False: every
    record in an 80-byte slot of its own, at an odd place in it, the slots in seeded order"""
    rng = np.random.default_rng(seed)
    if overlap:
        offs = rng.integers(0, n // 8 - RECORD, RECORDS)                                 # 4096 x 64 bytes into an eighth of the data
    else:
        assert n >= RECORDS * SLOT
        offs = rng.permutation(RECORDS) * SLOT + rng.integers(0, SLOT - RECORD + 1, RECORDS)
    return [(int(o), payload(7000 + i, RECORD)) for i, o in enumerate(offs)]


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def apply(data, ranges, payloads):
    """the plain sequential definition: ranges = [(offset, size)] applied one after the other in argument order"""
    out = bytearray(data)
    for (o, n), p in zip(ranges, payloads):
        assert len(p) == n and 0 <= o and o + n <= len(out), (o, n, len(out))
        out[o:o + n] = p
    return bytes(out)


def resolve(ranges, table):
    """ranges = [(offset, size)], table = the nblocks + 1 block starts -> (segments, touched blocks, wholly covered blocks).
    A segment is dict(range, block, off, len, src): `len` bytes of range `range` at byte `off` of block `block`, taken from byte
    `src` of the packed new bytes; every byte of the data has at most one, the last range in argument order that covers it."""
    B = [int(b) for b in table]
    n = B[-1]
    owner = np.full(n, -1, dtype=np.int64)
    D = [0]
    for i, (o, s) in enumerate(ranges):
        assert 0 <= o and o + s <= n, (i, o, s, n)
        owner[o:o + s] = i
        D.append(D[-1] + s)
    block_of = np.searchsorted(np.asarray(B, dtype=np.int64), np.arange(n), side="right") - 1
    segs = []
    for p in range(n):
        r = int(owner[p])
        if r < 0:
            continue
        k = int(block_of[p])
        g = segs[-1] if segs else None
        if g and g["range"] == r and g["block"] == k and B[k] + g["off"] + g["len"] == p:
            g["len"] += 1
        else:
            segs.append(dict(range=r, block=k, off=p - B[k], len=1, src=D[r] + p - ranges[r][0]))
    touched = sorted({g["block"] for g in segs})
    covered = [k for k in touched if bool((owner[B[k]:B[k + 1]] >= 0).all())]
    return segs, touched, covered


def apply_segments(data, table, segs, new):
    """the data patched with the segments alone, in any order: what the kernel does"""
    out = bytearray(data)
    for g in reversed(segs):
        at = table[g["block"]] + g["off"]
        out[at:at + g["len"]] = new[g["src"]:g["src"] + g["len"]]
    return bytes(out)
