"""Case set and models for the byte-addressed reads (kz_read_bytes / kz_read_bytes_device): the ranges asked of a stream of known
block lengths, model A (what every range must deliver: plain slicing), the plan's segments restated in Python, and model B (the
unit enumeration of the copy kernel k_knz_read: which 16-byte destination units a segment visits and how).  The streams are
knzrange.streams() as they are.  Nothing here touches the GPU."""
import numpy as np

import knzrange

CHUNK = knzrange.CHUNK        # KZ_STREAM_CHUNK of the seam cases
INVALID_FILE = -15
BATCH_STREAM = "bwt-64k"      # the stream of the 4096-record batch
LEAD = [(0, l) for l in range(16)]   # leading slots of 0 .. 15 bytes: the slot starts behind them take all 16 destination phases


def starts(lens):
    """the byte offset table of blocks of the given lengths: nblocks + 1 entries"""
    return [0] + [int(x) for x in np.cumsum(lens)]


def ranges(lens):
    """[(offset, size)] for a stream whose blocks have the given lengths, in the order they are asked"""
    B, n, nb = starts(lens), sum(lens), len(lens)
    out = list(LEAD)
    out += [(0, 0), (B[1], 0), (n, 0)]                                                   # empty
    for e in B[1:-1]:                                                                    # one byte at every block edge +- 1
        out += [(e - 1, 1), (e, 1), (e + 1, 1)]
    out += [(n - 1, 1), (0, 1)]
    out += [(B[0], lens[0]), (B[nb - 1], lens[nb - 1]), (B[2], lens[2])]                 # whole blocks
    out += [(B[1], B[3] - B[1]), (B[2] - 3, lens[2] + 6), (B[3], B[6] - B[3]), (B[1] + 5, B[4] - B[1] - 9)]   # two and three blocks
    out += [(0, n)]                                                                      # the whole stream
    out += [(B[1] - 17, l) for l in range(34)]                                           # lengths 0 .. 33 at one offset, across an edge
    out += [(B[2] + 1, l) for l in (15, 16, 17, 31, 32, 33)]                             # and at an odd one inside a block
    out += [(n - 5, 100), (n - 1, 2), (B[nb - 1] - 2, lens[nb - 1] + 50)]                # cut at the end
    out += [(n, 10), (n + 1, 1), (n + 10 ** 6, 10), (1 << 62, 5), ((1 << 63) - 2, 5)]    # at the end, far behind it, an end past int64
    out += [(B[1] + 7, 40)] * 3                                                          # repeats
    out += [(B[2] + 10, 100), (B[2] + 60, 100), (B[2] + 10, 20)]                         # overlaps
    out += [(B[k] - 2, 4) for k in range(nb - 1, 0, -1)]                                 # descending
    out += [(B[1] + p, 24) for p in range(4)]                                            # all 4 source word phases
    return out


def batch(lens, count=4096, seed=77):
    """the 4096-record batch: records of 1 .. 48 bytes at seeded offsets (all four source word phases by construction), behind the
    16 leading slots: enough units for many workgroups, and several segments in every wave"""
    rng = np.random.default_rng(seed)
    n = sum(lens)
    sizes = rng.integers(1, 49, count)
    offs = rng.integers(0, n - 48, count)
    offs = (offs & ~3) | (np.arange(count) & 3)
    B = starts(lens)
    offs[:8] = [B[k + 1] - 5 for k in range(8)]                                          # some of them across block edges
    return list(LEAD) + [(int(o), int(s)) for o, s in zip(offs, sizes)]


# ---- model A: what a call must deliver ----------------------------------------------------------------------------------------------
def model_a(blocks, bs, rngs, table=None):
    """blocks: the decoded blocks of the stream (bytes each); table: the caller's blockByteOff or None -> [(got, bytes or None)].
    Without a table block k is taken to hold bytes [k bs, (k + 1) bs): a block other than the last that is shorter fails the ranges
    that touch it with INVALID_FILE."""
    nb = len(blocks)
    lens = [len(b) for b in blocks]
    if table is None:
        B = [k * bs for k in range(nb)] + [((nb - 1) * bs + lens[-1]) if nb else 0]
        ok = [lens[k] == bs or k == nb - 1 for k in range(nb)]
    else:
        B = list(table)
        ok = [lens[k] == B[k + 1] - B[k] for k in range(nb)]
    end = B[nb]
    out = []
    for o, s in rngs:
        hi = min(o + s, end)
        if o >= hi:
            out.append((0, b""))
            continue
        touched = [k for k in range(nb) if B[k] < hi and (B[k + 1] if k < nb - 1 or table is not None else nb * bs) > o]
        if not all(ok[k] for k in touched):
            out.append((INVALID_FILE, None))
            continue
        data = b"".join(blocks[k][max(o, B[k]) - B[k]:hi - B[k]] for k in touched)
        assert len(data) == hi - o
        out.append((hi - o, data))
    return out


# ---- the plan's segments (knz_read_plan, kz_knz_host.h) ------------------------------------------------------------------------------
def segments(B, rngs, chunk=None):
    """B: nblocks + 1 block starts; -> (distinct covering blocks ascending, [segment]) with segment = dict(block, off, dst, len,
    range, chunk): one range cut with one block, in dst order; chunk = the block's place among the distinct blocks // chunk"""
    nb, end = len(B) - 1, B[-1]
    segs, D = [], 0
    for i, (o, s) in enumerate(rngs):
        d, at, left = D, o, (min(s, end - o) if o < end else 0)
        D += s
        if left <= 0:
            continue
        k = int(np.searchsorted(np.asarray(B, dtype=np.int64), o, side="right")) - 1
        while left > 0:
            l = min(left, B[k + 1] - at)
            segs.append(dict(block=k, off=at - B[k], dst=d, len=l, range=i, chunk=0))
            at, d, left, k = at + l, d + l, left - l, k + 1
    blocks = sorted({g["block"] for g in segs})
    rank = {k: r for r, k in enumerate(blocks)}
    for g in segs:
        g["chunk"] = rank[g["block"]] // chunk if chunk else 0
    return blocks, segs


# ---- model B: the kernel's unit enumeration ----------------------------------------------------------------------------------------------
def model_b(segs, base, row_len):
    """segs: segments of one launch; base: the destination's address mod 16; row_len: the bytes of a source row (the block size; rows
    are 16-byte aligned) -> [unit] with unit = dict(seg, addr, lo, hi, kind): segment `seg` visits the aligned unit at address
    `addr` (in bytes from the destination's aligned base) and writes destination bytes [lo, hi) of it; kind is "wide" (one 16-byte
    store of aligned 32-bit loads inside the row) or "bytes".  unit0 of a segment is the number of units in front of it."""
    out = []
    for j, g in enumerate(segs):
        a = base + g["dst"]
        for addr in range(a & ~15, a + g["len"], 16):
            lo, hi = max(addr, a), min(addr + 16, a + g["len"])
            kind = "bytes"
            if hi - lo == 16:
                p = g["off"] + (lo - a)                                                   # the source byte, from the row's first
                al = p & ~3
                if al + (20 if p & 3 else 16) <= row_len:
                    kind = "wide"
            out.append(dict(seg=j, addr=addr, lo=lo, hi=hi, kind=kind))
    return out
