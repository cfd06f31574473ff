"""The case set of the many-stream index and read (kz_knz_index_many_device / kz_read_bytes_many_device): the thirty streams of
manycases.buffers and two streams joined from shorter ones (short blocks in the middle: they carry tables of block starts), the
ranges asked of every one of them, interleaved over the streams by a seeded permutation behind sixteen leading slots, model A of
the whole call (knzread.model_a per stream) and the merged plan restated (knz_read_many_plan, kz_knz_host.h: rows by header group,
stream and block, chunks inside a group, range x block segments).  Nothing here touches the GPU or a stream's bytes: the set is made
of lengths alone.  tests/test_knz_store_cases.py shows that it reaches the seams, tests/test_gpu_knz_store.py runs it."""
import numpy as np

import knzread
import manycases as mc

CHUNK = knzread.CHUNK             # KZ_STREAM_CHUNK of the seam cases
SEED = 0x5703E
JOINED = [[6, 2, 8, 1, 4], [7, 3, 6, 8]]   # the streams of manycases.call_lengths whose join makes a table stream, in this order
LONG = 7                          # a stream of at least this many blocks gets knzread.ranges


def block_lengths(n, bs):
    return [min(bs, n - k * bs) for k in range((n + bs - 1) // bs)]


class Stream:
    """lens: the decoded length of every block; parts: None, or the streams it is joined from; table: None, or its block starts"""

    def __init__(self, name, lens, parts=None):
        self.name, self.lens, self.parts = name, list(lens), parts
        self.n = sum(lens)
        self.table = knzread.starts(lens) if parts is not None else None

    def starts(self):
        return knzread.starts(self.lens)


def streams(bs):
    """the thirty of manycases.call_lengths, then the two joined ones"""
    ns = mc.call_lengths(bs)
    out = [Stream("len-%d-%d" % (i, n), block_lengths(n, bs)) for i, n in enumerate(ns)]
    for j, parts in enumerate(JOINED):
        out.append(Stream("joined-%d" % j, [l for p in parts for l in block_lengths(ns[p], bs)], parts))
    return out


def short_ranges(lens):
    """a stream of fewer than LONG blocks, the empty one included: empty ranges, one byte at every block edge +- 1, the whole
    stream, ranges cut at the end and ranges behind it"""
    B, n = knzread.starts(lens), sum(lens)
    out = [(0, 0), (n, 0), (n // 2, 0)]
    for e in B:
        out += [(x, 1) for x in (e - 1, e, e + 1) if x >= 0]
    out += [(0, n), (0, n + 7)]
    out += [(max(n - 5, 0), 100), (max(n - 1, 0), 2), (n // 3, n)]
    out += [(n, 10), (n + 1, 1), (n + 10 ** 6, 10), (1 << 62, 5), ((1 << 63) - 2, 5)]
    return out


def stream_ranges(lens):
    return knzread.ranges(lens)[len(knzread.LEAD):] if len(lens) >= LONG else short_ranges(lens)


def call(sts, skip=(), only=None):
    """[(stream, offset, size)] of one call over the streams `sts`: sixteen leading slots of 0 .. 15 bytes (every destination phase
    occurs behind them), then the ranges of all streams but those in `skip`, interleaved by the seeded permutation.  A stream keeps
    the order of its own ranges.  only: the streams that are asked at all"""
    names = [s for s in range(len(sts)) if s not in set(skip) and (only is None or s in set(only))]
    first = next(s for s in names if sts[s].n >= 16)
    per = {s: stream_ranges(sts[s].lens) for s in names}
    order = np.concatenate([np.full(len(per[s]), s, dtype=np.int64) for s in names])
    order = order[np.random.default_rng(SEED).permutation(len(order))]
    at = {s: 0 for s in names}
    out = [(first, o, l) for o, l in knzread.LEAD]
    for s in order:
        s = int(s)
        out.append((s,) + per[s][at[s]])
        at[s] += 1
    return out


def of_stream(rngs, s):
    """the ranges of stream s in their call order -> ([(offset, size)], their places in the call)"""
    idx = [i for i, r in enumerate(rngs) if r[0] == s]
    return [rngs[i][1:] for i in idx], idx


# ---- model A of the whole call --------------------------------------------------------------------------------------------------
def model_a(blocks, bs, rngs, tables):
    """blocks[s]: the decoded blocks of stream s (bytes each); tables[s]: its table or None -> [(got, bytes or None)] in call order"""
    out = [None] * len(rngs)
    for s in sorted({r[0] for r in rngs}):
        mine, idx = of_stream(rngs, s)
        for i, w in zip(idx, knzread.model_a(blocks[s], bs, mine, tables[s])):
            out[i] = w
    return out


# ---- the merged plan (knz_read_many_plan) -----------------------------------------------------------------------------------------
def groups_of(headers, rngs):
    """headers[s]: anything that compares equal for streams of one header group -> group[s] for the named streams, numbered in order of
    first appearance in stream order"""
    seen, out = [], {}
    for s in sorted({r[0] for r in rngs}):
        if headers[s] not in seen:
            seen.append(headers[s])
        out[s] = seen.index(headers[s])
    return out


def merged_plan(B, group, rngs, chunk):
    """B[s]: the nblocks + 1 block starts of stream s; group[s]: its header group; chunk: blocks per chunk (a number, or one per group)
    -> (rows, chunks, segs): rows = [(group, stream, block)] ascending, chunks = [(group, [row numbers])], segs = knzread.segments'
    dicts with dst and range counted over the whole call, and stream, row and chunk"""
    segs, D = [], 0
    for i, (s, o, n) in enumerate(rngs):
        _, mine = knzread.segments(B[s], [(o, n)])
        for g in mine:
            g.update(stream=s, dst=g["dst"] + D, range=i)
        segs += mine
        D += n
    rows = sorted({(group[g["stream"]], g["stream"], g["block"]) for g in segs})
    chunks = []
    for r, (g, s, k) in enumerate(rows):
        size = chunk[g] if isinstance(chunk, (list, tuple, dict)) else chunk
        if chunks and chunks[-1][0] == g and len(chunks[-1][1]) < size:
            chunks[-1][1].append(r)
        else:
            chunks.append((g, [r]))
    place = {row: r for r, row in enumerate(rows)}
    chunk_of = {r: c for c, (_, rs) in enumerate(chunks) for r in rs}
    for g in segs:
        g["row"] = place[(group[g["stream"]], g["stream"], g["block"])]
        g["chunk"] = chunk_of[g["row"]]
    return rows, chunks, segs
