"""The case set of the many-stream write (kz_write_bytes_many_device) and the merged write plan restated in plain Python
(knz_write_many_plan, kz_knz_host.h, and the emit of kz_stream_device.hip): fifteen streams of BS = 1024 byte blocks, two of them
joined from shorter ones (short blocks in the middle: they carry tables of block starts), the ranges written to them interleaved
over the streams by a seeded permutation, the later-wins segments of every stream, the rows by header group, stream and block, the
chunks, and per chunk the emissions of every stream with their bit ranges, launch by launch.  Under NONE&NONE a block's bits follow
from its length alone (none_bits), so the whole layout of such a call is known without a GPU.  Nothing here touches the GPU or a
stream's bytes.  tests/test_knz_store_write_cases.py shows that the set reaches the seams, tests/test_gpu_knz_store_write.py runs it."""
import numpy as np

import knzread
import knzwrite
import manycases as mc
import storecases as sc

BS = 1024
CHUNK = sc.CHUNK                  # KZ_STREAM_CHUNK of the seam cases
SEED = 0x3717E
HDR_BITS = 176                    # the stream header of a stream with fewer than 2^16 bytes of data; 160 for an empty one
# the streams' data lengths; JOINED's numbers (storecases) name entries of this list
LENGTHS = [12 * BS + 1, 1, 15, 16, 11 * BS, BS - 1, BS + 1, 3 * BS, 9 * BS + 15, 0, 5 * BS + 100, 7 * BS]
UNNAMED = 1                       # no range names it
POISON = 0xA5


def streams():
    """storecases.Stream objects: the twelve of LENGTHS, the two joined ones (with tables), and one more of seven blocks"""
    out = [sc.Stream("len-%d-%d" % (i, n), sc.block_lengths(n, BS)) for i, n in enumerate(LENGTHS)]
    for j, parts in enumerate(sc.JOINED):
        out.append(sc.Stream("joined-%d" % j, [l for p in parts for l in sc.block_lengths(LENGTHS[p], BS)], parts))
    out.append(sc.Stream("len-14-%d" % (7 * BS), sc.block_lengths(7 * BS, BS)))
    return out


def chain_of(s, four):
    return mc.CHAINS[s % 4] if four else mc.CHAINS[0]


def stream_ranges(s, lens):
    """[(offset, size)] written to stream s, in the stream's own order"""
    B, n, nb = knzread.starts(lens), sum(lens), len(lens)
    if s == 0:      # every block touched: its rows fill several chunks; overlaps that other streams' ranges separate in call order
        return [(B[k] + 5 + k, 3) for k in range(nb - 1)] + [(B[3] + 100, 200), (n - 1, 1), (B[3] + 150, 20), (B[3] + 90, 30)]
    if s == UNNAMED:
        return []
    if s == 2:      # named, and no byte survives: a copy
        return [(0, 0)]
    if s == 3:      # the first range is buried whole under the second
        return [(2, 4), (0, 10)]
    if s == 4:      # kept blocks before, between and behind the touched ones
        return [(B[2] + 7, 9), (B[7] - 3, 6), (B[9] + 1000, 24)]
    if s == 5:      # the only block wholly covered, without a table: it is decoded all the same
        return [(0, n)]
    if s == 6:
        return [(BS - 4, 5)]
    if s == 7:      # block 1 wholly covered, without a table
        return [(B[1], BS)]
    if s == 8:
        return [(B[2] - 2, BS + 4), (B[8] + 3, 900), (B[9], 15), (B[5] + 17, 33), (B[8] + 500, 100)]
    if s == 9:      # the empty stream: a copy of no blocks
        return [(0, 0)]
    if s == 10:
        return [(B[1] + 3, 10), (B[3] - 1, 2), (n - 50, 50)]
    if s == 11:
        return [(B[2] + 1, 2), (B[5] - 1, 2)]
    if s == 14:     # zero lengths alone: a copy of seven blocks, more than an emit launch takes
        return [(B[2], 0), (n, 0)]
    if s == 12:     # joined-0: the short middle blocks 1 (1 byte) and 2 (15 bytes) wholly covered, with a table
        return [(B[1] - 3, 3 + 1 + 15 + 4), (B[12], 1), (B[13] + 1, 1), (B[20] + 9, 2000)]
    if s == 13:     # joined-1: the 16-byte block 3 wholly covered by the union of two ranges, with a table
        return [(B[3], 8), (B[5], 1), (B[3] + 8, 8), (B[14] + 2, 13)]
    raise ValueError(s)


def call(sts, only=None):
    """[(stream, offset, size)] of one call: the ranges of all streams interleaved by the seeded permutation; a stream keeps the order
    of its own ranges"""
    names = [s for s in range(len(sts)) if only is None or s in set(only)]
    per = {s: stream_ranges(s, sts[s].lens) for s in names}
    order = np.concatenate([np.full(len(per[s]), s, dtype=np.int64) for s in names])
    order = order[np.random.default_rng(SEED).permutation(len(order))]
    at, out = {s: 0 for s in names}, []
    for s in order:
        s = int(s)
        out.append((s,) + per[s][at[s]])
        at[s] += 1
    return out


def payloads(rngs):
    return [knzwrite.payload(4000 + i, n) for i, (_, _, n) in enumerate(rngs)]


def data_places(rngs):
    D = [0]
    for _, _, n in rngs:
        D.append(D[-1] + n)
    return D


# ---- the format, as far as lengths go --------------------------------------------------------------------------------------------------
def lw(w):
    return 3 if w < 8 else (w >> 3).bit_length() - 1 + 4


def none_bits(length):
    """the bits of a NONE&NONE block of `length` >= 1 bytes without a checksum: the mode byte, the byte of skip flags, the size field of
    one byte per 8 bits of the length's magnitude, the bytes"""
    return 8 * (2 + ((length.bit_length() - 1) >> 3) + 1 + length)


def header_bits(n):
    """160 + 16 per 16 bits of the size field (an empty stream declares no size)"""
    return 160 if n == 0 else 160 + 16 * ((n.bit_length() - 1) // 16 + 1)


# ---- the plan of one stream: later wins, without a per-byte array and without a sweep ----------------------------------------------------
def stream_segments(B, rngs_with_place):
    """B: nblocks + 1 block starts; rngs_with_place: [(offset, size, place in the packed data, number in the call)] in the stream's own
    order -> (segments, touched blocks, covered blocks); a segment is dict(range, block, off, len, src).  From the last range to the
    first, each takes what no later one has taken."""
    free = [(0, B[-1])]
    segs = []
    for o, n, place, number in reversed(rngs_with_place):
        assert 0 <= o and o + n <= B[-1]
        rest = []
        for a, b in free:
            lo, hi = max(a, o), min(b, o + n)
            if lo >= hi:
                rest.append((a, b))
                continue
            if a < lo:
                rest.append((a, lo))
            if hi < b:
                rest.append((hi, b))
            k = int(np.searchsorted(np.asarray(B, dtype=np.int64), lo, side="right")) - 1
            while lo < hi:
                l = min(hi, B[k + 1]) - lo
                if l > 0:
                    segs.append(dict(range=number, block=k, off=lo - B[k], len=l, src=place + lo - o))
                    lo += l
                k += 1
        free = sorted(rest)
    segs.sort(key=lambda g: (g["block"], g["off"]))
    touched = sorted({g["block"] for g in segs})
    have = {k: sum(g["len"] for g in segs if g["block"] == k) for k in touched}
    covered = [k for k in touched if have[k] == B[k + 1] - B[k]]
    return segs, touched, covered


# ---- the merged plan --------------------------------------------------------------------------------------------------------------------
class Plan:
    pass


def merged_plan(sts, rngs, group, chunk, use=None):
    """sts: the streams; rngs: the call; group[s]: the header group of a named stream; chunk: rows per chunk; use: the named streams
    that are written (all by default) -> Plan with rows = [(group, stream, block)], covered = [bool] per row (a table gave the
    length), chunks = [(group, [row numbers])], segs = the patch segments of all streams with row, chunk and slot, per stream touched."""
    P = Plan()
    D = data_places(rngs)
    named = sorted({r[0] for r in rngs})
    use = named if use is None else [s for s in named if s in set(use)]
    P.named, P.use, P.touched, P.stream_segs = named, use, {}, {}
    rows, covered = [], {}
    for s in use:
        mine = [(o, n, D[i], i) for i, (t, o, n) in enumerate(rngs) if t == s]
        segs, touched, cov = stream_segments(sts[s].starts(), mine)
        P.touched[s], P.stream_segs[s] = touched, segs
        for k in touched:
            rows.append((group[s], s, k))
            covered[(s, k)] = sts[s].table is not None and k in cov
    rows.sort()
    P.rows = rows
    P.covered = [covered[(s, k)] for _, s, k in rows]
    P.chunks = []
    for r, (g, s, k) in enumerate(rows):
        if P.chunks and P.chunks[-1][0] == g and len(P.chunks[-1][1]) < chunk:
            P.chunks[-1][1].append(r)
        else:
            P.chunks.append((g, [r]))
    place = {(s, k): r for r, (_, s, k) in enumerate(rows)}
    chunk_of = {r: c for c, (_, rs) in enumerate(P.chunks) for r in rs}
    P.segs = []
    for _, s, k in rows:
        for g in P.stream_segs[s]:
            if g["block"] == k:
                r = place[(s, k)]
                P.segs.append(dict(g, stream=s, row=r, chunk=chunk_of[r], slot=r - P.chunks[chunk_of[r]][1][0]))
    P.copies = [s for s in use if not P.touched[s]]
    return P


def emissions(P, sts, old_bits, new_bits, hdr_bits, cap):
    """The emit launches.  old_bits[s][k]: the bits of block k of stream s; new_bits[(s, k)]: the bits of a recoded block; hdr_bits[s];
    cap: pieces and spans per launch -> [launch], a launch = [span], a span = dict(stream, start, end, hdr (bytes), pieces = [(block,
    recoded, prefix start, payload start, bits)]).  A stream's first span starts at bit 0 and carries its header."""
    launches, cur, state = [], [], dict(npc=0, span=None)
    pos, nxt, done, started = {}, {s: 0 for s in P.use}, {s: 0 for s in P.use}, set()

    def flush():
        if cur:
            launches.append(list(cur))
        del cur[:]
        state["npc"] = 0

    def begin(s, start, hdr):
        state["span"] = dict(stream=s, start=start, end=None, hdr=hdr, pieces=[])

    def end(bit):
        sp = state["span"]
        state["span"] = None
        if bit <= sp["start"]:
            state["npc"] -= len(sp["pieces"])
            return
        sp["end"] = bit
        cur.append(sp)
        if len(cur) == cap:
            flush()

    def piece(at, p):
        if state["npc"] == cap:
            s = state["span"]["stream"]
            end(at)
            flush()
            begin(s, at, 0)
        state["span"]["pieces"].append(p)
        state["npc"] += 1

    def emit(s, k1, recoded, tail):
        p = pos[s] if s in started else hdr_bits[s]
        begin(s, p if s in started else 0, 0 if s in started else hdr_bits[s] // 8)
        for k in range(nxt[s], k1):
            w = new_bits[(s, k)] if k in recoded else old_bits[s][k]
            pay = p + 5 + lw(w)
            piece(p, (k, k in recoded, p, pay, w))
            p = pay + w
        p += tail
        started.add(s)
        pos[s], nxt[s] = p, k1
        end(p)

    copies, at = list(P.copies), 0
    for _, rs in P.chunks:
        i = 0
        while i < len(rs):
            s = P.rows[rs[i]][1]
            j = i
            while j < len(rs) and P.rows[rs[j]][1] == s:
                j += 1
            last = done[s] + (j - i) == len(P.touched[s])
            k1 = len(sts[s].lens) if last else P.rows[rs[j - 1]][2] + 1
            emit(s, k1, {P.rows[r][2] for r in rs[i:j]}, 8 if last else 0)
            done[s] += j - i
            i = j
        while at < len(copies) and 0 < len(cur) < cap and len(sts[copies[at]].lens) <= cap - state["npc"]:
            emit(copies[at], len(sts[copies[at]].lens), set(), 8)
            at += 1
        flush()
    while at < len(copies):
        emit(copies[at], len(sts[copies[at]].lens), set(), 8)
        at += 1
    flush()
    return launches, {s: (pos[s] + 7) >> 3 for s in pos}


def none_layout(P, sts, cap):
    """emissions for a call whose streams are all NONE&NONE: every block's bits follow from its length"""
    old = {s: [none_bits(l) for l in sts[s].lens] for s in P.use}
    new = {(s, k): old[s][k] for _, s, k in P.rows}
    return emissions(P, sts, old, new, {s: header_bits(sts[s].n) for s in P.use}, cap)


def tight_caps(sizes, nstreams):
    """slot capacities that end where the new streams end, rounded up to even (so that every slot starts at an odd offset); two
    bytes for a stream that is not written"""
    return [(sizes.get(s, 2) + 1) & ~1 for s in range(nstreams)]


# ---- the kernel's units (k_knz_splice_many) ------------------------------------------------------------------------------------------------
def model_units(launch, slot_addr):
    """launch: spans; slot_addr[s]: the address of stream s's slot -> [unit] = dict(span, addr, lo, hi): the lane of the 16-byte aligned
    unit at `addr` writes the bytes [lo, hi) (addresses) of span number `span`.  unit0 of a span is the number of units in front."""
    out = []
    for j, sp in enumerate(launch):
        d = slot_addr[sp["stream"]]
        first, last = d + (sp["start"] >> 3), d + ((sp["end"] + 7) >> 3)
        for addr in range(first & ~15, last, 16):
            lo, hi = max(addr, first), min(addr + 16, last)
            if lo < hi:
                out.append(dict(span=j, addr=addr, lo=lo, hi=hi))
    return out
