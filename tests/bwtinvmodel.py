"""A CPU model of the PLAN of the device's inverse BWT (kanzi_amd/csrc/kz_bwt_inv.hip), not only of its bytes: what k_bwti_parse
accepts, the link array of k_bwti_scatter, the grid of walkers of k_bwti_walk1 (segment lengths, successors, the walk cap, the
chunks they take from the pool), the ruling-set ranking and the stitching check of k_bwti_resolve, the placement of the chunks by
k_bwti_copy, and the reference's literal walkers (k_bwti_literal; K/transform/BWTBlockCodec.java:138-213 and BWT.java:245-374)
that finish a block the check refuses.  plan(frame, maxN) returns all of it for one framed block (mode byte, primary indexes,
payload) in a batch whose longest framed block has maxN bytes.

The model restates the kernels' arithmetic; it runs none of their code.  Walks are computed by pointer doubling over the whole
link array (22 numpy rounds for a block of 2^20 bytes), never by stepping a walker, so that the blocks whose single walker carries
a megabyte cost a second.  `Variant` holds one switch per place where a slip is likely; tests/test_bwt_inverse_cases.py turns each
and requires the case set (tests/bwtinvcases.py) to notice.

Two facts about the link array that follow from its construction and that the case set relies on:
 * every row index appears at most once as a link (i - 1 for i < pIdx, i for i >= pIdx, END for i = 0), and row pIdx - 1, the text
   head, appears never: whatever the payload and the primary indexes, the links are one path from the head to END plus disjoint
   cycles.  Two paths cannot merge; damage to a payload byte moves rows from the path into cycles.
 * a link is never >= n, so the walkers' `corrupt link` exit is taken only through a primary index, and k_bwti_parse refuses those."""
import dataclasses

import numpy as np

TILE = 4096            # BI_TILE: rows per workgroup of the histogram and the scatter
MAXSEG = 16448         # BI_MAXSEG
HEADS = 8              # BI_HEADS
CH = 128               # BI_CH
SPL = 16               # BI_SPL
END = -1               # the link behind row 0
HUGE = 1 << 40


@dataclasses.dataclass(frozen=True)
class Variant:
    """the kernels as they are; every other value is a mutant"""
    cap_inclusive: bool = True      # while (steps <= cap)
    partial_tail: bool = True       # the last steps & 7 bytes of a segment are stored
    ck_round_up: bool = True        # ckSize = ceil(n / 8)
    link_le: bool = False           # i <= pIdx -> i - 1
    spl_stop: int = 16              # a sublist ends at a segment whose index is a multiple of BI_SPL
    chunk_pitch: int = CH           # start = seq * BI_CH in k_bwti_copy
    head_check: bool = True         # heads 1..7 sit k * ckSize into the text
    one_index_below: int = 256      # chunks == (n < 256 ? 1 : 8)
    grid_from_batch: bool = True    # logS from the batch's maxN


KERNEL = Variant()


@dataclasses.dataclass
class Plan:
    # parse
    mode: int = 0
    chunks: int = 0
    p_size: int = 0
    header: int = 0
    n: int = 0
    refused: str = ""               # which test of k_bwti_parse refuses the block ("" = accepted)
    prim: tuple = ()                # primary indexes as the kernels hold them (stored value + 1)
    # geometry
    logS: int = 0
    S: int = 0
    G: int = 0
    GS: int = 0
    max_chunks: int = 0
    cap: int = 0
    seg_len: np.ndarray = None      # [G + 8]
    seg_next: np.ndarray = None     # [G + 8]  -1 = END, -2 = the walk gave up
    start_link: np.ndarray = None   # [G + 8]  the link of the row a walker starts on (END = -1)
    reach: np.ndarray = None        # [G + 8]  links from a walker's start to its stop if nothing capped the walk (HUGE: a cycle)
    demand: int = 0                 # chunks the recording walkers take
    # resolve
    NG: int = 0
    NSP: int = 0
    rounds: int = 0
    cycle_guard: bool = False       # a sublist walk ran into `steps > M`
    head_rest: tuple = ()           # bytes from head k to the end of the text, as the ranking finds them
    head_at_end: tuple = ()
    splitter_order: tuple = ()      # grid splitter indexes in the order the head chain meets them
    path: str = ""                  # "refused", "trivial" (n < 2), "stitched" or "fallback"
    why_fallback: str = ""
    # result
    ok: bool = False
    out: bytes = b""


def _ceil_div(a, b):
    return -(-a // b)


def grid(maxN):
    """logS, GS, NS and maxChunks as kz_stage_bwt_inverse picks them for a batch whose longest framed block has maxN bytes"""
    logS = 6
    while _ceil_div(maxN, 1 << logS) > MAXSEG - HEADS - 8:
        logS += 1
    GS = _ceil_div(maxN, 1 << logS) + HEADS
    NS = _ceil_div(max(maxN, 1), TILE) * TILE
    return logS, GS, NS, NS // CH + GS + 4


def parse(frame, v=KERNEL):
    """k_bwti_parse (BWTBlockCodec.java:138-213 and the range tests of BWT.java:261, :305-311)"""
    p = Plan()
    size = len(frame)
    if size == 0:
        return p
    p.mode = frame[0]
    p.chunks = 1 << ((p.mode >> 2) & 7)
    p.p_size = (p.mode & 3) + 1
    p.header = 1 + p.chunks * p.p_size
    if size < p.header:
        p.refused = "blockSize < headerSize"
        return p
    if p.chunks > 8:
        p.refused = "chunks > 8"
        return p
    n = size - p.header
    if p.chunks != (1 if n < v.one_index_below else 8):
        p.refused = "chunks != (n < 256 ? 1 : 8)"
        return p
    prim = [0] * 8
    for i in range(p.chunks):
        pi = int.from_bytes(frame[1 + i * p.p_size:1 + (i + 1) * p.p_size], "big")
        if pi >= 0x7FFFFFFF:
            p.refused = "pi >= 0x7FFFFFFF"
            return p
        prim[i] = pi + 1
    if n >= 2:
        if prim[0] <= 0 or prim[0] > n:
            p.refused = "p0 outside 1..n"
        if p.chunks == 8 and any(t - 1 < 0 or t - 1 >= n for t in prim):
            p.refused = p.refused or "index outside 0..n-1"
        if p.refused:
            return p
    p.n = n
    p.prim = tuple(prim)
    return p


def links(payload, p_idx, v=KERNEL):
    """k_bwti_scatter: row r of the link array holds (next, byte) of the r-th payload byte in stable symbol order"""
    a = np.frombuffer(payload, dtype=np.uint8)
    order = np.argsort(a, kind="stable").astype(np.int64)
    low = order <= p_idx if v.link_le else order < p_idx
    nxt = np.where(low, order - 1, order)
    nxt[order == 0] = END
    return nxt, a[order]


def _run_to_stop(nxt, stop):
    """for every row t: the number of links read from t up to and including the first row whose link is a stop, and that link.
    Rows that never meet one (cycles) get HUGE.  Pointer doubling; stop rows are absorbing."""
    n = len(nxt)
    idx = np.arange(n, dtype=np.int64)
    fin = stop.copy()
    D = np.ones(n, dtype=np.int64)
    E = np.where(stop, nxt, 0)
    P = np.where(stop, idx, nxt)
    for _ in range(max(n, 2).bit_length() + 1):
        u = np.flatnonzero(~fin)
        if len(u) == 0:
            break
        q = P[u]
        Dn = np.minimum(D[u] + D[q], HUGE)
        En, fn, Pn = E[q], fin[q], P[q]
        D[u], E[u], fin[u], P[u] = Dn, En, fn, Pn
    D[~fin] = HUGE
    return D, E


def _literal(nxt, byte, n, prim, v):
    """k_bwti_literal: BWT.java:295-368, the dummy link 0xFF behind row 0 and the failure on a link >= n included"""
    walkers = 1 if n < v.one_index_below else 8
    if walkers == 1:
        ck = n
    else:
        ck = (n >> 3) + (1 if (n & 7) and v.ck_round_up else 0)
    out = bytearray(n)
    nx, by = nxt.tolist(), byte.tolist()
    for lane in range(walkers):
        steps = ck if lane < 7 else n - 7 * ck
        t = prim[lane] - 1
        base = lane * ck
        for i in range(steps):
            if t >= n or t < 0:
                return False, b""
            if base + i < n:
                out[base + i] = by[t]
            t = nx[t]
            if t == END:
                t = 0xFF
    return True, bytes(out)


def plan(frame, maxN=None, v=KERNEL, want_bytes=True):
    """everything the device does with one framed block of a batch whose longest framed block has maxN bytes (want_bytes False:
    the plan without the output bytes, for the searches of the case set)"""
    frame = bytes(frame)
    maxN = len(frame) if maxN is None else maxN
    assert maxN >= len(frame) and maxN < (1 << 24) - 1, "8-byte links are not modelled"
    p = parse(frame, v)
    p.logS, p.GS, _, p.max_chunks = grid(maxN if v.grid_from_batch else len(frame))
    p.S = 1 << p.logS
    if p.refused:
        p.path = "refused"
        return p
    n = p.n
    payload = frame[p.header:]
    if n < 2:
        p.path, p.ok, p.out = "trivial", True, payload
        return p
    S, logS = p.S, p.logS
    G = p.G = _ceil_div(n, S)
    M = G + HEADS
    nxt, byte = links(payload, p.prim[0], v)
    # ---- k_bwti_walk1 ----
    p.cap = min(n, max(1 << 20, S << 5))
    limit = p.cap + 1 if v.cap_inclusive else p.cap               # the most links a walker reads
    stop = (nxt == END) | ((nxt & (S - 1)) == 0) | (nxt >= n)
    D, E = _run_to_stop(nxt, stop)
    heads = 1 if n < v.one_index_below else 8
    starts = [w << logS for w in range(G)] + [p.prim[k] - 1 for k in range(heads)]
    seg_len = np.zeros(M, dtype=np.int64)
    seg_next = np.full(M, -1, dtype=np.int64)
    gave_up = False
    for w, t in enumerate(starts):
        if t >= n:                                                # corrupt link at the first step
            seg_len[w], seg_next[w], gave_up = 0, -2, True
        elif D[t] > limit:
            seg_len[w], seg_next[w], gave_up = limit, -2, True
        else:
            e = int(E[t])
            seg_len[w] = D[t]
            if e == END:
                seg_next[w] = -1
            elif e >= n:
                seg_next[w], gave_up = -2, True
            else:
                seg_next[w] = e >> logS
    p.seg_len, p.seg_next = seg_len, seg_next
    p.reach = np.array([int(D[t]) if t < n else 0 for t in starts], dtype=np.int64)
    p.start_link = np.array([int(nxt[t]) if t < n else -2 for t in starts], dtype=np.int64)
    rec =list(range(G)) + [G]
    p.demand = int(sum(_ceil_div(int(seg_len[w]), CH) for w in rec))
    if gave_up or p.demand > p.max_chunks:
        p.why_fallback = "a walker gave up" if gave_up else "chunk pool"
    # ---- k_bwti_resolve ----
    spl = SPL
    NG = p.NG = _ceil_div(G, spl)
    NSP = p.NSP = NG + HEADS
    p.rounds = 1
    while (1 << p.rounds) < NSP:
        p.rounds += 1
    if not p.why_fallback:
        sl = seg_len.tolist()
        sn = [(-1 if x == -2 else x) for x in seg_next.tolist()]
        first = lambda k: k * spl if k < NG else G + (k - NG)
        spT, spN = [0] * NSP, [None] * NSP
        for k in range(NSP):
            s, x, steps = 0, first(k), 0
            while True:
                s += sl[x]
                nx = sn[x]
                if nx < 0 or nx >= M:
                    break
                if nx >= G or nx % v.spl_stop == 0:
                    spN[k] = NG + (nx - G) if nx >= G else nx // spl
                    break
                if steps > M:
                    p.cycle_guard = True
                    break
                x = nx
                steps += 1
            spT[k] = s & 0xFFFFFFFF
        order, k = [], NG
        while k is not None and len(order) <= NSP:                 # the head chain's grid splitters, for the case set's reach
            if k < NG:
                order.append(k)
            k = spN[k]
        p.splitter_order = tuple(order)
        for _ in range(p.rounds):
            t2 = [(spT[k] + spT[spN[k]]) & 0xFFFFFFFF if spN[k] is not None else spT[k] for k in range(NSP)]
            n2 = [spN[spN[k]] if spN[k] is not None else None for k in range(NSP)]
            spT, spN = t2, n2
        seg_off = [None] * M
        for k in range(NSP):
            x, running, steps = first(k), spT[k], 0
            while True:
                seg_off[x] = n - running if running <= n else None
                if k > NG:
                    break
                running = (running - sl[x]) & 0xFFFFFFFF
                nx = sn[x]
                if nx < 0 or nx >= G or nx % v.spl_stop == 0 or steps > M:
                    break
                x = nx
                steps += 1
        p.head_rest = tuple(spT[NG:NG + HEADS])
        p.head_at_end = tuple(spN[NG + k] is None for k in range(HEADS))
        ck = (n >> 3) + (1 if (n & 7) and v.ck_round_up else 0)
        for k in range(HEADS):
            rk = spT[NG + k]
            if k == 0:
                good = rk == n and p.head_at_end[0] and not p.cycle_guard
            elif n >= v.one_index_below and v.head_check:
                good = p.head_at_end[k] and rk <= n and n - rk == k * ck
            else:
                good = True
            if not good:
                p.why_fallback = p.why_fallback or ("head 0 does not reach END in n steps" if k == 0 else "head %d is not %d * ckSize in" % (k, k))
    if p.why_fallback:
        p.path = "fallback"
        if want_bytes:
            p.ok, p.out = _literal(nxt, byte, n, p.prim, v)
        return p
    # ---- k_bwti_copy: head 0 reaches END after n links, so every row lies on its path and a walker's bytes are a slice of the text ----
    p.path, p.ok = "stitched", True
    if not want_bytes:
        return p
    R, _ = _run_to_stop(nxt, nxt == END)
    text = np.zeros(n, dtype=np.uint8)
    on = R <= n
    text[n - R[on]] = byte[on]
    out = np.full(n, 0xA5, dtype=np.uint8)
    for w in rec:
        ln, off = int(seg_len[w]), seg_off[w]
        if off is None or off + ln > n:
            continue
        t = starts[w]
        at = n - int(R[t]) if R[t] <= n else None
        stored = ln if v.partial_tail else ln & ~7               # bytes of the segment that reached the pool
        got = np.zeros(_ceil_div(ln, CH) * CH, dtype=np.uint8)
        if at is not None:
            got[:stored] = text[at:at + stored]
        if v.chunk_pitch == CH and stored == ln:
            out[off:off + ln] = got[:ln]
            continue
        for seq in range(_ceil_div(stored, CH)):                  # chunks that were allocated
            start = seq * v.chunk_pitch
            if start >= ln:
                continue
            cnt = min(CH, ln - start)
            out[off + start:off + start + cnt] = got[seq * CH:seq * CH + cnt]
    p.out = out.tobytes()
    return p


def longest_segment(p):
    """the longest walk of a recording walker, as long as it would be without the cap"""
    return int(p.reach[:p.G + 1].max()) if p.reach is not None and p.G else 0
