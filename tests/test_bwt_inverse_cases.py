"""The inverse BWT's case set (tests/bwtinvcases.py) held against its plan model (tests/bwtinvmodel.py) on the CPU: the model gives
the oracle's verdict and bytes on every case, every seam the set is built for is reached (asserted from the model's geometry, not
from a case's name), well-formed blocks are stitched unless built for the fallback, and nine mutants of the model are each noticed
by some case.  No GPU.

katmodels.bwt_block_inverse restates the Java's test `src.index > src.length` (BWT.java:206), which refuses a block whose payload
is shorter than its header; the oracle and the device do not have it.  One case of the set is that short (a payload of one byte
behind a header of two), and there the comparison is with the oracle alone."""
import functools

import numpy as np
import pytest

import bwtinvcases as C
import bwtinvmodel as M
import katmodels
import oracle


@functools.lru_cache(maxsize=None)
def want(frame, cap=None):
    """the oracle's inverse of a frame: (verdict, bytes; none where it refuses)"""
    ok, out = oracle.transform_inverse("BWT", frame, max(len(frame), 1) if cap is None else cap)
    return ok, out if ok else b""


@functools.lru_cache(maxsize=None)
def plan(name, maxN=None):
    return M.plan(C.by_name(name).frame, maxN)


def got(p):
    return p.ok, p.out if p.ok else b""


def all_plans():
    return [(c, plan(c.name)) for c in C.cases()]


def test_model_oracle_and_katmodels_agree_on_every_case():
    for c, p in all_plans():
        assert got(p) == want(c.frame), (c.name, p.path, p.refused or p.why_fallback)
        if c.text is not None:
            assert p.ok and p.out == c.text, c.name
        if 0 < p.n < p.header:
            continue                                              # (see the module's docstring)
        try:
            ok_k, out_k = katmodels.bwt_block_inverse(c.frame, max(len(c.frame), 1))
        except katmodels.JavaException:
            ok_k, out_k = False, b""
        assert (ok_k, out_k if ok_k else b"") == want(c.frame), ("katmodels", c.name)
    assert sum(1 for c, p in all_plans() if 0 < p.n < p.header) == 1


def test_block_streams_are_the_encoders_and_decode_like_the_frame():
    """block_stream() frames a BWT stage's output the way the encoder does (oracle.encode_block), and the oracle's block decoder makes
    of such a stream what its inverse BWT makes of the frame: the batched device tests may expect the single-block result"""
    n = 0
    for c in C.cases():
        if not c.frame:
            continue
        s, w = C.block_stream(c.frame)
        if c.text is not None and len(c.text) > 15 and c.frame == C.fwd(c.text):
            so, wo, sf, pl = oracle.encode_block("BWT", "NONE", c.text)
            assert (s, w) == (so, wo), c.name
            n += 1
        bs = max(len(c.frame), 64)
        r, by = oracle.decode_block("BWT", "NONE", bs, s, w, bs + 512)
        ok, out = want(c.frame)
        assert (r >= 0, by if r >= 0 else b"") == (ok, out), (c.name, r)
    assert n >= 40


def test_well_formed_blocks_are_stitched_unless_built_for_the_fallback():
    for c, p in all_plans():
        if c.text is None or p.n < 2:
            continue
        assert p.path == ("fallback" if c.fallback else "stitched"), (c.name, p.why_fallback)
        assert not p.refused


def test_parse_seams_are_reached():
    ps = [p for c, p in all_plans()]
    acc = [p for p in ps if not p.refused and p.mode | p.header]
    assert {p.n for p in acc} >= set(C.LENGTH_SEAMS) - {0}
    assert any(c.frame == b"" for c in C.cases())
    # one index below 256 bytes, eight from there on; every index width with both; the payload 2..5 and 9, 17, 25, 33 bytes in
    assert {p.header for p in acc if p.chunks == 1 and p.n >= 2} == {2, 3, 4, 5}
    assert {p.header for p in acc if p.chunks == 8} == {9, 17, 25, 33}
    assert all((p.chunks == 1) == (p.n < 256) for p in acc)
    assert max(p.n for p in acc if p.chunks == 1) == 255 and min(p.n for p in acc if p.chunks == 8) == 256
    assert {p.n & 7 == 0 for p in acc if p.chunks == 8} == {True, False}
    p257 = next(p for p in acc if p.n == 257)
    assert (257 - 7 * 33, (257 >> 3) + 1) == (26, 33) and p257.path == "stitched"
    assert {p.n % 16 for p in acc if p.n > 4000} >= {0, 1, 15}                   # the histogram's 16-byte pieces
    assert {p.n for p in acc} >= {1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193}
    assert any(p.header == p.chunks * p.p_size + 1 and p.n == 0 and p.path == "trivial" and p.mode | p.header for p in acc)
    refusals = {p.refused for p in ps}
    assert refusals >= {"blockSize < headerSize", "chunks > 8", "chunks != (n < 256 ? 1 : 8)", "pi >= 0x7FFFFFFF", "p0 outside 1..n",
                        "index outside 0..n-1"}
    frames = [c.frame for c in C.cases() if c.frame]
    assert {(f[0] >> 2) & 7 for f in frames} >= {0, 3, 4, 5, 6, 7}
    assert any(((f[0] >> 2) & 7) == 0 and len(f) - 1 - ((f[0] & 3) + 1) >= 256 for f in frames)          # one index, n >= 256
    assert any(((f[0] >> 2) & 7) == 3 and 0 <= len(f) - 1 - 8 * ((f[0] & 3) + 1) < 256 for f in frames)  # eight indexes, n < 256
    assert any(len(f) == 1 + (1 << ((f[0] >> 2) & 7)) * ((f[0] & 3) + 1) - 1 for f in frames)              # blockSize = headerSize - 1
    assert any((f[0] & 3) == 3 and f[1:5] == b"\x7f\xff\xff\xff" for f in frames)


def test_scatter_seams_are_reached():
    pays = [np.frombuffer(c.frame[plan(c.name).header:], dtype=np.uint8) for c in C.cases() if not plan(c.name).refused and plan(c.name).n >= 64]
    assert any(len(set(a.tolist())) == 1 and len(a) > M.TILE for a in pays)                     # every row takes the one-symbol shortcut
    foreign = set()
    for a in pays:
        vals, cnt = np.unique(a, return_counts=True)
        if len(vals) == 2 and cnt.min() == 1:
            at = int(np.flatnonzero(a == vals[cnt.argmin()])[0])
            foreign.add("lane0" if at % 64 == 0 and at > 0 else "lane63" if at % 64 == 63 else "other")
            if at == 1024:
                foreign.add("wave1")
    assert foreign >= {"lane0", "lane63", "wave1"}
    assert any(len(set(a.tolist())) == 256 and all(len(set(a[r:r + 64].tolist())) == 64 for r in range(0, len(a) - 63, 64)) for a in pays)
    def only_in_last_partial_row(a):
        last = (len(a) // 64) * 64
        return len(a) % 64 and len(a) > M.TILE and any(int(s) not in set(a[:last].tolist()) for s in set(a[last:].tolist()))
    assert any(only_in_last_partial_row(a) for a in pays)


def test_walk_seams_are_reached():
    ps = {c.name: p for c, p in all_plans() if p.path == "stitched" and p.n >= 2}
    lens = set()
    for p in ps.values():
        lens |= set(p.seg_len[:p.G + 1].tolist())
    assert lens >= set(C.SEGMENT_LENGTHS) | {1}
    # segments of one byte whose successor is the next grid walker: most of the grid
    assert any(int(((p.seg_len[:p.G] == 1) & (p.seg_next[:p.G] >= 0)).sum()) >= p.G - 3 and p.G >= 60 for p in ps.values())
    assert any((p.prim[0] - 1) % p.S == 0 for p in ps.values())                                   # the head on a grid row
    assert any(bool((p.start_link[:p.G] == M.END).any()) for p in ps.values())                    # END at a grid walker's first step
    assert any(bool((p.start_link[:p.G] == 0).any()) for p in ps.values())                        # row 0 linked from a grid row
    # one walker carries the block, at S = 64 ...
    assert any(M.longest_segment(p) >= p.n - 72 and p.n >= 4000 and p.S == 64 for p in ps.values())
    # ... and at S = 128, which a small block only has beside a block of 1 051 649 bytes
    assert M.grid(1051648)[0] == 6 and M.grid(1051649)[0] == 7
    wide = [plan(c.name, 1051649) for c in C.cases() if c.name.endswith("_s128")]
    assert wide and all(p.S == 128 and p.path == "stitched" for p in wide)
    assert any(M.longest_segment(p) >= p.n - 72 for p in wide)
    assert all(plan(c.name, 1051648).S == 64 for c in C.cases() if c.name.endswith("_s128"))


def test_chunk_pool_slack():
    """demand against maxChunks over the well-formed cases: never above it, except in the one block found that the pool cannot hold
    (the head on a grid row with a long segment behind it: two walkers record the same bytes).  That block decodes through the
    literal walkers, and the model and the oracle agree on its bytes (first test)."""
    slack = {c.name: p.max_chunks - p.demand for c, p in all_plans() if c.text is not None and p.n >= 2}
    over = sorted(k for k, v in slack.items() if v < 0)
    assert over == ["pool_overflow"], over
    p = plan("pool_overflow")
    assert (p.path, p.why_fallback, p.max_chunks - p.demand) == ("fallback", "chunk pool", -47) and (p.prim[0] - 1) % p.S == 0
    least = min((v, k) for k, v in slack.items() if v >= 0)
    print("least slack:", least, "random 8 KiB:", slack["len_8191"])
    assert least[0] == 13 and least[1].startswith("periodic_")
    assert plan("pool_overflow", 1051649).path == "stitched"      # beside a long neighbour the pool is the batch's: room enough


def test_resolve_seams_are_reached():
    ps = [p for c, p in all_plans() if p.path == "stitched" and p.n >= 2]
    assert {p.NSP for p in ps} >= {255, 256, 257}
    assert {p.G for p in ps} >= {15, 16, 17, 32, 33}
    assert {p.rounds for p in ps} >= {4, 8, 9}
    mono = lambda o, sign: len(o) >= 3 and all(sign * (b - a) > 0 for a, b in zip(o, o[1:]))
    # ascending: all splitters but 0, whose row is the text head itself in a sorted text (no row links to the head)
    assert any(mono(p.splitter_order, 1) and p.splitter_order == tuple(range(1, p.NG)) and (p.prim[0] - 1) == 0 for p in ps)
    assert any(mono(p.splitter_order, -1) and len(p.splitter_order) == p.NG for p in ps)         # all splitters, descending


def test_targeted_damage_is_decided_where_the_set_says():
    base = C.by_name("damage_base")
    reasons = {}
    for c, p in all_plans():
        if c.text is None and p.path == "fallback":
            reasons.setdefault(p.why_fallback, []).append((c, p))
    for k in range(1, 8):
        hit = [c for c, p in reasons["head %d is not %d * ckSize in" % (k, k)] if c.name.startswith("index_")]
        assert hit, k
        for c in hit:                                             # the reference succeeds, with other bytes: so must the fallback
            ok, out = want(c.frame)
            assert ok and out != base.text and len(out) == len(base.text), c.name
    assert any(c.name.startswith("index_0") for c, p in reasons["head 0 does not reach END in n steps"])
    assert any(p.cycle_guard for c, p in all_plans())
    assert not any(p.ok for c, p in all_plans() if c.name.startswith("small_"))                 # the 0xFF link past a table of 200 rows
    assert plan("last_byte_cut").n == plan("damage_base").n - 1
    assert any(p.why_fallback == "a walker gave up" for c, p in all_plans())


def test_batches():
    b = C.batches()
    for name in ("small", "mid"):
        blocks = b[name]
        maxN = max(len(c.frame) for c in blocks)
        assert not blocks[0].frame and not blocks[-1].frame and any(not c.frame for c in blocks[2:-2])
        kinds = {("well" if c.text is not None else "damaged") for c in blocks if c.frame}
        assert kinds == {"well", "damaged"}
        for c in blocks:
            if c.frame:
                assert got(M.plan(c.frame, maxN)) == want(c.frame), (name, c.name)
    assert {c.name for c in b["small"]} >= {c.name for c in C.cases() if c.group == "small" and c.frame}
    assert len(b["many"]) == 2000 and all(len(c.text) <= 300 for c in b["many"])                 # k_bwti_ord's second pass of 1024
    assert max(len(c.frame) for c in b["beside_1051648"]) == 1051648 and max(len(c.frame) for c in b["beside_1051649"]) == 1051649


MUTANTS = {
    "steps < cap": dict(cap_inclusive=False),
    "the partial tail dropped": dict(partial_tail=False),
    "ckSize = n >> 3": dict(ck_round_up=False),
    "i <= pIdx": dict(link_le=True),
    "splitter period 15": dict(spl_stop=15),
    "chunk start seq * 120": dict(chunk_pitch=120),
    "the heads' position check removed": dict(head_check=False),
    "the 1 / 8 switch at 255": dict(one_index_below=255),
    "logS from the block's own length": dict(grid_from_batch=False),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_of_the_model_is_caught(mutant):
    """each slip changes the model's verdict (refused / stitched / fallback, applied or not) or its bytes on some case; the cases are
    taken alone and, for the grid's choice, beside the neighbour that sets S = 128"""
    v = M.Variant(**MUTANTS[mutant])
    caught = []
    if mutant == "steps < cap":                                   # cap = n below 2^20, and no walker reads n + 1 links: the large pair only
        pool = [(c, None) for c in C.large_cases() if c.name.startswith("cap_plus_")]
    else:
        pool = [(c, None) for c in C.cases() if c.group == "small"] + [(c, 1051649) for c in C.cases() if c.group == "small" and len(c.frame) > 3000]
    for c, maxN in pool:
        a = plan(c.name, maxN)
        b = M.plan(c.frame, maxN, v)
        if (a.ok, a.path, a.out if a.ok else b"") != (b.ok, b.path, b.out if b.ok else b""):
            caught.append(c.name)
            if len(caught) >= 3:
                break
    print(mutant, "caught by", caught)
    assert caught, mutant


def test_large_cases():
    """a megabyte each: the valid block past the walk cap goes to the literal walkers, the long one inside the cap is stitched, and
    the exact pair (cap + 1 links stitched, cap + 2 not) where the search found it"""
    seen = {}
    for c in C.large_cases():
        p = plan(c.name)
        assert got(p) == want(c.frame) and p.out == c.text, c.name
        assert p.path == ("fallback" if c.fallback else "stitched"), (c.name, p.why_fallback)
        seen[c.name] = (M.longest_segment(p) - p.cap, p.S, p.n)
        assert p.n > 1 << 20 and p.cap == 1 << 20
    print(seen)
    assert seen["past_cap"][0] > 1 and seen["past_cap"][1] == 128 and plan("past_cap").why_fallback == "a walker gave up"
    assert -(1 << 19) < seen["stitched_long"][0] <= 0 and seen["stitched_long"][1] == 128
    assert seen["neighbour_1051648"][1] == 64 and seen["neighbour_1051649"][1] == 128
    for d in C.PAIR_SEEDS:
        assert seen["cap_plus_%d" % d][0] == d
