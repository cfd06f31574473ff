"""The many-stream write without a GPU: the two entry points are exported and bound, and the case set of tests/storewritecases.py is
worth running -- with KZ_STREAM_CHUNK = 3 every header group is cut by chunk seams, chunks hold touched blocks of several streams,
streams lie in several chunks, kept blocks lie before, between and behind touched ones, copies ride along; the continuation
emissions of the NONE&NONE streams start at all eight bit phases in slots that share 16-byte units; every emitted byte has one
writer per launch; and the patch segments of all streams are what knzwrite.resolve makes of each stream's ranges."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import knzwrite
import manycases as mc
import storecases as sc
import storewritecases as wc

NONE = ("NONE", "NONE")


def _call(four):
    sts = wc.streams()
    rngs = wc.call(sts)
    group = sc.groups_of([wc.chain_of(s, four) for s in range(len(sts))], rngs)
    return sts, rngs, group, wc.merged_plan(sts, rngs, group, wc.CHUNK)


CALLS = {"one chain": False, "four chains": True}


def test_the_names_are_exported_and_bound(built):
    L = ctypes.CDLL(kz.LIB_PATH)
    for name, res in (("kz_write_bytes_many_bound", ctypes.c_int64), ("kz_write_bytes_many_device", ctypes.c_int32)):
        assert hasattr(L, name) and name in kz.ABI_SYMBOLS, name
        assert getattr(kz.load_library(), name).restype is res
    for name in ("write_bytes_many_bound", "write_bytes_many_device"):
        assert callable(getattr(kz, name)), name
    assert callable(kz.KnzStore.write_many) and callable(kz.KnzStore.write)
    assert kz.load_library().kz_abi_version() == 3
    names = [kz.load_library().kz_get_kernel_name(i).decode() for i in range(kz.load_library().kz_get_kernel_count())]
    assert "k_knz_splice_many" in names and "k_knz_splice" in names and "k_knz_write" in names


def test_the_bound_is_the_single_bound_per_stream(built):
    lib = kz.load_library()
    bits = [[8216] * 3, [], [100, 1 << 20], [8224]]
    total, caps = kz.write_bytes_many_bound(bits_to_index(bits), [1024, 1024, 4096, 65536])
    assert caps == [kz.write_bytes_bound(b, bs) for b, bs in zip(bits, [1024, 1024, 4096, 65536])] and total == sum(caps)
    first = np.asarray([0, 3, 3, 5, 6], dtype=np.int64)
    flat = np.asarray([w for b in bits for w in b], dtype=np.int64)
    bs = np.asarray([1024, 1024, 4096, 65536], dtype=np.int32)
    assert lib.kz_write_bytes_many_bound(first.ctypes.data, flat.ctypes.data, bs.ctypes.data, 4, None) == total       # slotCap may be NULL
    assert lib.kz_write_bytes_many_bound(None, None, None, 0, None) == 0
    bad = bs.copy()
    bad[2] = 1000                                                                        # no block size
    assert lib.kz_write_bytes_many_bound(first.ctypes.data, flat.ctypes.data, bad.ctypes.data, 4, None) == -18
    down = first.copy()
    down[2] = 2                                                                          # a descending indexFirst
    assert lib.kz_write_bytes_many_bound(down.ctypes.data, flat.ctypes.data, bs.ctypes.data, 4, None) == -18
    assert lib.kz_write_bytes_many_bound(first.ctypes.data, flat.ctypes.data, bs.ctypes.data, -1, None) == -18


def bits_to_index(bits):
    return [[(0, w) for w in b] for b in bits]


@pytest.mark.parametrize("which", sorted(CALLS))
def test_the_set_reaches_the_seams(which):
    sts, rngs, group, P = _call(CALLS[which])
    assert len(sts) == 15 and [s.parts for s in sts[12:14]] == sc.JOINED and all(s.table is None for s in sts[:12] + sts[14:])
    assert any(l < wc.BS for s in sts[12:14] for l in s.lens[:-1])                          # short blocks in the middle, with tables
    named = {r[0] for r in rngs}
    assert named == set(range(len(sts))) - {wc.UNNAMED}                                  # one stream that no range names
    rows, chunks = P.rows, P.chunks
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    assert [r for _, rs in chunks for r in rs] == list(range(len(rows)))
    assert all(len({rows[r][0] for r in rs}) == 1 for _, rs in chunks)                   # a chunk never mixes header groups
    for g in set(group.values()):                                                        # every header group is cut by a seam
        mine = [c for c in chunks if c[0] == g]
        assert len(mine) >= 2, (which, g, "a group that no seam cuts")
        assert all(len(rs) == wc.CHUNK for _, rs in mine[:-1]) and 1 <= len(mine[-1][1]) <= wc.CHUNK
    assert len(set(group.values())) == (4 if CALLS[which] else 1)
    assert any(len({rows[r][1] for r in rs}) >= 3 for _, rs in chunks), (which, "no chunk with touched blocks of three streams")
    per_stream = {}
    for c, (_, rs) in enumerate(chunks):
        for r in rs:
            per_stream.setdefault(rows[r][1], set()).add(c)
    assert any(len(c) >= 2 for c in per_stream.values()), (which, "no stream in two chunks")
    assert all(sorted(cs) == list(range(min(cs), max(cs) + 1)) for cs in per_stream.values())   # a stream's rows lie side by side
    # kept blocks before, between and behind the touched ones
    t = P.touched[4]
    assert t[0] > 0 and t[-1] < len(sts[4].lens) - 1 and any(b - a > 1 for a, b in zip(t, t[1:]))
    # named streams of which no byte survives: copies, one of them empty; and a range buried whole under a later one
    assert P.copies == [2, 9, 14] and len(sts[9].lens) == 0 and len(sts[14].lens) == 7 > wc.CHUNK
    assert all(n == 0 for s, _, n in rngs if s in (2, 9, 14))
    buried = [i for i, (s, o, n) in enumerate(rngs) if n and not any(g["range"] == i for g in P.segs)]
    assert buried and {rngs[i][0] for i in buried} >= {3}
    # wholly covered blocks with a table (left out of the decode) and without one (decoded all the same)
    with_table = [(s, k) for (_, s, k), c in zip(rows, P.covered) if c]
    assert (12, 1) in with_table and (12, 2) in with_table and (13, 3) in with_table and (13, 5) in with_table
    assert all(sts[s].table is not None for s, _ in with_table)
    assert sts[12].lens[1] == 1 and sts[12].lens[2] == 15 and sts[13].lens[3] == 16     # the short middle blocks
    for s, k in ((5, 0), (7, 1), (8, 9)):
        segs, touched, cov = knzwrite.resolve(wc.stream_ranges(s, sts[s].lens), sts[s].starts())
        assert k in cov and sts[s].table is None and not P.covered[rows.index((group[s], s, k))]
    # overlapping ranges of one stream that ranges of other streams separate in call order
    mine = [i for i, r in enumerate(rngs) if r[0] == 0]
    over = [(a, b) for a in mine for b in mine if a < b and rngs[a][2] and rngs[b][2] and rngs[a][1] < rngs[b][1] + rngs[b][2] and rngs[b][1] < rngs[a][1] + rngs[a][2]]
    assert over and all(any(rngs[i][0] != 0 for i in range(a + 1, b)) for a, b in over)
    # interleaved: the stream changes from one range to the next nearly everywhere, and every stream keeps its own order
    assert sum(1 for a, b in zip(rngs, rngs[1:]) if a[0] != b[0]) > len(rngs) // 2
    for s in named:
        assert sc.of_stream(rngs, s)[0] == wc.stream_ranges(s, sts[s].lens), s


@pytest.mark.parametrize("which", sorted(CALLS))
def test_patch_segments_are_the_resolved_ranges_of_every_stream(which):
    sts, rngs, group, P = _call(CALLS[which])
    D = wc.data_places(rngs)
    total = D[-1]
    owned = bytearray(total)                                                             # bytes of the packed data that some segment takes
    for s in P.use:
        mine, idx = sc.of_stream(rngs, s)
        local, touched, cov = knzwrite.resolve(mine, sts[s].starts())
        Dl = [0]
        for _, n in mine:
            Dl.append(Dl[-1] + n)
        want = sorted(((idx[g["range"]], g["block"], g["off"], g["len"], D[idx[g["range"]]] + g["src"] - Dl[g["range"]]) for g in local), key=lambda x: (x[1], x[2]))
        got = [(g["range"], g["block"], g["off"], g["len"], g["src"]) for g in P.segs if g["stream"] == s]
        assert got == want, (which, s)
        assert P.touched[s] == touched, (which, s)
        assert [k for (_, t, k), c in zip(P.rows, P.covered) if t == s and c] == (cov if sts[s].table is not None else []), (which, s)
    for g in P.segs:
        assert g["len"] > 0 and sum(owned[g["src"]:g["src"] + g["len"]]) == 0, (which, "two segments take one byte of the data")
        owned[g["src"]:g["src"] + g["len"]] = b"\1" * g["len"]
        i = g["range"]
        assert rngs[i][0] == g["stream"] and D[i] <= g["src"] and g["src"] + g["len"] <= D[i + 1]
    # the segments of a chunk lie in row order, a row's by offset: disjoint inside every row
    for c in range(len(P.chunks)):
        mine = [(g["slot"], g["off"], g["len"]) for g in P.segs if g["chunk"] == c]
        assert mine == sorted(mine) and all(a[0] != b[0] or a[1] + a[2] <= b[1] for a, b in zip(mine, mine[1:])), (which, c)
    # patched through the segments alone = the ranges one after the other, stream by stream
    new = b"".join(wc.payloads(rngs))
    for s in P.use:
        old = bytes([(7 * s + 1) & 0xFF]) * sts[s].n
        mine, idx = sc.of_stream(rngs, s)
        want = knzwrite.apply(old, mine, [new[D[i]:D[i + 1]] for i in idx])
        assert knzwrite.apply_segments(old, sts[s].starts(), [g for g in P.segs if g["stream"] == s], new) == want, (which, s)


def _slots(sts, P):
    caps = []
    for s, st in enumerate(sts):
        c = kz.write_bytes_bound([wc.none_bits(l) for l in st.lens], wc.BS)
        caps.append(c + (c & 1))                                                         # even: every slot starts at an odd offset
    return caps, mc.slots(caps)[0]


@pytest.mark.parametrize("which", sorted(CALLS))
def test_continuation_emissions_start_at_all_eight_phases_in_slots_that_share_units(built, which):
    sts, rngs, group, P = _call(CALLS[which])
    launches, sizes = wc.none_layout(P, sts, wc.CHUNK)                                  # (bits of the other chains' blocks: stand-ins; a stream's places depend on its own alone)
    none = [s for s in P.use if wc.chain_of(s, CALLS[which]) == NONE]
    assert len(none) >= 4
    phases, first = set(), set()
    for la in launches:
        assert len({sp["stream"] for sp in la}) == len(la), "two spans of one stream in a launch"
        for sp in la:
            if sp["stream"] not in none:
                continue
            if sp["start"] == 0:
                assert sp["hdr"] == wc.header_bits(sts[sp["stream"]].n) // 8 and sp["stream"] not in first
                first.add(sp["stream"])
            else:
                assert sp["hdr"] == 0 and sp["stream"] in first
                phases.add(sp["start"] & 7)
    assert first == set(none)
    assert phases == set(range(8)), (which, sorted(phases))
    assert any(not sp["pieces"] for la in launches for sp in la), "no span without a piece"
    caps, offs = _slots(sts, P)
    assert all(o & 1 for o in offs) and all(c % 2 == 0 for c in caps)
    gaps = [offs[i + 1] - offs[i] - caps[i] for i in range(len(offs) - 1)]
    assert gaps == [mc.SLOT_GAPS[i % 3] for i in range(len(gaps))]
    assert any(g < 16 for g in gaps)                                                     # neighbouring slots share 16-byte units
    for s in P.use:
        assert sizes[s] <= caps[s]
        assert sizes[s] == (wc.header_bits(sts[s].n) + sum(5 + wc.lw(wc.none_bits(l)) + wc.none_bits(l) for l in sts[s].lens) + 8 + 7) // 8


@pytest.mark.parametrize("base", [0, 5, 15])
def test_every_emitted_byte_has_one_writer_per_launch(built, base):
    sts, rngs, group, P = _call(False)
    launches, sizes = wc.none_layout(P, sts, wc.CHUNK)
    caps = wc.tight_caps(sizes, len(sts))                                                # slots that end where their streams end: neighbours share units
    offs = mc.slots(caps)[0]
    assert all(o & 1 for o in offs)
    addr = {s: base + offs[s] for s in range(len(sts))}
    total = base + offs[-1] + caps[-1] + 16
    done = {s: 0 for s in P.use}                                                         # the bytes of a stream that earlier launches finished
    mid = shared = 0
    for la in launches:
        writers = np.zeros(total, dtype=np.uint8)
        units = wc.model_units(la, addr)
        for u in units:
            sp = la[u["span"]]
            d = addr[sp["stream"]]
            assert d + (sp["start"] >> 3) <= u["lo"] < u["hi"] <= d + ((sp["end"] + 7) >> 3), "a unit writes outside its span"
            assert u["addr"] <= u["lo"] and u["hi"] <= u["addr"] + 16
            writers[u["lo"]:u["hi"]] += 1
        # unit0: a prefix sum that grows strictly with the span
        first_unit = [min(i for i, u in enumerate(units) if u["span"] == j) for j in range(len(la))]
        assert first_unit == sorted(set(first_unit)) and first_unit[0] == 0
        want = np.zeros(total, dtype=np.uint8)
        for sp in la:
            d = addr[sp["stream"]]
            lo, hi = d + (sp["start"] >> 3), d + ((sp["end"] + 7) >> 3)
            assert not want[lo:hi].any(), "two spans of a launch share a byte"
            want[lo:hi] = 1
            assert hi <= d + caps[sp["stream"]]
            assert (sp["start"] + 7) >> 3 >= done[sp["stream"]] - (1 if sp["start"] & 7 else 0)
            if sp["start"] & 7:                                                          # the byte that keeps its high bits: one lane reads and writes it
                mid += 1
                assert done[sp["stream"]] == (sp["start"] >> 3) + 1
                assert sum(1 for u in units if u["lo"] <= lo < u["hi"]) == 1
            else:
                assert done[sp["stream"]] == sp["start"] >> 3
            done[sp["stream"]] = (sp["end"] + 7) >> 3
        assert writers.tobytes() == want.tobytes(), "a byte of a span with no writer or with two"
        # two spans of neighbouring slots in one aligned unit of memory: a unit each
        by_addr = {}
        for u in units:
            by_addr.setdefault(u["addr"], []).append(u["span"])
        assert all(len(v) == len(set(v)) for v in by_addr.values())
        shared += sum(1 for v in by_addr.values() if len(v) > 1)
    assert mid >= 8 and done == sizes
    assert shared > 0, "no aligned unit that two spans share"
