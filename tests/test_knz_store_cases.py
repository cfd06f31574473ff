"""The many-stream index and read without a GPU: the two entry points are exported and bound, and the case set of
tests/storecases.py is worth running -- with KZ_STREAM_CHUNK = 3 every header group is cut by chunk seams, ranges lie across them,
chunks hold blocks of several streams and streams lie in several chunks; every delivered byte has one owner, and the segments tile
every range (the per-call form of tests/test_knz_read_cases.py's checks, through the restated merged plan)."""
import ctypes

import pytest

import kanzi_amd as kz
import knzread
import manycases as mc
import storecases as sc

BS = 1024


def _one_chain():
    sts = sc.streams(BS)
    rngs = sc.call(sts)
    return sts, rngs, {s: 0 for s in range(len(sts))}


def _four_chains():
    """the same streams, stream s under chain s mod 4: four header groups in one call"""
    sts = sc.streams(BS)
    rngs = sc.call(sts)
    return sts, rngs, sc.groups_of([mc.CHAINS[s % 4] for s in range(len(sts))], rngs)


CALLS = {"one chain": _one_chain, "four chains": _four_chains}


def test_the_names_are_exported_and_bound(built):
    L = ctypes.CDLL(kz.LIB_PATH)
    for name in ("kz_knz_index_many_device", "kz_read_bytes_many_device"):
        assert hasattr(L, name) and name in kz.ABI_SYMBOLS, name
        assert getattr(kz.load_library(), name).restype is ctypes.c_int64
    for name in ("knz_index_many_device", "read_bytes_many_device"):
        assert callable(getattr(kz, name)), name
    assert callable(kz.KnzStore.read_many) and callable(kz.KnzStore.read) and callable(kz.KnzStore.from_compress_many)
    assert kz.load_library().kz_abi_version() == 3
    names = [kz.load_library().kz_get_kernel_name(i).decode() for i in range(kz.load_library().kz_get_kernel_count())]
    assert "k_knz_check_rows" in names and "k_knz_read" in names and "k_knz_unpack_many" in names


def test_the_set_names_every_stream_and_every_phase():
    sts, rngs, _ = _one_chain()
    assert len(sts) == 32 and [s.parts for s in sts[30:]] == sc.JOINED and all(s.table is None for s in sts[:30])
    assert all(s.table == kz.block_byte_offsets([sts[p].n for p in s.parts], BS) for s in sts[30:])
    assert any(l < BS for s in sts[30:] for l in s.lens[:-1])                            # short blocks in the middle
    assert {r[0] for r in rngs} == set(range(len(sts)))                                  # no stream is left without ranges
    assert [r[1:] for r in rngs[:16]] == knzread.LEAD
    D, phases = 0, set()
    for s, o, n in rngs:
        phases.add(D % 16)
        D += n
    assert phases == set(range(16))
    # interleaved: the stream changes from one range to the next nearly everywhere, and every stream keeps its own order
    assert sum(1 for a, b in zip(rngs, rngs[1:]) if a[0] != b[0]) > len(rngs) // 2
    for s in range(len(sts)):
        mine, _ = sc.of_stream(rngs[16:], s)
        assert mine == sc.stream_ranges(sts[s].lens), s
    # a call that names some streams in no range
    rngs = sc.call(sts, skip=(0, 9, 30))
    assert {r[0] for r in rngs} == set(range(len(sts))) - {0, 9, 30}


@pytest.mark.parametrize("which", sorted(CALLS))
def test_chunks_of_three_cut_every_group(which):
    sts, rngs, group = CALLS[which]()
    B = [s.starts() for s in sts]
    rows, chunks, segs = sc.merged_plan(B, group, rngs, sc.CHUNK)
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    assert {(s, k) for _, s, k in rows} == {(s, k) for s in range(len(sts)) for k in range(len(sts[s].lens))}    # the set touches every block
    for g in set(group.values()):
        mine = [c for c in chunks if c[0] == g]
        assert len(mine) >= 2, (which, g, "a group that no seam cuts")
        assert all(len(rs) == sc.CHUNK for _, rs in mine[:-1]) and 1 <= len(mine[-1][1]) <= sc.CHUNK
    assert all(len({rows[r][0] for r in rs}) == 1 for _, rs in chunks)                   # a chunk never mixes header groups
    assert [r for _, rs in chunks for r in rs] == list(range(len(rows)))
    spans = {}
    for g in segs:
        spans.setdefault(g["range"], set()).add(g["chunk"])
    assert any(len(c) == 2 for c in spans.values()) and any(len(c) >= 3 for c in spans.values()), which
    assert any(len({rows[r][1] for r in rs}) >= 3 for _, rs in chunks), (which, "no chunk with blocks of three streams")
    per_stream = {}
    for c, (_, rs) in enumerate(chunks):
        for r in rs:
            per_stream.setdefault(rows[r][1], set()).add(c)
    assert any(len(c) >= 2 for c in per_stream.values())
    # a stream's rows lie side by side, and a chunk's segments stay in dst order
    assert all(sorted(cs) == list(range(min(cs), max(cs) + 1)) for cs in per_stream.values())
    for c in range(len(chunks)):
        d = [g["dst"] for g in segs if g["chunk"] == c]
        assert d == sorted(d), (which, c)


@pytest.mark.parametrize("which", sorted(CALLS))
def test_every_delivered_byte_has_one_owner(which):
    sts, rngs, group = CALLS[which]()
    B = [s.starts() for s in sts]
    _, _, segs = sc.merged_plan(B, group, rngs, sc.CHUNK)
    total = sum(n for _, _, n in rngs)
    owned = bytearray(total)
    for g in segs:
        assert sum(owned[g["dst"]:g["dst"] + g["len"]]) == 0, (which, "two segments own a byte")
        owned[g["dst"]:g["dst"] + g["len"]] = b"\1" * g["len"]
    by_range = {}
    for g in segs:
        by_range.setdefault(g["range"], []).append(g)
    at = 0
    for r, (s, o, n) in enumerate(rngs):
        got = max(min(o + n, B[s][-1]) - o, 0)
        mine = by_range.get(r, [])
        assert sum(g["len"] for g in mine) == got and all(g["len"] > 0 and g["stream"] == s for g in mine), (which, r)
        assert [g["dst"] for g in mine] == [at + sum(x["len"] for x in mine[:i]) for i in range(len(mine))], (which, r)
        assert bytes(owned[at + got:at + n]) == b"\0" * (n - got), (which, r, "the tail of a cut slot")
        at += n
    # the kernel's units of one chunk's launch at some destination phases: one writer per delivered byte of that chunk, none elsewhere
    import numpy as np
    for base in (0, 5, 15):
        writers = np.zeros(base + total + 16, dtype=np.uint8)
        for c in sorted({g["chunk"] for g in segs}):
            for u in knzread.model_b([g for g in segs if g["chunk"] == c], base, BS):
                writers[u["lo"]:u["hi"]] += 1
        assert writers[base:base + total].tobytes() == bytes(owned), (which, base)
        assert not writers[:base].any() and not writers[base + total:].any(), (which, base)


def test_model_a_of_the_call_is_the_streams_models():
    sts = sc.streams(BS)
    rngs = sc.call(sts)
    blocks = [[bytes([(7 * s + k) & 0xFF]) * l for k, l in enumerate(st.lens)] for s, st in enumerate(sts)]
    want = sc.model_a(blocks, BS, rngs, [st.table for st in sts])
    assert len(want) == len(rngs) and all(g >= 0 for g, _ in want)
    for (s, o, n), (g, b) in zip(rngs, want):
        assert b == b"".join(blocks[s])[o:o + n] and g == len(b)
    # without their tables the joined streams have byte addresses only where their blocks are whole
    want = sc.model_a(blocks, BS, rngs, [None] * len(sts))
    assert knzread.INVALID_FILE in {g for (s, _, _), (g, _) in zip(rngs, want) if s >= 30}
    assert all(g >= 0 for (s, _, _), (g, _) in zip(rngs, want) if s < 30)
