"""The case set of the byte-addressed writes (tests/knzwrite.py) without a GPU: the model's disjoint segments reproduce the plain
sequential definition on every case, and the set reaches every seam of the plan, counted here one by one.  Also the public names
of the feature and kz_write_bytes_bound, which needs no context."""
import numpy as np
import pytest

import kanzi_amd as kz
import knzwrite

STREAMS = knzwrite.streams()


def _all():
    """[(stream, case name, table, ranges, payloads, segments, touched, covered)] over the whole set"""
    out = []
    for s in STREAMS:
        lens = s.block_lengths()
        s.data = s.original()
        B = knzwrite.starts(lens)
        for name, writes in knzwrite.cases(lens):
            rngs = [(o, len(p)) for o, p in writes]
            segs, touched, covered = knzwrite.resolve(rngs, B)
            out.append((s, name, B, rngs, [p for _, p in writes], segs, touched, covered))
    return out


@pytest.fixture(scope="module")
def resolved():
    return _all()


def test_the_streams_are_the_ones_the_issue_names():
    assert [s.name for s in STREAMS] == knzwrite.STREAM_NAMES
    assert sorted({s.bs for s in STREAMS}) == [1024, 4096] and all(s.nblocks() <= 40 for s in STREAMS)
    assert {(s.chain, s.ent) for s in STREAMS} == {("NONE", "NONE"), ("BWT+RANK+ZRLT", "ANS0"), ("LZ", "HUFFMAN"), ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0")}
    assert {s.checksum for s in STREAMS} == {0, 32, 64}
    assert any(s.block_lengths()[-1] == 1 for s in STREAMS) and any(s.block_lengths()[-1] % 16 for s in STREAMS if s.block_lengths()[-1] > 1)
    assert knzwrite.BATCH.n >= knzwrite.RECORDS * knzwrite.SLOT and knzwrite.BATCH.bs == 4096


def test_the_segments_reproduce_the_sequential_definition(resolved):
    for s, name, B, rngs, pays, segs, touched, covered in resolved:
        data, new = s.data, b"".join(pays)
        want = knzwrite.apply(data, rngs, pays)
        assert len(want) == len(data)
        assert knzwrite.apply_segments(data, B, segs, new) == want, (s.name, name)
        seen = np.zeros(len(data), dtype=np.int32)                                       # every byte has at most one segment
        for g in segs:
            assert g["len"] > 0 and 0 <= g["off"] and g["off"] + g["len"] <= B[g["block"] + 1] - B[g["block"]], (s.name, name, g)
            seen[B[g["block"]] + g["off"]:B[g["block"]] + g["off"] + g["len"]] += 1
        assert int(seen.max(initial=0)) <= 1, (s.name, name)
        assert touched == sorted({g["block"] for g in segs}) and set(covered) <= set(touched), (s.name, name)


def test_the_set_reaches_every_seam(resolved):
    n_ = dict.fromkeys(["one-byte segment", "segment at a block's first byte", "segment at a block's last byte", "three blocks, the middle wholly covered",
                        "the whole data", "zero length", "descending", "the same range twice", "nested: two pieces survive", "chain of partial overlaps",
                        "buried", "covered by a union only", "ends at the end of data", "short middle block", "no surviving byte", "kept run between touched blocks"], 0)
    for s, name, B, rngs, pays, segs, touched, covered in resolved:
        n, nb = B[-1], len(B) - 1
        blen = [B[k + 1] - B[k] for k in range(nb)]
        by_range = {}
        for g in segs:
            by_range.setdefault(g["range"], []).append(g)
        n_["one-byte segment"] += sum(g["len"] == 1 for g in segs)
        n_["segment at a block's first byte"] += sum(g["off"] == 0 for g in segs)
        n_["segment at a block's last byte"] += sum(g["off"] + g["len"] == blen[g["block"]] for g in segs)
        for r, gs in by_range.items():
            ks = [g["block"] for g in gs]
            for g in gs:
                k = g["block"]
                if g["off"] == 0 and g["len"] == blen[k] and k - 1 in ks and k + 1 in ks and rngs[r][0] > B[k - 1] and rngs[r][0] + rngs[r][1] < B[k + 2]:
                    n_["three blocks, the middle wholly covered"] += 1
            for a, b in zip(gs, gs[1:]):                                                  # two pieces of one range in one block, a later range between them
                if a["block"] == b["block"] and a["off"] + a["len"] < b["off"]:
                    n_["nested: two pieces survive"] += 1
        n_["the whole data"] += sum(r == (0, n) for r in rngs)
        n_["zero length"] += sum(r[1] == 0 for r in rngs)
        n_["descending"] += sum(a[0] > b[0] > c[0] for a, b, c in zip(rngs, rngs[1:], rngs[2:]))
        n_["the same range twice"] += sum(a == b and a[1] > 0 and pa != pb for a, b, pa, pb in zip(rngs, rngs[1:], pays, pays[1:]))
        n_["chain of partial overlaps"] += sum(a[0] < b[0] < a[0] + a[1] < b[0] + b[1] and b[0] < c[0] < b[0] + b[1] < c[0] + c[1] for a, b, c in zip(rngs, rngs[1:], rngs[2:]))
        n_["buried"] += sum(r[1] > 0 and i not in by_range for i, r in enumerate(rngs))
        n_["covered by a union only"] += sum(len({g["range"] for g in segs if g["block"] == k}) > 1 and
                                             not any(g["len"] == blen[k] for g in segs if g["block"] == k) for k in covered)
        n_["ends at the end of data"] += sum(r[1] > 0 and r[0] + r[1] == n for r in rngs)
        n_["short middle block"] += sum(k < nb - 1 and blen[k] < s.bs for k in touched) if s.lens else 0
        n_["no surviving byte"] += not segs
        n_["kept run between touched blocks"] += sum(b - a > 1 for a, b in zip(touched, touched[1:]))
    missing = [k for k, v in n_.items() if v == 0]
    assert not missing, (missing, n_)
    # with KZ_STREAM_CHUNK = CHUNK a range of the set lies across a chunk seam and a kept run does
    for s, name, B, rngs, pays, segs, touched, covered in resolved:
        if name == "across-seam":
            chunk = {k: i // knzwrite.CHUNK for i, k in enumerate(touched)}
            assert any(len({chunk[g["block"]] for g in segs if g["range"] == r}) > 1 for r in range(len(rngs))), (s.name, touched)
        if name == "kept-run":
            assert len(touched) == 2 and touched[1] - touched[0] > knzwrite.CHUNK, (s.name, touched)


def test_the_batches():
    n = knzwrite.BATCH.n
    for overlap in (True, False):
        w = knzwrite.batch(n, overlap)
        assert len(w) == knzwrite.RECORDS and all(len(p) == knzwrite.RECORD and 0 <= o and o + len(p) <= n for o, p in w)
        owner = np.zeros(n, dtype=np.int32)
        for o, p in w:
            owner[o:o + len(p)] += 1
        assert (int(owner.max()) > 4) if overlap else (int(owner.max()) == 1)
        assert len({o & 15 for o, _ in w}) == 16 and any(o // 4096 != (o + 63) // 4096 for o, _ in w)   # every phase, and across block edges


def test_public_names(built):
    for name in ("write_bytes_bound", "write_bytes", "write_bytes_device"):
        assert callable(getattr(kz, name)), name
    assert callable(kz.KnzReader.write_many)
    for name in ("kz_write_bytes_bound", "kz_write_bytes", "kz_write_bytes_device"):
        assert name in kz.ABI_SYMBOLS and hasattr(kz.load_library(), name), name


def test_write_bytes_bound(built):
    """host arrays only, no context: the longest header (26 bytes), per block 39 prefix bits and the longer of its own payload and a
    recoded block's bound, the end marker"""
    for bs in (1024, 4096):
        rec = 8 * kz.max_block_stream_bytes(bs)
        for bits in ([], [8], [rec + 8, 3], [100] * 37):
            want = 26 + (8 + sum(39 + max(b, rec) for b in bits) + 7) // 8
            assert kz.write_bytes_bound(bits, bs) == want, (bs, bits)
    for bits, bs in (([-1], 1024), ([1 << 34], 1024), ([8], 1000), ([8], 0)):
        with pytest.raises(kz.KanziError):
            kz.write_bytes_bound(bits, bs)
