"""The byte-addressed reads without a GPU: the two entry points are exported and bound, and the case set of tests/knzread.py is
worth running -- under the kernel's unit enumeration (model B) every delivered byte has exactly one writer and no other byte has
any, every class of unit occurs, and with KZ_STREAM_CHUNK = 3 ranges lie across chunk seams."""
import ctypes

import numpy as np

import kanzi_amd as kz
import knzrange
import knzread

STREAMS = {s.name: s for s in knzrange.streams()}


def _cases():
    """[(name, block starts, block size, ranges)]: every stream's case set, and the batch"""
    out = []
    for s in STREAMS.values():
        lens = s.block_lengths()
        out.append((s.name, knzread.starts(lens), s.bs, knzread.ranges(lens)))
    s = STREAMS[knzread.BATCH_STREAM]
    out.append(("batch", knzread.starts(s.block_lengths()), s.bs, knzread.batch(s.block_lengths())))
    return out


def test_the_names_are_exported_and_bound(built):
    L = ctypes.CDLL(kz.LIB_PATH)
    for name in ("kz_read_bytes", "kz_read_bytes_device"):
        assert hasattr(L, name) and name in kz.ABI_SYMBOLS, name
        assert getattr(kz.load_library(), name).restype is ctypes.c_int64
    for name in ("read_bytes", "read_bytes_device", "block_byte_offsets"):
        assert callable(getattr(kz, name)), name
    assert callable(kz.KnzReader.read_many)
    assert kz.load_library().kz_abi_version() == 3
    names = [kz.load_library().kz_get_kernel_name(i).decode() for i in range(kz.load_library().kz_get_kernel_count())]
    assert "k_knz_read" in names and "k_knz_scatter" in names


def test_every_delivered_byte_has_one_writer_at_every_base_phase():
    for name, B, bs, rngs in _cases():
        _, segs = knzread.segments(B, rngs)
        total = sum(s for _, s in rngs)
        owned = bytearray(total)                                                         # 1: a byte some range is delivered into
        for g in segs:
            assert sum(owned[g["dst"]:g["dst"] + g["len"]]) == 0, (name, "two segments own a byte")
            owned[g["dst"]:g["dst"] + g["len"]] = b"\1" * g["len"]
        # the segments tile every delivered range: model A's lengths
        at = 0
        for (o, s), r in zip(rngs, range(len(rngs))):
            got = max(min(o + s, B[-1]) - o, 0)
            mine = [g for g in segs if g["range"] == r]
            assert sum(g["len"] for g in mine) == got and all(g["len"] > 0 for g in mine), (name, r)
            assert [g["dst"] for g in mine] == [at + sum(x["len"] for x in mine[:i]) for i in range(len(mine))], (name, r)
            assert bytes(owned[at + got:at + s]) == b"\0" * (s - got), (name, r, "the tail of a cut slot")
            at += s
        for base in range(16):
            writers = np.zeros(base + total + 16, dtype=np.uint8)
            units = knzread.model_b(segs, base, bs)
            for u in units:
                assert u["addr"] % 16 == 0 and u["addr"] <= u["lo"] < u["hi"] <= u["addr"] + 16
                writers[u["lo"]:u["hi"]] += 1
            assert writers[base:base + total].tobytes() == bytes(owned), (name, base, "one writer per delivered byte, none elsewhere")
            assert not writers[:base].any() and not writers[base + total:].any(), (name, base, "a byte outside dst")
            # unit0 is the prefix sum of the segments' unit counts: units come segment by segment
            assert [u["seg"] for u in units] == sorted(u["seg"] for u in units), (name, base)


def test_the_case_set_hits_every_class_of_unit():
    seen = set()
    for name, B, bs, rngs in _cases():
        _, segs = knzread.segments(B, rngs)
        for base in (0, 5):
            units = knzread.model_b(segs, base, bs)
            per_addr, per_seg = {}, {}
            for u in units:
                per_addr.setdefault(u["addr"], set()).add(u["seg"])
                per_seg.setdefault(u["seg"], []).append(u)
            for j, us in per_seg.items():
                g = segs[j]
                if any(u["kind"] == "wide" for u in us):
                    seen.add("wide")
                if len(us) > 1 and us[0]["hi"] - us[0]["lo"] < 16:
                    seen.add("bytewise head")
                if len(us) > 1 and us[-1]["hi"] - us[-1]["lo"] < 16:
                    seen.add("bytewise tail")
                if len(us) == 1 and g["len"] < 16:
                    seen.add("short segment inside one unit")
                if us[-1]["hi"] % 16 == 0:
                    seen.add("ends on a unit edge")
                # (rows are 16-byte aligned and a multiple of 16 long: the load window of a whole unit never leaves its row)
                assert all(u["kind"] == "wide" for u in us if u["hi"] - u["lo"] == 16), (name, j)
            for addr, js in per_addr.items():
                if len(js) == 2:
                    seen.add("two segments in one unit")
                if len(js) >= 3:
                    seen.add("three or more segments in one unit")
    assert seen == {"wide", "bytewise head", "bytewise tail", "short segment inside one unit", "ends on a unit edge",
                    "two segments in one unit", "three or more segments in one unit"}, seen


def test_ranges_lie_across_chunk_seams():
    """With chunks of three blocks a range of two blocks is finished by two launches, one of the whole stream by three or more; and
    a range that spans three chunks has, in the chunk in the middle, neither its first nor its last segment."""
    for name, B, bs, rngs in _cases():
        if name == "batch":
            continue
        blocks, segs = knzread.segments(B, rngs, knzread.CHUNK)
        assert blocks == list(range(len(B) - 1)), name                                   # the case set touches every block
        spans = {}
        for g in segs:
            spans.setdefault(g["range"], []).append(g["chunk"])
        assert any(len(set(c)) == 2 for c in spans.values()), name
        three = [r for r, c in spans.items() if len(set(c)) >= 3]
        assert three, name
        r = three[0]
        mine = [g for g in segs if g["range"] == r]
        mid = sorted(set(spans[r]))[1]
        assert all(g is not mine[0] and g is not mine[-1] for g in mine if g["chunk"] == mid), name
        # a chunk's segments stay in dst order, and some chunk holds segments of ranges that another chunk completes
        for c in set(g["chunk"] for g in segs):
            d = [g["dst"] for g in segs if g["chunk"] == c]
            assert d == sorted(d), (name, c)


def test_block_byte_offsets_agrees_with_short_middle():
    s = STREAMS["short-middle"]
    lens = s.block_lengths()
    # the stream is what a join of streams with these input sizes looks like: every block is a stream's last
    assert kz.block_byte_offsets(lens, s.bs) == knzread.starts(lens)
    assert kz.block_byte_offsets([1024 + 100, 1024 + 17, 1023, 2048, 5], s.bs) == knzread.starts(lens)
    assert kz.block_byte_offsets([], 1024) == [0] and kz.block_byte_offsets([0, 5, 0], 1024) == [0, 5]
    assert kz.block_byte_offsets([2048], 1024) == [0, 1024, 2048] and kz.block_byte_offsets([2049], 1024) == [0, 1024, 2048, 2049]


def test_model_a_is_plain_slicing():
    s = STREAMS["short-middle"]
    blocks = [b.tobytes() for b in s.block_data()]
    data, B = b"".join(blocks), knzread.starts(s.block_lengths())
    rngs = knzread.ranges(s.block_lengths())
    for (o, n), (got, b) in zip(rngs, knzread.model_a(blocks, s.bs, rngs, table=B)):
        assert got == len(data[o:o + n]) and b == data[o:o + n]
    # without the table the stream has byte addresses only where its blocks are whole
    out = knzread.model_a(blocks, s.bs, [(0, 1024), (0, 1025), (1024, 1), (2 * 1024 + 3, 9), (7 * 1024, 100), (7 * 1024 + 5, 1)], table=None)
    assert [g for g, _ in out] == [1024, knzread.INVALID_FILE, knzread.INVALID_FILE, 9, 5, 0]
    assert out[0][1] == blocks[0] and out[3][1] == blocks[2][3:12] and out[4][1] == blocks[7]
