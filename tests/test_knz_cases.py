"""The case set of tests/knzcases.py reaches the seams of the container's bit layout.  No GPU: the host kz_knz_assemble /
kz_knz_index place the blocks, and the layout they report is looked at.  If the set is thinned, these fail."""
import numpy as np
import pytest

import kanzi_amd as kz
import knzcases


@pytest.fixture(scope="module")
def laid(built):
    L = kz.load_library()
    out = {}
    for c in knzcases.cases():
        knz = knzcases.assemble_host(L, c)
        out[c.name] = (c, knz, kz.knz_index(knz))
    return out


def _fields(idx, header_bits):
    """[(prefix start, payload start, W)] of an indexed stream"""
    out, pos = [], header_bits
    for off, w in idx["blocks"]:
        out.append((pos, off, w))
        pos = off + w
    return out


def _header_bits(knz, idx):
    blocks = idx["blocks"]
    if not blocks:
        return len(knz) * 8 - 8
    off, w = blocks[0]
    return off - 5 - knzcases.lw(w)


def test_index_returns_the_cases_lengths(laid):
    for c, knz, idx in laid.values():
        assert [w for _, w in idx["blocks"]] == [b for b in c.bits if b > 0], c.name
        assert idx["inputSize"] == (c.input_size if 0 < c.input_size < (1 << 48) else 0) and idx["checksum"] == c.checksum, c.name
        rows = c.rows()
        live = [r for r, b in zip(rows, c.bits) if b > 0]
        for (off, w), r in list(zip(idx["blocks"], live))[:80]:
            want = bytearray(r[:(w + 7) // 8].tobytes())
            if w % 8:
                want[-1] &= (0xFF << (8 - w % 8)) & 0xFF
            assert kz.extract_bits(knz, off, w) == bytes(want), c.name
        hb = _header_bits(knz, idx)
        assert hb % 8 == 0
        end = idx["blocks"][-1][0] + idx["blocks"][-1][1] if idx["blocks"] else hb
        assert len(knz) == (end + 8 + 7) // 8                                # end marker: 5 + 3 zero bits


def test_every_start_phase_meets_every_length_residue(laid):
    c, knz, idx = laid["a-phases"]
    assert len(idx["blocks"]) == 64
    assert {(off % 8, w % 8) for off, w in idx["blocks"]} == {(p, r) for p in range(8) for r in range(8)}


def test_every_prefix_width(laid):
    seen = set()
    for c, knz, idx in laid.values():
        for pre, off, w in _fields(idx, _header_bits(knz, idx)):
            assert off - pre - 5 == knzcases.lw(w)
            seen.add(off - pre - 5)
    need = knzcases.lw(8 * (1 << 20))                                        # what a 1 MiB stream needs
    assert need == 24 and seen >= set(range(3, need + 1))
    # both sides of every step, and the step itself
    c, knz, idx = laid["d-lw"]
    ws = [w for _, w in idx["blocks"]]
    for k in range(21):
        assert {8 * (1 << k) - 1, 8 * (1 << k), 8 * (1 << k) + 1} <= set(ws)
        assert knzcases.lw(8 * (1 << k) - 1) == k + 3 and knzcases.lw(8 * (1 << k)) == k + 4


def test_block_boundaries_at_every_byte_position_of_a_wide_store(laid):
    c, knz, idx = laid["b-tiny"]
    assert len(idx["blocks"]) == 4096 and min(c.bits) == 24 and max(c.bits) == 72
    at = {(pre // 8) % 16 for pre, _, _ in _fields(idx, _header_bits(knz, idx))}
    assert at == set(range(16))
    # several whole blocks inside one 16-byte span
    starts = [pre // 128 for pre, _, _ in _fields(idx, _header_bits(knz, idx))]
    assert max(np.bincount(np.array(starts) - starts[0])) >= 3


def test_a_byte_shared_by_three_fields(laid):
    """the end of a payload, a whole 5-bit field and the start of the length field behind it in one destination byte"""
    n = 0
    for name in ("a-phases", "b-tiny"):
        c, knz, idx = laid[name]
        for pre, off, w in _fields(idx, _header_bits(knz, idx))[1:]:
            if pre % 8 in (1, 2):
                n += 1
    assert n >= 8


def test_one_mebibyte_streams_with_odd_bit_counts(laid):
    c, knz, idx = laid["c-1MiB"]
    assert len(idx["blocks"]) == 3 and all(w % 8 for _, w in idx["blocks"]) and all(w > 8 * 1000 * 1000 for _, w in idx["blocks"])
    assert len({off % 8 for off, _ in idx["blocks"]}) >= 2


def test_header_lengths(laid):
    lens = {}
    for name, (c, knz, idx) in laid.items():
        if name.startswith("f-"):
            lens.setdefault(_header_bits(knz, idx) // 8, set()).add(c.checksum)
    assert sorted(lens) == [20, 22, 24, 26] and all(v == {0, 32, 64} for v in lens.values())
    assert len([n for n in laid if n.startswith("f-")]) == 27


def test_empty_entries_and_empty_stream(laid):
    c, knz, idx = laid["e-zeros"]
    assert c.bits.count(0) == 5 and c.bits[0] == 0 and c.bits[-1] == 0 and len(idx["blocks"]) == 4
    for name in ("e-none", "e-only-zeros"):
        c, knz, idx = laid[name]
        assert idx["blocks"] == [] and len(knz) == 21 and knz[-1] == 0
