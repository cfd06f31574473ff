"""The case set of the many-stream calls (tests/manycases.py) reaches the seams the kernels have: shown on the host, with the
oracle's streams and the host container helpers.  No GPU."""
import numpy as np

import kanzi_amd as kz
import manycases as mc
import oracle

BS = 1024
CHAINS = [("BWT+RANK+ZRLT", "ANS0"), ("LZ", "HUFFMAN")]
_STREAMS = {}


def streams(chain, ent):
    """the oracle's .knz stream of every buffer of the set at 1 KiB blocks, with its index"""
    if (chain, ent) not in _STREAMS:
        out = []
        for b in mc.buffers(chain, BS):
            s = oracle.compress(chain, ent, BS, b)
            out.append((s, kz.knz_index(s)))
        _STREAMS[(chain, ent)] = out
    return _STREAMS[(chain, ent)]


def test_lengths_and_source_layout():
    for bs in mc.BLOCK_SIZES:
        assert mc.lengths(bs) == [0, 1, 15, 16, bs - 1, bs, bs + 1, 3 * bs, 3 * bs + 15, 40 * bs + 777]
        bufs = mc.buffers("NONE", bs)
        assert [len(b) for b in bufs] == mc.call_lengths(bs) and set(mc.lengths(bs)) == set(mc.call_lengths(bs))
        buf, offs = mc.pack(bufs)
        assert {o % 16 for o in offs} == set(range(16)), sorted({o % 16 for o in offs})
        gaps = [offs[i + 1] - offs[i] - len(bufs[i]) for i in range(len(bufs) - 1)]
        assert set(gaps) == set(mc.GAPS), gaps
        for o, b in zip(offs, bufs):
            assert buf[o:o + len(b)].tobytes() == b.tobytes()
        m = mc.outside_slots(len(buf), offs, [len(b) for b in bufs])
        assert bool((buf[m] == 0xA5).all()) and int(m.sum()) == len(buf) - sum(len(b) for b in bufs)
        # segments shorter than one 16-byte unit, and segments that share a unit of the source with a neighbour
        assert any(0 < len(b) < 16 for b in bufs)
        assert any(len(bufs[i]) and len(bufs[i + 1]) and (offs[i] + len(bufs[i]) - 1) // 16 == offs[i + 1] // 16 for i in range(len(bufs) - 1))


def test_slots_are_odd_and_share_units():
    for bs in mc.BLOCK_SIZES:
        lens = mc.call_lengths(bs)
        for caps in ([kz.compress_bound(n, bs) for n in lens], [n & ~1 for n in lens]):
            offs, total = mc.slots(caps)
            assert all(o % 2 == 1 for o in offs) and total >= offs[-1] + caps[-1]
            assert all(offs[i] + caps[i] <= offs[i + 1] for i in range(len(caps) - 1))          # no overlap
            gaps = {offs[i + 1] - offs[i] - caps[i] for i in range(len(caps) - 1)}
            assert gaps == set(mc.SLOT_GAPS)
            # two slots in one 16-byte aligned unit of the destination (the frame's payload starts on such a unit)
            assert any(caps[i] and caps[i + 1] and (offs[i] + caps[i] - 1) // 16 == offs[i + 1] // 16 for i in range(len(caps) - 1))
    # the exact decoded sizes as capacities: slots of 1 and 15 bytes lie inside one unit with their neighbours
    lens = mc.call_lengths(1024)
    offs, _ = mc.slots(lens)
    assert any(0 < lens[i] < 16 and offs[i] // 16 == (offs[i] + lens[i] - 1) // 16 for i in range(len(lens)))


def test_streams_end_at_every_bit_phase():
    phases, straddle, short_units = set(), 0, 0
    for chain, ent in CHAINS:
        ss = streams(chain, ent)
        caps = [kz.compress_bound(len(b), BS) for b in mc.buffers(chain, BS)]
        offs, _ = mc.slots(caps)
        for (s, idx), slot in zip(ss, offs):
            blocks = idx["blocks"]
            if not blocks:
                assert len(s) == 21                                            # header and end marker: longer than one unit
                continue
            off, w = blocks[-1]
            phases.add((off + w) % 8)
            assert (off + w + 8 + 7) // 8 == len(s)                             # the end marker behind the last block, then padding
            for off, w in blocks:                                              # a prefix whose bits lie in two 16-byte units of the slot
                pre = off - 5 - _lw(w)
                if (slot * 8 + pre) // 128 != (slot * 8 + off - 1) // 128:
                    straddle += 1
    assert phases == set(range(8)), sorted(phases)
    assert straddle >= 3, straddle


def _lw(w):
    return 3 if w < 8 else (w >> 3).bit_length() + 3


def test_damaged_streams_cover_the_walks_stop_reasons():
    data = mc.small_input()
    knz = oracle.compress(mc.SMALL_CHAIN[0], mc.SMALL_CHAIN[1], mc.SMALL_BS, data)
    idx = kz.knz_index(knz)
    assert len(idx["blocks"]) == 3 and len(knz) < 200
    cuts = mc.truncations(knz)
    assert [len(b) for _, b in cuts] == list(range(len(knz)))
    assert sum(1 for _, b in cuts if len(b) < 16) == 16                         # streams shorter than one 16-byte unit
    heads = mc.header_faults(knz)
    assert len(heads) == 11 and all(len(b) == len(knz) and b != knz for _, b in heads)
    pre = mc.prefix_faults(knz, idx["blocks"])
    assert len(pre) == 3 * 9 + 1 and all(b != knz for _, b in pre)
    # what the host walk says about them: good prefixes, a prefix or a payload past the end, and an early end marker all occur
    verdicts = set()
    for _, b in cuts[21:] + pre:
        src = np.frombuffer(b + b"\0" * 16, dtype=np.uint8)
        verdicts.add(min(kz.load_library().kz_knz_index(src.ctypes.data, len(b), None, None, None, None, None, None, None, 0), 0) or "ok")
    assert verdicts >= {"ok", -11}, verdicts                                   # (-11: ERR_READ_FILE)
    bad = mc.block_header_fault(knz, idx["blocks"], 1, 0)
    assert bad != knz and kz.knz_index(bad)["blocks"] == idx["blocks"]           # the container is whole: the fault is the block's
    streams_, goods = mc.interleave(pre, knz)
    assert len(streams_) == 2 * len(pre) + 1 and goods == list(range(0, len(streams_), 2)) and all(streams_[i] == knz for i in goods)


def test_groups_split_between_streams_at_chunks_of_three():
    lens = mc.call_lengths(BS)
    plan = mc.writer_groups(lens, BS, 3)
    assert sorted(i for _, g in plan for i in g) == list(range(len(lens)))
    singles = [g[0] for k, g in plan if k == "single"]
    assert singles and all((lens[i] + BS - 1) // BS > 3 for i in singles)       # streams larger than a group: 4 and 41 blocks
    assert {lens[i] for i in singles} == {3 * BS + 15, 40 * BS + 777}
    groups = [g for k, g in plan if k == "group"]
    assert sum(1 for g in groups if len(g) > 1) >= 2                            # groups of several streams ...
    for g in groups:
        assert sum(max((lens[i] + BS - 1) // BS, 1) for i in g) <= 3
    # ... that are full before the next stream begins: a group ends between two streams, never inside one
    assert any(k0 == "group" and k1 == "group" for (k0, _), (k1, _) in zip(plan, plan[1:]))
    # the default chunk (2 048 blocks at 1 KiB) takes the whole set in one group
    assert mc.writer_groups(lens, BS, 2048) == [("group", list(range(len(lens))))]
