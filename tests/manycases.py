"""The case set of the many-stream calls (kz_compress_many_device / kz_decompress_many_device): stream lengths around the block
size, segments packed into one source buffer at every residue mod 16, slots at odd offsets with poison between them, and the
damaged streams that are built from one small good stream.  No GPU and no randomness beyond datagen's seeded blocks;
tests/test_many_cases.py shows that the set reaches the seams, tests/test_gpu_knz_many.py runs it."""
import numpy as np

import datagen
import knzcases
import refinputs
import textgen

BLOCK_SIZES = [1024, 65536]
GAPS = (0, 1, 37)                 # bytes between one source segment and the next, in turn
SLOT_GAPS = (0, 2, 38)            # bytes between one slot and the next: even, so that every slot starts at an odd offset
LEAD = 5                          # the first segment's offset in the source buffer
SLOT_LEAD = 3                     # the first slot's offset in the destination
CHAINS = [("NONE", "NONE"), ("LZ", "HUFFMAN"), ("BWT+RANK+ZRLT", "ANS0"), ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0")]


def lengths(bs):
    return [0, 1, 15, 16, bs - 1, bs, bs + 1, 3 * bs, 3 * bs + 15, 40 * bs + 777]


def call_lengths(bs):
    """the streams of one call: every length of the set three times, the second time in reverse order (most lengths are 0, 1 or 15
    mod 16 and the gaps 0, 1 and 5: it takes thirty segments to reach every residue mod 16)"""
    return lengths(bs) + lengths(bs)[::-1] + lengths(bs)


_DATA = {}


def data_for(chain, bs):
    """41 blocks, block classes mixed so that the block streams differ in length (text in every other block for TEXT)"""
    key = ("text" if "TEXT" in chain else "bin", bs)
    if key not in _DATA:
        n = 40 * bs + 777
        parts = []
        text = np.frombuffer(textgen.english(3 * bs, 7), dtype=np.uint8) if key[0] == "text" else None
        for b in range(41):
            if key[0] == "text" and b % 2 == 0:
                at = (b * 7919) % (2 * bs)
                parts.append(text[at:at + bs])
            else:
                parts.append(datagen.block(b, bs))
        _DATA[key] = np.ascontiguousarray(np.concatenate(parts)[:n])
    return _DATA[key]


def buffers(chain, bs):
    """the input buffers of one call, one per entry of call_lengths: stream i is a window of data_for that starts i blocks in"""
    d = data_for(chain, bs)
    out = []
    for i, n in enumerate(call_lengths(bs)):
        at = (i * bs) % max(len(d) - n, 1) if n < len(d) else 0
        out.append(np.ascontiguousarray(d[at:at + n]))
    return out


def plan_gaps(lens, lead=LEAD, gaps=GAPS):
    """the gap behind each segment: of the three, in turn from i % 3, the first that puts the next segment on a residue mod 16
    no segment had yet (the turn's own gap when none does)"""
    seen, at, out = set(), lead, []
    for i, n in enumerate(lens):
        seen.add(at % 16)
        order = [gaps[(i + k) % len(gaps)] for k in range(len(gaps))]
        g = next((g for g in order if (at + n + g) % 16 not in seen), order[0])
        out.append(g)
        at += n + g
    return out


def pack(chunks, lead=LEAD, gaps=None, fill=0xA5, tail=64):
    """chunks back to back in one buffer: the first at `lead`, gaps[i] bytes of `fill` behind chunk i (plan_gaps by default),
    `tail` bytes of `fill` behind the last -> (buffer, offsets)"""
    if gaps is None:
        gaps = plan_gaps([len(c) for c in chunks], lead)
    offs, at = [], lead
    for i, c in enumerate(chunks):
        offs.append(at)
        at += len(c) + gaps[i % len(gaps)]
    buf = np.full(at + tail, fill, dtype=np.uint8)
    for o, c in zip(offs, chunks):
        buf[o:o + len(c)] = np.frombuffer(bytes(c), dtype=np.uint8) if not isinstance(c, np.ndarray) else c
    return buf, offs


def slots(caps, lead=SLOT_LEAD, gaps=SLOT_GAPS):
    """slot offsets for the capacities `caps`: odd offsets when the capacities are even -> (offsets, payload bytes)"""
    offs, at = [], lead
    for i, c in enumerate(caps):
        offs.append(at)
        at += int(c) + gaps[i % len(gaps)]
    return offs, at


def outside_slots(total, offs, caps):
    """mask over [0, total): True for the bytes that belong to no slot"""
    m = np.ones(total, dtype=bool)
    for o, c in zip(offs, caps):
        m[o:o + int(c)] = False
    return m


# ---- damaged streams, all from one small good stream --------------------------------------------------------------------------
SMALL_BS = 1024
SMALL_CHAIN = ("BWT+RANK+ZRLT", "ANS0")


def small_input():
    """three compressible 1 KiB blocks: a stream of well under 200 bytes"""
    return np.frombuffer(b"ab" * 512 + b"cdc" * 341 + b"c" + b"efgh" * 256, dtype=np.uint8)


def truncations(knz):
    return [("cut %d" % cut, bytes(knz[:cut])) for cut in range(len(knz))]


def header_faults(knz):
    return [(what, bad) for what, bad, _ in refinputs.header_faults(knz)]


def prefix_faults(knz, blocks):
    """tests/test_gpu_knz_device.py::test_length_prefix_faults' edits: bit flips in the three blocks' prefixes, a 34-bit length, no
    end marker.  blocks: [(bit offset, W)] as knz_index returns them"""
    out = []
    for k in (0, 1, 2):
        off, w = blocks[k]
        pre = off - 5 - knzcases.lw(w)
        for bit in [pre + i for i in range(5)] + [pre + 5, pre + 5 + knzcases.lw(w) // 2, off - 1]:
            bad = bytearray(knz)
            bad[bit >> 3] ^= 0x80 >> (bit & 7)
            out.append(("block %d bit %d" % (k, bit - pre), bytes(bad)))
        bad = bytearray(knz)
        refinputs.set_bits(bad, pre, 5, 31)
        out.append(("block %d lw 34" % k, bytes(bad)))
    out.append(("no end marker", bytes(knz[:-1])))
    return out


def block_header_fault(knz, blocks, k=1, byte=0):
    """a flipped bit in byte `byte` of block k's header (k = 1: block 2 of 3)"""
    off, _ = blocks[k]
    bad = bytearray(knz)
    bit = off + 8 * byte + 3
    bad[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(bad)


def interleave(bad, good):
    """good, bad[0], good, bad[1], ..., good -> (streams, indices of the good ones)"""
    streams, goods = [], []
    for _, b in bad:
        goods.append(len(streams))
        streams.append(good)
        streams.append(b)
    goods.append(len(streams))
    streams.append(good)
    return streams, goods


# ---- the grouping both calls use, restated (kz_stream_device.hip) ----------------------------------------------------------------------
def writer_groups(lens, bs, chunk):
    """kz_compress_many_device: consecutive streams with at most `chunk` blocks together (an empty stream counts as one); a
    stream with more blocks goes alone through the single-stream call -> [("group", [i ...]) | ("single", [i])]"""
    nb = [(n + bs - 1) // bs for n in lens]
    out, i = [], 0
    while i < len(lens):
        if nb[i] > chunk:
            out.append(("single", [i]))
            i += 1
            continue
        g, tot = [], 0
        while i < len(lens) and nb[i] <= chunk and (not g or tot + max(nb[i], 1) <= chunk):
            tot += max(nb[i], 1)
            g.append(i)
            i += 1
        out.append(("group", g))
    return out
