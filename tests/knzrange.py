"""Case set and helpers for the seekable .knz calls (kz_decompress_range / kz_decompress_range_device, kz_decode_indexed /
kz_decode_indexed_device): the streams, the block ranges read from them, the damage done to them, the re-assembled stream that
says what a range read must give, and a Python model of the check every entry of a caller's index gets (k_knz_check).  Nothing here
touches the GPU: a stream is built by whatever compressor the caller hands in (the oracle in tests/test_knz_range_cases.py, the
library in tests/test_gpu_knz_range.py; the two write the same bytes)."""
import numpy as np

import kanzi_amd as kz
import datagen
import knzcases
import textgen

CHUNK = 3                     # KZ_STREAM_CHUNK of the seam cases: walks and decodes go in steps of three blocks
BWT = "BWT+RANK+ZRLT"


class Stream:
    """n bytes cut into blocks of bs, or (lens) blocks of the given lengths assembled into a stream with short middle blocks"""

    def __init__(self, name, chain, ent, bs, n=None, checksum=0, lens=None):
        self.name, self.chain, self.ent, self.bs, self.checksum, self.lens = name, chain, ent, bs, checksum, lens
        self.n = sum(lens) if lens else n

    def nblocks(self):
        return len(self.lens) if self.lens else (self.n + self.bs - 1) // self.bs

    def block_lengths(self):
        return list(self.lens) if self.lens else [min(self.bs, self.n - i * self.bs) for i in range(self.nblocks())]

    def block_data(self):
        """[block bytes]: block classes mixed so that the block streams differ in length; English text in every other block of a
        TEXT chain"""
        bs, out = self.bs, []
        text = np.frombuffer(textgen.english(3 * bs, 7), dtype=np.uint8) if "TEXT" in self.chain else None
        for b, l in enumerate(self.block_lengths()):
            if text is not None and b % 2 == 0:
                at = (b * 7919) % (2 * bs)
                out.append(text[at:at + bs][:l])
            else:
                out.append(datagen.block(b, bs)[:l])
        return out

    def original(self):
        return b"".join(b.tobytes() for b in self.block_data())

    def build(self, compress, encode_block=None):
        """compress(chain, ent, bs, data, checksum) -> .knz bytes; encode_block(chain, ent, bs, block, checksum) -> (stream, W)"""
        if not self.lens:
            return compress(self.chain, self.ent, self.bs, np.frombuffer(self.original(), dtype=np.uint8), self.checksum)
        coded = [encode_block(self.chain, self.ent, self.bs, b, self.checksum) for b in self.block_data()]
        return kz.knz_assemble(self.chain, self.ent, self.bs, self.n, [s for s, _ in coded], [w for _, w in coded], checksum=self.checksum)


def streams():
    return [Stream("none-1k-last1", "NONE", "NONE", 1024, 9 * 1024 + 1),
            Stream("bwt-1k-x32", BWT, "ANS0", 1024, 10 * 1024 + 333, checksum=32),
            Stream("lz-4k-x64", "LZ", "HUFFMAN", 4096, 8 * 4096, checksum=64),
            Stream("text-4k-last1", "TEXT+UTF+" + BWT, "ANS0", 4096, 9 * 4096 + 1),
            Stream("cm-1k", "LZP+BWT", "CM", 1024, 8 * 1024 + 100),
            Stream("bwt-64k", BWT, "ANS0", 65536, 8 * 65536 + 9),
            Stream("short-middle", BWT, "ANS0", 1024, lens=[1024, 100, 1024, 17, 1023, 1024, 1024, 5])]


def ranges(nb):
    """[(name, first block, count)] for a stream of nb blocks"""
    out = [("none", 0, 0), ("all", 0, nb), ("first", 0, 1), ("last", nb - 1, 1), ("last+4", nb - 1, 5), ("behind", nb, 3),
           ("far-behind", nb + 7, 1)]
    out += [("one-%d" % f, f, 1) for f in range(nb)]
    # with KZ_STREAM_CHUNK = CHUNK: a range whose first block lies in the second chunk of the skipping walk, one that lies across the
    # walk's first seam, and one that is decoded in two chunks
    out += [("second-chunk", CHUNK + 1, 2), ("across-walk-seam", CHUNK - 1, 3), ("two-decode-chunks", 1, CHUNK + 2)]
    return out


def header_bits(knz):
    """bit length of the stream header: 160 + 16 per 16 bits of the size field (CompressedOutputStream.java:236-313)"""
    v = int.from_bytes(knz[:20], "big")
    return 160 + 16 * ((v >> (160 - 121)) & 3)


def fields(knz, idx):
    """[(prefix start, payload start, W)] of an indexed stream"""
    out, pos = [], header_bits(knz)
    for off, w in idx["blocks"]:
        out.append((pos, off, w))
        pos = off + w
    return out


def reassemble(knz, idx, first, count):
    """the blocks [first, first + count) of knz (idx: its index, or the index of the undamaged stream it was made from) behind knz's
    own header parameters: kz_decompress of this stream is what a range read of knz must give"""
    blocks = idx["blocks"][first:first + count] if count > 0 else []
    return kz.knz_assemble(idx["transform"], idx["entropy"], idx["blockSize"], idx["inputSize"], [kz.extract_bits(knz, off, w) for off, w in blocks],
                           [w for _, w in blocks], checksum=idx["checksum"])


def _flip_bit(knz, bit):
    bad = bytearray(knz)
    bad[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(bad)


PAYLOAD_MIN_BITS = 8 * 40     # a block whose payload is damaged is at least this long: the middle lies behind header and checksum


def damaged(knz, idx, first, count):
    """[(kind, damaged stream, truth)] for the range [first, first + count), 0 < first, first + count < blocks.
    truth: "slice" = success and the undamaged range; "reassembled" = whatever kz_decompress says of reassemble(damaged stream);
    "whole" = the code kz_decompress gives for the damaged stream, nothing delivered; ("cut", nbytes) = whatever kz_decompress says
    of the undamaged range's re-assembled stream cut to nbytes"""
    nb = len(idx["blocks"])
    assert 0 < first and count > 0 and first + count < nb

    def mid(k):
        off, w = idx["blocks"][k]
        assert w >= PAYLOAD_MIN_BITS, (k, w)
        return off + w // 2

    f = fields(knz, idx)
    out = [("payload-front", _flip_bit(knz, mid(first - 1)), "slice"),
           ("payload-inside", _flip_bit(knz, mid(first + count // 2)), "reassembled"),
           ("payload-behind", _flip_bit(knz, mid(first + count)), "slice"),
           ("header-front", _flip_bit(knz, idx["blocks"][first - 1][0] + 3), "whole"),                 # the mode byte of the block header
           ("prefix-front", _flip_bit(knz, idx["blocks"][0][0] - 1), "whole")]                         # the last bit of block 0's length
    # truncation in the middle of the payload of the range's last block: its prefix and header are whole, its bits run out.  The
    # re-assembled stream is cut at the byte that holds the same bit of the same block (the cuts differ by less than a byte).
    cut = mid(first + count - 1) >> 3
    rel = 8 * cut - f[first][0]
    out.append(("truncated-inside", knz[:cut], ("cut", (header_bits(knz) + rel) >> 3)))
    return out


# ---- the check of an untrusted index entry (k_knz_check, kz_knz_gpu.hip) ----
def _bits(knz, at, k):
    return int.from_bytes(kz.extract_bits(knz, at, k), "big") >> ((-k) % 8)


def check_entry(knz, off, w):
    """W > 0; off at least 8 bits behind the stream header; off + W inside the stream; and an lr in 3 .. 34 whose 5 + lr bits in front
    of off lie behind the stream header and read (lr - 3, W): the walk could have produced (off, W) at this place"""
    hb, nbits = header_bits(knz), 8 * len(knz)
    if w <= 0 or off < hb + 8 or off + w > nbits:
        return False
    for lr in range(max(3, w.bit_length()), 35):
        at = off - 5 - lr
        if at < hb:
            break
        if _bits(knz, at, 5) + 3 == lr and _bits(knz, at + 5, lr) == w:
            return True
    return False


def index_mutants(knz, idx):
    """[(name, position of the bad entry, offsets, lengths)]: a true index with one entry made wrong"""
    blocks = idx["blocks"]
    nb, nbits = len(blocks), 8 * len(knz)
    out = []

    def mutant(name, i, off, w):
        offs, ws = [o for o, _ in blocks], [x for _, x in blocks]
        offs[i], ws[i] = off, w
        out.append((name, i, offs, ws))

    for name, i, d_off, d_w in (("off+1", 0, 1, 0), ("off-1", nb // 2, -1, 0), ("off+8", nb - 1, 8, -8), ("w+1", 1, 0, 1), ("w-1", nb - 2, 0, -1)):
        mutant(name, i, blocks[i][0] + d_off, blocks[i][1] + d_w)
    mutant("off-in-header", 2, 100, blocks[2][1])
    mutant("off-at-header-end", 0, header_bits(knz), blocks[0][1])
    mutant("end-past-stream", nb - 1, blocks[nb - 1][0], nbits - blocks[nb - 1][0] + 1)
    mutant("off-past-stream", 3, nbits + 64, blocks[3][1])
    mutant("w-zero", 1, blocks[1][0], 0)
    mutant("w-negative", 1, blocks[1][0], -blocks[1][1])
    mutant("off-negative", 0, -blocks[0][0], blocks[0][1])
    mutant("w-2^40", 0, blocks[0][0], 1 << 40)
    return out


def synthetic(nb=10, seed=5, bs=1024):
    """a stream of nb blocks of random bits (knzcases' kind: the container does not look inside them), for the checks that need no
    real block streams"""
    rng = np.random.default_rng(seed)
    ws = [int(w) for w in rng.integers(8 * 60, 8 * 700, nb)]
    rows = [rng.integers(0, 256, (w + 7) // 8, dtype=np.uint8).tobytes() for w in ws]
    return kz.knz_assemble("NONE", "NONE", bs, nb * bs, rows, ws)


lw = knzcases.lw
