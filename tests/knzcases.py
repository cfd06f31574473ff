"""A deterministic case set for the .knz container's assemble / index pair (kz_knz_assemble / kz_knz_index on the host,
kz_knz_assemble_device / kz_knz_index_device on the GPU): synthetic block streams, random bits of chosen lengths with random
garbage behind the W bits of every row (the spare bits of the last byte and the bytes after it), so that anything a packer reads
beyond a stream shows in the result.  tests/test_knz_cases.py shows on the host that the set reaches the seams it is meant to."""
import numpy as np

BLOCK_SIZE = 1 << 20          # the header's block size: the container does not look inside the streams
GARBAGE = 24                  # garbage bytes behind every stream


class Case:
    def __init__(self, name, bits, seed, input_size=0, checksum=0):
        self.name, self.bits, self.input_size, self.checksum = name, [int(b) for b in bits], int(input_size), int(checksum)
        self.seed = seed

    def rows(self):
        """[row bytes]: (W + 7) // 8 bytes of random bits (spare bits random too) + GARBAGE random bytes; empty rows for W == 0"""
        rng = np.random.default_rng(0x6B6E7A00 + self.seed)
        return [rng.integers(0, 256, (w + 7) // 8 + GARBAGE, dtype=np.uint8) if w > 0 else rng.integers(0, 256, GARBAGE, dtype=np.uint8)
                for w in self.bits]

    def layout(self, lead=0, odd=False):
        """-> (buffer, offset of row 0, stride): the rows `stride` apart behind `lead` bytes, stride odd on request; the gaps zero"""
        rows = self.rows()
        stride = max([len(r) for r in rows] + [8])
        if odd and stride % 2 == 0:
            stride += 1
        buf = np.zeros(lead + max(len(rows), 1) * stride, dtype=np.uint8)
        for i, r in enumerate(rows):
            buf[lead + i * stride:lead + i * stride + len(r)] = r
        return buf, lead, stride

    def capacity(self):
        return 26 + sum((w + 7) // 8 + 8 for w in self.bits) + 8


def _euler_phases():
    """64 values of W mod 8 such that, with a 15-bit prefix in front of every block (lw = 10) and the first prefix on a byte
    boundary, the pairs (bit phase of the payload's start, W mod 8) are all 64 different: an Euler circuit of the graph
    phase -> (phase + w + 15) mod 8."""
    left = {p: list(range(8)) for p in range(8)}
    stack, path = [(7, None)], []                 # the first payload starts at phase (0 + 15) mod 8
    while stack:
        p, w = stack[-1]
        if left[p]:
            w2 = left[p].pop()
            stack.append(((p + w2 + 15) % 8, w2))
        else:
            stack.pop()
            if w is not None:
                path.append(w)
    return path[::-1]


def lw(w):
    return 3 if w < 8 else (w >> 3).bit_length() - 1 + 4


def cases():
    out = []
    # (a) 64 blocks: W through every residue mod 8 while the payload's start runs through every bit phase (lw = 10 throughout)
    ws = _euler_phases()
    out.append(Case("a-phases", [8 * (64 + (i * 37) % 64) + w for i, w in enumerate(ws)], 1))
    # (b) 4096 tiny streams of 24-72 bits: many blocks, prefixes and boundaries inside one lane's span
    rng = np.random.default_rng(0xB0B)
    out.append(Case("b-tiny", rng.integers(24, 73, 4096), 2))
    # (c) three streams of about 1 MiB with odd bit counts: span interiors, wide-store alignment
    out.append(Case("c-1MiB", [8 * (1 << 20) + 3, 8 * (1 << 20) - 5, 8 * ((1 << 20) + 4099) + 1], 3))
    # (d) W = 8 * 2^k - 1, 8 * 2^k, 8 * 2^k + 1: every lw, both sides of each step
    out.append(Case("d-lw", [8 * (1 << k) + d for k in range(21) for d in (-1, 0, 1)], 4))
    # (e) bits[i] == 0 between others; no blocks at all
    out.append(Case("e-zeros", [0, 77, 0, 0, 1234, 9, 0, 8191, 0], 5))
    out.append(Case("e-none", [], 6))
    out.append(Case("e-only-zeros", [0, 0, 0], 7))
    # (f) input sizes at the steps of the header's size field (size mask 0 .. 3: headers of 20 to 26 bytes) x checksum kinds
    sizes = [0, 65535, 65536, 1 << 30, (1 << 30) + 16, (1 << 32) - 1, 1 << 32, (1 << 48) - 1, 1 << 48]
    for i, sz in enumerate(sizes):
        for chk in (0, 32, 64):
            out.append(Case("f-size%d-chk%d" % (i, chk), [100 + 13 * i + chk, 57], 100 + 3 * i + chk // 32, input_size=sz, checksum=chk))
    return out


def assemble_host(L, case, transform=0, entropy=0):
    """kz_knz_assemble (host, no GPU) of a case -> bytes"""
    buf, lead, stride = case.layout()
    b = np.ascontiguousarray(case.bits, dtype=np.int64)
    cap = case.capacity()
    dst = np.full(cap, 0xA5, dtype=np.uint8)
    rc = L.kz_knz_assemble(transform, entropy, BLOCK_SIZE, case.input_size, case.checksum, buf.ctypes.data + lead, stride,
                           b.ctypes.data if len(b) else None, len(b), dst.ctypes.data, cap)
    assert rc > 0, (case.name, rc)
    return dst[:rc].tobytes()
