"""CPU model of the reference's CM entropy coder (EntropyCodecFactory.CM_TYPE = 6), written from its Java:
  K/entropy/CMPredictor.java:100-124 (initial state), :136-160 (update), :172-186 (get, the bitstream version >= 4 branch),
  K/entropy/BinaryEntropyEncoder.java:117-155 (encode), :187-204 (encodeBit), :212-218 (flush), :250-255 (dispose),
  K/entropy/BinaryEntropyDecoder.java:117-167 (decode), :196-218 (decodeBit), :226-239 (read),
  K/entropy/EntropyUtils.java:259-300 (writeVarInt / readVarInt).
One coder and one fresh predictor per block (EntropyCodecFactory builds them per EncodingTask); the writer calls dispose() after every
block, so a block's bit string is  varint(szBytes) | szBytes payload bytes | (low | 0xFFFFFF) as 56 bits.  Blocks of 1 << 26 bytes and
more (the reference splits them into 8 or 16 chunks) are refused, as the device code refuses them.

encode / decode keep the reference's `while` loops and record what they saw in `stats` (reset by every call):
  pmin, pmax      smallest / largest prediction handed to the coder
  cmin, cmax      smallest / largest counter value, the initial ones included
  max_flushes     most passes of the flush / read loop behind one bit
  flush_at        encode: the byte index at which each 32-bit flush happened
  read_at         decode: the byte index at which each 32-bit read happened (overruns included)
  overruns        decode: the number of bits at which a read passed bufLimit
"""

TOP = 0x00FFFFFFFFFFFFFF
MASK_24_56 = 0x00FFFFFFFF000000
MASK_0_24 = 0x0000000000FFFFFF
MASK_0_32 = 0x00000000FFFFFFFF
MASK_0_56 = 0x00FFFFFFFFFFFFFF
PSCALE = 65536
FAST_RATE, MEDIUM_RATE, SLOW_RATE = 2, 4, 6
MAX_CHUNK_SIZE = 1 << 26

stats = {}


def _reset_stats():
    stats.clear()
    stats.update(pmin=4096, pmax=-1, cmin=0, cmax=65535, max_flushes=0, flush_at=[], read_at=[], overruns=0)


class Predictor:
    """CMPredictor, one call per bit as the coder makes them (the model's encode / decode below run the same statements inline)"""

    def __init__(self):
        self.c1 = self.c2 = 0
        self.ctx = 1
        self.idx = 0
        self.run_mask = 0
        self.counter1 = [[PSCALE >> 1] * 257 for _ in range(256)]
        self.counter2 = [[j << 12 for j in range(16)] + [65535] for _ in range(512)]

    def get(self):
        pc1 = self.counter1[self.ctx]
        p = (13 * (pc1[256] + pc1[self.c1]) + 6 * pc1[self.c2]) >> 5
        self.idx = p >> 12
        pc2 = self.counter2[self.ctx | self.run_mask]
        return (p + p + 3 * (pc2[self.idx] + pc2[self.idx + 1]) + 64) >> 7

    def update(self, bit):
        c1_ = self.counter1[self.ctx]
        c2_ = self.counter2[self.ctx | self.run_mask]
        i = self.idx
        if bit == 0:
            c1_[256] -= c1_[256] >> FAST_RATE
            c1_[self.c1] -= c1_[self.c1] >> MEDIUM_RATE
            c2_[i] -= c2_[i] >> SLOW_RATE
            c2_[i + 1] -= c2_[i + 1] >> SLOW_RATE
            self.ctx += self.ctx
        else:
            c1_[256] -= (c1_[256] - PSCALE + 16) >> FAST_RATE
            c1_[self.c1] -= (c1_[self.c1] - PSCALE + 16) >> MEDIUM_RATE
            c2_[i] -= (c2_[i] - PSCALE + 16) >> SLOW_RATE
            c2_[i + 1] -= (c2_[i + 1] - PSCALE + 16) >> SLOW_RATE
            self.ctx += self.ctx + 1
        if self.ctx > 255:
            self.c2 = self.c1
            self.c1 = self.ctx & 0xFF
            self.ctx = 1
            self.run_mask = 0x100 if self.c1 == self.c2 else 0


def varint(value):
    """EntropyUtils.writeVarInt"""
    out = bytearray()
    while value >= 128:
        out.append(0x80 | (value & 0x7F))
        value >>= 7
    out.append(value)
    return bytes(out)


def encode(data):
    """-> (bytes, nbits) of encode(block, 0, len(data)) followed by dispose()"""
    count = len(data)
    if count >= MAX_CHUNK_SIZE:
        raise ValueError("CM blocks go up to (1 << 26) - 1 bytes here")
    _reset_stats()
    low, high = 0, TOP
    if count == 0:                                             # encode() returns 0 at once, dispose() still writes the tail
        return (low | MASK_0_24).to_bytes(7, "big"), 56
    counter1 = [[PSCALE >> 1] * 257 for _ in range(256)]
    counter2 = [[j << 12 for j in range(16)] + [65535] for _ in range(512)]
    c1 = c2 = run_mask = 0
    sba = bytearray()
    pmin, pmax, cmin, cmax, max_flushes = 4096, -1, 0, 65535, 0
    flush_at = stats["flush_at"]
    for i in range(count):
        val = data[i]
        ctx = 1
        for sh in (7, 6, 5, 4, 3, 2, 1, 0):
            bit = (val >> sh) & 1
            # predictor.get()
            pc1 = counter1[ctx]
            a, b = pc1[256], pc1[c1]
            p = (13 * (a + b) + 6 * pc1[c2]) >> 5
            idx = p >> 12
            pc2 = counter2[ctx | run_mask]
            x1, x2 = pc2[idx], pc2[idx + 1]
            pred = (p + p + 3 * (x1 + x2) + 64) >> 7
            if pred < pmin:
                pmin = pred
            if pred > pmax:
                pmax = pred
            # encodeBit
            split = (((high - low) >> 4) * pred) >> 8
            if bit == 0:
                low += split + 1
                a -= a >> FAST_RATE
                b -= b >> MEDIUM_RATE
                x1 -= x1 >> SLOW_RATE
                x2 -= x2 >> SLOW_RATE
                ctx += ctx
                if b < cmin or a < cmin or x1 < cmin:
                    cmin = min(a, b, x1)
            else:
                high = low + split
                a -= (a - PSCALE + 16) >> FAST_RATE
                b -= (b - PSCALE + 16) >> MEDIUM_RATE
                x1 -= (x1 - PSCALE + 16) >> SLOW_RATE
                x2 -= (x2 - PSCALE + 16) >> SLOW_RATE
                ctx += ctx + 1
                if a > cmax or b > cmax or x2 > cmax:
                    cmax = max(a, b, x2)
            pc1[256] = a
            pc1[c1] = b
            pc2[idx] = x1
            pc2[idx + 1] = x2
            assert low <= high
            flushes = 0
            while ((low ^ high) & MASK_24_56) == 0:
                sba += ((high >> 24) & MASK_0_32).to_bytes(4, "big")
                low = (low << 32) & 0xFFFFFFFFFFFFFFFF
                high = ((high << 32) | MASK_0_32) & 0xFFFFFFFFFFFFFFFF
                flushes += 1
                flush_at.append(i)
            if flushes > max_flushes:
                max_flushes = flushes
        c2 = c1
        c1 = val
        run_mask = 0x100 if c1 == c2 else 0
    stats.update(pmin=pmin, pmax=pmax, cmin=cmin, cmax=cmax, max_flushes=max_flushes)
    out = varint(len(sba)) + bytes(sba) + ((low | MASK_0_24) & MASK_0_56).to_bytes(7, "big")
    return out, 8 * len(out)


def decode(bits, nbits, count):
    """-> (ok, bytes, bits consumed); ok False where the reference returns -1 or its bit stream throws"""
    if count >= MAX_CHUNK_SIZE:
        raise ValueError("CM blocks go up to (1 << 26) - 1 bytes here")
    _reset_stats()
    if count == 0:
        return True, b"", 0
    avail = nbits >> 3                                         # every read below is of whole bytes at a byte boundary
    pos = 0
    # EntropyUtils.readVarInt
    if pos >= avail:
        return False, b"", 0
    value = bits[pos]
    pos += 1
    sz = value & 0x7F
    shift = 7
    while value >= 128:
        if pos >= avail:
            return False, b"", 0
        value = bits[pos]
        pos += 1
        sz |= (value & 0x7F) << shift
        if shift == 28:
            break
        shift += 7
    sz &= 0xFFFFFFFF
    if sz >= 1 << 31:                                          # a negative int: readBits(array, 0, 8 * szBytes) throws
        return False, b"", 0
    if sz > min(count << 5, 0x7FFFFFFF >> 3):                  # BinaryEntropyDecoder.java:141-144
        return False, b"", 0
    if pos + 7 + sz > avail:                                   # readBits(56) or the payload read runs off the stream
        return False, b"", 0
    current = int.from_bytes(bits[pos:pos + 7], "big")
    pos += 7
    buf = bits[pos:pos + sz]
    pos += sz
    buf_limit = sz
    index = 0
    counter1 = [[PSCALE >> 1] * 257 for _ in range(256)]
    counter2 = [[j << 12 for j in range(16)] + [65535] for _ in range(512)]
    c1 = c2 = run_mask = 0
    low, high = 0, TOP
    out = bytearray(count)
    pmin, pmax, cmin, cmax, max_flushes, overruns = 4096, -1, 0, 65535, 0, 0
    read_at = stats["read_at"]
    ok = True
    for i in range(count):
        ctx = 1
        for _ in range(8):
            pc1 = counter1[ctx]
            a, b = pc1[256], pc1[c1]
            p = (13 * (a + b) + 6 * pc1[c2]) >> 5
            idx = p >> 12
            pc2 = counter2[ctx | run_mask]
            x1, x2 = pc2[idx], pc2[idx + 1]
            pred = (p + p + 3 * (x1 + x2) + 64) >> 7
            if pred < pmin:
                pmin = pred
            if pred > pmax:
                pmax = pred
            split = ((((high - low) >> 4) * pred) >> 8) + low
            if split >= current:
                high = split
                a -= (a - PSCALE + 16) >> FAST_RATE
                b -= (b - PSCALE + 16) >> MEDIUM_RATE
                x1 -= (x1 - PSCALE + 16) >> SLOW_RATE
                x2 -= (x2 - PSCALE + 16) >> SLOW_RATE
                ctx += ctx + 1
                if a > cmax or b > cmax or x2 > cmax:
                    cmax = max(a, b, x2)
            else:
                low = split + 1
                a -= a >> FAST_RATE
                b -= b >> MEDIUM_RATE
                x1 -= x1 >> SLOW_RATE
                x2 -= x2 >> SLOW_RATE
                ctx += ctx
                if b < cmin or a < cmin or x1 < cmin:
                    cmin = min(a, b, x1)
            pc1[256] = a
            pc1[c1] = b
            pc2[idx] = x1
            pc2[idx + 1] = x2
            reads = 0
            while ((low ^ high) & MASK_24_56) == 0:
                low = (low << 32) & MASK_0_56
                high = ((high << 32) | MASK_0_32) & MASK_0_56
                reads += 1
                read_at.append(i)
                if index + 4 > buf_limit:
                    current = (current << 32) & MASK_0_56
                    index = buf_limit + 1
                    overruns += 1
                else:
                    current = ((current << 32) | int.from_bytes(buf[index:index + 4], "big")) & MASK_0_56
                    index += 4
            if reads > max_flushes:
                max_flushes = reads
        val = ctx & 0xFF
        out[i] = val
        c2 = c1
        c1 = val
        run_mask = 0x100 if c1 == c2 else 0
        if index > buf_limit:                                  # :159-160
            ok = False
            break
    stats.update(pmin=pmin, pmax=pmax, cmin=cmin, cmax=cmax, max_flushes=max_flushes, overruns=overruns)
    return ok, bytes(out), 8 * pos


def greedy_adversary(n):
    """n bytes, every bit the one the predictor thinks less likely (pred is the probability of a 1 in 1/4096): the input that
    makes this coder expand the most among those a bit-by-bit choice finds"""
    pr = Predictor()
    out = bytearray(n)
    for i in range(n):
        v = 0
        for _ in range(8):
            bit = 0 if pr.get() >= 2048 else 1
            pr.update(bit)
            v = (v << 1) | bit
        out[i] = v
    return bytes(out)


def encode_steps(data, trace=None):
    """encode() again, statement by statement as the Java has it, with the Predictor class: -> (bytes, nbits).  `trace` collects
    (pred, low, high) behind every bit, before the flush loop."""
    pr = Predictor()
    low, high = 0, TOP
    sba = bytearray()
    for val in data:
        for sh in (7, 6, 5, 4, 3, 2, 1, 0):
            bit = (val >> sh) & 1
            pred = pr.get()
            split = (((high - low) >> 4) * pred) >> 8
            if bit == 0:
                low += split + 1
            else:
                high = low + split
            pr.update(bit)
            if trace is not None:
                trace.append((pred, low, high))
            while ((low ^ high) & MASK_24_56) == 0:
                sba += ((high >> 24) & MASK_0_32).to_bytes(4, "big")
                low = (low << 32) & 0xFFFFFFFFFFFFFFFF
                high = ((high << 32) | MASK_0_32) & 0xFFFFFFFFFFFFFFFF
    out = (varint(len(sba)) + bytes(sba) if data else b"") + ((low | MASK_0_24) & MASK_0_56).to_bytes(7, "big")
    return out, 8 * len(out)
