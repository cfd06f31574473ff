"""CPU model of the range ANS coder at order 0 and order 1, written from the reference's Java (K/ = the kanzi Java sources,
io/github/flanglet/kanzi/), not from the HIP kernels.  EntropyCodecFactory builds ANSRangeEncoder(obs, ctx, order) and
ANSRangeDecoder(ibs, ctx, order) (entropy/EntropyCodecFactory.java:124-128, :175-179): ANS0 is order 0, ANS1 is order 1.

encode(data, order, lr, chunk) -> (bytes, bits); decode(data, nbits, count, order, chunk) -> (return value, bytes, bits consumed,
clean).  Where the Java throws, decode raises katmodels.JavaException (the block fails).  `clean` is False when a chunk's byte count
does not come out (decodeChunkV2 returns false, ANSRangeDecoder.java:439): decode() then stops and still returns count (:217-219);
the bytes it never wrote are zero here, as the GPU decoder leaves them."""
from katmodels import JavaException, _encode_alphabet, _normalize, _write_varint

ANS_TOP = 1 << 15                                           # ANSRangeEncoder.java:37
MAX_CHUNK_SIZE = 1 << 27                                    # :46


def default_params(order):
    """(logRange, chunk size) of the (obs, ctx, order) constructors: ANSRangeEncoder.java:154-156, ANSRangeDecoder.java:130-131
    (bit stream version >= 4): lr 12 / 16 KiB at order 0, lr 11 / 16 KiB << 8 = 4 MiB at order 1."""
    return (12, 16384) if order == 0 else (11, min(16384 << 8, MAX_CHUNK_SIZE))


class _Bits:
    """MSB-first bit string (K/bitstream/DefaultOutputBitStream.java:103-123), katmodels._Bits's interface; whole bytes leave the
    accumulator at once, so that a 4 MiB block is written in linear time"""

    def __init__(self):
        self.out, self.acc, self.na, self.n = bytearray(), 0, 0, 0

    def write(self, value, count):
        self.acc = (self.acc << count) | (value & ((1 << count) - 1))
        self.na += count
        self.n += count
        if self.na >= 8:
            nb = self.na >> 3
            rest = self.na - 8 * nb
            self.out += (self.acc >> rest).to_bytes(nb, "big")
            self.acc &= (1 << rest) - 1
            self.na = rest

    def bytes(self):
        return bytes(self.out) + ((self.acc << (8 - self.na)).to_bytes(1, "big") if self.na else b"")


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


class _EncSymbol:
    """ANSRangeEncoder.Symbol (:463-496); a fresh one (new Symbol(), :278-283) is all zero"""

    def __init__(self):
        self.x_max = self.bias = self.cmpl = self.inv_shift = self.inv_freq = 0

    def reset(self, cum, freq, lr):
        if freq >= 1 << lr:
            freq = (1 << lr) - 1
        self.x_max = _i32(((ANS_TOP >> lr) << 16) * freq)
        self.cmpl = (1 << lr) - freq
        if freq < 2:
            self.inv_freq, self.inv_shift, self.bias = 0xFFFFFFFF, 32, cum + (1 << lr) - 1
        else:
            shift = 0
            while freq > (1 << shift):
                shift += 1
            self.inv_freq = (((1 << (shift + 31)) + freq - 1) // freq) & 0xFFFFFFFF
            self.inv_shift, self.bias = 32 + shift - 1, cum


def _histogram(chunk, order):
    """rebuildStatistics :419-449 -> freqs[ctx][sym] (order 0: one context).  Order 1: Global.computeHistogramOrder1
    (Global.java:341-390) on each quarter; inside a range of 32 bytes or more its four interleaved walks chain up (prv1 =
    block[n1 - 1], ...), so every range is one walk that starts in context 0.  With quarter 0 the whole chunk is one range;
    otherwise the len & 3 tail bytes are not counted."""
    dim = 256 if order else 1
    freqs = [[0] * 256 for _ in range(dim)]
    if order == 0:
        for b in chunk:
            freqs[0][b] += 1
        return freqs
    quarter = len(chunk) >> 2
    ranges = [(0, len(chunk))] if quarter == 0 else [(q * quarter, (q + 1) * quarter) for q in range(4)]
    for s, e in ranges:
        prv = 0
        for i in range(s, e):
            freqs[prv][chunk[i]] += 1
            prv = chunk[i]
    return freqs


def _header_freqs(bs, alphabet, freqs, lr):
    """encodeHeader :221-250, after encodeAlphabet"""
    n = len(alphabet)
    if n <= 1:
        return
    chk = 8 if n >= 64 else 6
    llr = 3
    while (1 << llr) <= lr:
        llr += 1
    for i in range(1, n, chk):
        endj = min(i + chk, n)
        mx = max(freqs[alphabet[j]] - 1 for j in range(i, endj))
        log_max = 0
        while (1 << log_max) <= mx:
            log_max += 1
        bs.write(log_max, llr)
        if log_max:
            for j in range(i, endj):
                bs.write(freqs[alphabet[j]] - 1, log_max)


def encode(data, order=1, lr=None, chunk=None):
    """ANSRangeEncoder.encode :263-305.  lr / chunk default to the factory's (default_params); at order 1 the (bs, order, chunk, lr)
    constructor takes max(lr - 1, 8) and chunk << 8 (:126-127): here lr and chunk are the values the coder runs with."""
    data = bytes(data)
    dlr, dchunk = default_params(order)
    lr = dlr if lr is None else lr
    chunk = dchunk if chunk is None else chunk
    bs = _Bits()
    count = len(data)
    if count <= 32:                                                        # :267-270
        for b in data:
            bs.write(b, 8)
        return bs.bytes(), bs.n
    dim = 256 if order else 1
    symbols = [[_EncSymbol() for _ in range(256)] for _ in range(dim)]     # :278-283, once per block
    for start in range(0, count, chunk):
        end = min(start + chunk, count)
        freqs = _histogram(data[start:end], order)
        bs.write(lr - 8, 3)                                                # updateFrequencies :167
        total_alpha = 0
        for k in range(dim):
            f = freqs[k]
            alphabet = _normalize(f, sum(f), 1 << lr)                     # EntropyUtils.normalizeFrequencies (64-bit product)
            cum = 0
            for i in alphabet:                                             # :177-186 (ascending symbol order)
                symbols[k][i].reset(cum, f[i], lr)
                cum += f[i]
            _encode_alphabet(bs, alphabet)                                 # encodeHeader :211-219
            _header_freqs(bs, alphabet, f, lr)
            total_alpha += len(alphabet)
        if order == 0 and total_alpha <= 1:                                # :292-295, order 0 only
            continue
        _encode_chunk(bs, data, start, end, order, symbols)
    return bs.bytes(), bs.n


def _encode_chunk(bs, block, start, end, order, symbols):
    """encodeChunk :337-407 with encodeSymbol :315-328: the chunk is coded backwards into the END of a buffer (built reversed
    here: rev[0] is the buffer's last byte)"""
    rev = bytearray()
    end4 = start + ((end - start) & -4)
    for i in range(end - 1, end4 - 1, -1):
        rev.append(block[i])
    st = [ANS_TOP] * 4

    def enc(state, sym):
        if state >= sym.x_max:                                             # int compare: both sides are below 2^31
            rev.append(state & 0xFF)
            rev.append((state >> 8) & 0xFF)
            state >>= 16
        q = (state * sym.inv_freq) >> sym.inv_shift
        return _i32(state + sym.bias + _i32(q) * sym.cmpl) & 0xFFFFFFFF

    if order == 0:
        symb = symbols[0]
        i = end4 - 1
        while i > start:
            for lane in range(4):
                st[lane] = enc(st[lane], symb[block[i - lane]])
            i -= 4
    else:
        quarter = (end4 - start) >> 2                                      # :361-389
        idx = [start + (q + 1) * quarter - 2 for q in range(3)] + [end4 - 2]
        prv = [block[i + 1] for i in idx]                                  # quarter 0: block[start - 1], the previous chunk's last byte
        while idx[0] >= start:
            for lane in range(4):
                cur = block[idx[lane]]
                st[lane] = enc(st[lane], symbols[cur][prv[lane]])
                prv[lane] = cur
                idx[lane] -= 1
        for lane in range(4):                                              # each quarter's first byte, in context 0
            st[lane] = enc(st[lane], symbols[0][prv[lane]])
    _write_varint(bs, len(rev))                                            # :393-396
    for s in st:
        bs.write(s, 32)
    if rev:
        bs.write(int.from_bytes(bytes(reversed(rev)), "big"), 8 * len(rev))


class _DecSymbol:
    """ANSRangeDecoder.Symbol (:561-580)"""

    def __init__(self):
        self.cum = self.freq = 0


def decode(data, nbits, count, order=1, chunk=None):
    """ANSRangeDecoder.decode :188-236 (bit stream version >= 4), decodeHeader :452-544, decodeChunkV2 :357-440."""
    src = bytes(data)
    big = int.from_bytes(src, "big") if src else 0
    total = len(src) * 8
    pos = 0
    chunk = default_params(order)[1] if chunk is None else chunk

    def read_bits(n):
        nonlocal pos
        if n == 0:
            return 0
        if pos + n > nbits or pos + n > total:
            raise JavaException("BitStreamException: end of stream")
        v = (big >> (total - pos - n)) & ((1 << n) - 1)
        pos += n
        return v

    out = bytearray(count)
    if count <= 32:                                                        # :193-196
        for i in range(count):
            out[i] = read_bits(8)
        return count, bytes(out), pos, True
    dim = 256 if order else 1
    freqs = [[0] * 256 for _ in range(dim)]                                # the decoder object lives for one block
    f2s = [bytearray() for _ in range(dim)]                                # new byte[0] (:142): decoding into it throws
    symbols = [[_DecSymbol() for _ in range(256)] for _ in range(dim)]
    buf = bytearray()
    log_range = 12
    start = 0
    while start < count:
        end = min(start + chunk, count)
        # ---- decodeHeader :452-544 ----
        log_range = 8 + read_bits(3)
        scale = 1 << log_range
        total_alpha = 0
        for k in range(dim):
            if read_bits(1) == 0:                                          # EntropyUtils.decodeAlphabet
                alphabet = [] if read_bits(1) == 1 else list(range(256))
            else:
                last = read_bits(5)
                alphabet = []
                for i in range(last + 1):
                    m = read_bits(8)
                    alphabet += [(i << 3) + j for j in range(8) if m & (1 << j)]
            asz = len(alphabet)
            if asz == 0:                                                   # :467-468: the context keeps its tables
                continue
            llr = 3
            while (1 << llr) <= log_range:
                llr += 1
            f = freqs[k]
            if asz != 256:
                f[:] = [0] * 256
            if len(f2s[k]) < scale:
                f2s[k] = bytearray(scale)
            chk = 8 if asz >= 64 else 6
            s = 0
            for i in range(1, asz, chk):
                log_max = read_bits(llr)
                if (1 << log_max) > scale:
                    raise JavaException("BitStreamException: incorrect frequency size")
                for j in range(i, min(i + chk, asz)):
                    fr = 1 if log_max == 0 else 1 + read_bits(log_max)
                    if fr <= 0 or fr >= scale:
                        raise JavaException("BitStreamException: incorrect frequency")
                    f[alphabet[j]] = fr
                    s += fr
            if scale <= s:
                raise JavaException("BitStreamException: incorrect frequency (first symbol)")
            f[alphabet[0]] = scale - s
            s = 0
            for i in range(256):                                           # reverse mapping :528-538
                if f[i] == 0:
                    continue
                f2s[k][s:s + f[i]] = bytes([i]) * f[i]
                symbols[k][i].cum = s
                symbols[k][i].freq = scale - 1 if f[i] >= scale else f[i]  # Symbol.reset :576-579
                s += f[i]
            total_alpha += asz
        if total_alpha == 0:                                               # :213-215
            return start, bytes(out), pos, True
        if order == 0 and total_alpha == 1:                                # :217-220
            a = next(i for i in range(256) if freqs[0][i])
            out[start:end] = bytes([a]) * (end - start)
            start = end
            continue
        # ---- decodeChunkV2 :357-440 ----
        value = read_bits(8)
        sz = value & 0x7F
        shift = 7
        while value >= 128:
            value = read_bits(8)
            sz |= (value & 0x7F) << shift
            if shift == 28:
                break
            shift += 7
        sz = _i32(sz)
        if sz >= MAX_CHUNK_SIZE:                                           # :360-361
            return count, bytes(out), pos, False
        st = [read_bits(32) for _ in range(4)]                             # st0 .. st3
        min_buf = max(2 * (end - start), 256)
        if len(buf) < min_buf:
            buf = bytearray(min_buf)
        buf[:] = bytes(len(buf))
        if sz < 0 or sz > len(buf):
            raise JavaException("ArrayIndexOutOfBounds / negative length")
        if sz:
            buf[:sz] = read_bits(8 * sz).to_bytes(sz, "big")
        n = 0
        mask = scale - 1
        end4 = start + ((end - start) & -4)

        def step(lane, table_k, sym_k, i):
            nonlocal n
            x = st[lane]
            if (x & mask) >= len(table_k):
                raise JavaException("ArrayIndexOutOfBounds: f2s")
            cur = table_k[x & mask]
            out[i] = cur
            sym = sym_k[cur]
            x = (sym.freq * (x >> log_range) + (x & mask) - sym.cum) & 0xFFFFFFFF
            if _i32(x) < ANS_TOP:                                          # decodeSymbol :326-334
                x = ((x << 16) | (buf[n] << 8) | buf[n + 1]) & 0xFFFFFFFF
                n += 2
            st[lane] = x
            return cur

        if order == 0:
            for i in range(start, end4, 4):
                for lane in (3, 2, 1, 0):
                    step(lane, f2s[0], symbols[0], i + 3 - lane)
        else:                                                              # :406-432
            quarter = (end4 - start) >> 2
            prv = [0, 0, 0, 0]
            for j in range(quarter):
                for lane in (3, 2, 1, 0):
                    prv[lane] = step(lane, f2s[prv[lane]], symbols[prv[lane]], start + lane * quarter + j)
        for i in range(end4, end):                                         # :436-437
            out[i] = buf[n]
            n += 1
        if n != sz:                                                        # :439
            return count, bytes(out), pos, False
        start = end
    return count, bytes(out), pos, True
