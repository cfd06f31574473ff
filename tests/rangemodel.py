"""CPU model of the order-0 range coder (entropy id 4, RANGE), written line by line from the reference's Java (K/ = the kanzi Java
sources, io/github/flanglet/kanzi/): K/entropy/RangeEncoder.java and K/entropy/RangeDecoder.java, not from the HIP kernels.
EntropyCodecFactory builds RangeEncoder(obs) / RangeDecoder(ibs): chunk size 32 KiB, logRange 12 (RangeEncoder.java:65-70, :110-112).

encode(data, lr, chunk) -> (bytes, bits); decode(data, nbits, count, chunk) -> (return value, bytes, bits consumed).  Where the Java
throws, both raise katmodels.JavaException (the block fails).  Java's `long` is emulated exactly: every value is kept masked to 64
bits and read as signed where the Java compares (`range > BOTTOM_RANGE`), divides, casts to int or indexes an array.

The normalisation loop (RangeEncoder.java:303-315, RangeDecoder.java:312-324) has no exit when `range` is 0: the top bits of low and
low + 0 always agree.  Each pass shifts range and low left by 28 bits, so a non-zero range survives at most three passes without the
low-range branch, and from the second pass of a byte on, low's 28 low bits are zero: the branch `range = -low & 0xFFFF` then gives
0.  A byte that makes more than MAX_PASSES passes therefore never leaves the loop.  The Java encoder would write until memory runs
out; the Java decoder reads 28 bits per pass and throws at the end of the stream.  Both fail the block here (JavaException), as the
device does.  Valid input cannot get there: on the FIRST pass the branch is only taken when bits 32..59 of low and low + range differ
with range <= 0xFFFF, i.e. low mod 2^32 >= 2^32 - 0xFFFF, whose low 16 bits are not zero, so -low & 0xFFFF >= 1; and the encoder's
frequencies are >= 1.  A decoder reaches range = 0 through a stale f2s entry (a symbol of frequency 0 in the current chunk).

low_range_hits lists, per coded chunk of the last encode() / decode() call, how often `range = -low & 0xFFFF` ran; stale_reads[0]
counts the last decode()'s f2s reads at or above the chunk's scale (entries an earlier, wider chunk of the block left there)."""
from katmodels import JavaException, _encode_alphabet, _normalize
from ans1model import _Bits

TOP_RANGE = 0x0FFFFFFFFFFFFFFF                              # RangeEncoder.java:50
BOTTOM_RANGE = 0x000000000000FFFF                           # :55
RANGE_MASK = 0x0FFFFFFF00000000                             # :60
DEFAULT_CHUNK_SIZE = 1 << 15                                # :65
DEFAULT_LOG_RANGE = 12                                      # :70
MAX_PASSES = 8                                              # see the module docstring: more passes in one byte never end
M64 = (1 << 64) - 1

low_range_hits = []                                         # one entry per coded chunk of the last encode() / decode() call
stale_reads = [0]                                           # f2s reads at or above the chunk's scale in the last decode() call


def _s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def _jdiv(a, b):
    """Java's long division: truncates toward zero"""
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def encode_header(bs, alphabet, freqs, lr):
    """RangeEncoder.encodeHeader :186-228"""
    _encode_alphabet(bs, alphabet)
    n = len(alphabet)
    if n == 0:                                                                  # encoded == 0 :192-193
        return
    bs.write(lr - 8, 3)
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
        if log_max == 0:
            continue
        for j in range(i, endj):
            bs.write(freqs[alphabet[j]] - 1, log_max)


def encode_chunk(bs, data, lr):
    """one pass of the loop of RangeEncoder.encode :255-279 -> times the low-range branch ran"""
    freqs = [0] * 256
    for b in data:                                                              # rebuildStatistics :328-331
        freqs[b] += 1
    alphabet = _normalize(freqs, len(data), 1 << lr)                           # updateFrequencies :159-175
    cum = [0] * 257
    for i in range(256):
        cum[i + 1] = cum[i] + freqs[i]
    encode_header(bs, alphabet, freqs, lr)
    if len(alphabet) <= 1:                                                      # :265-269
        return 0
    low, rng, hits = 0, TOP_RANGE, 0
    for b in data:                                                              # encodeByte :292-316
        c = cum[b]
        f = cum[b + 1] - c
        rng >>= lr
        low = (low + c * rng) & M64
        rng = (rng * f) & M64
        passes = 0
        while True:
            if ((low ^ (low + rng)) & RANGE_MASK) != 0:
                if _s64(rng) > BOTTOM_RANGE:
                    break
                rng = (-low) & BOTTOM_RANGE
                hits += 1
            passes += 1
            if passes > MAX_PASSES:
                raise JavaException("range encoder: the normalisation loop does not end (range == 0)")
            bs.write(low >> 32, 28)
            rng = (rng << 28) & M64
            low = (low << 28) & M64
    bs.write(low, 60)                                                           # :277
    return hits


def encode(data, lr=DEFAULT_LOG_RANGE, chunk=DEFAULT_CHUNK_SIZE):
    """RangeEncoder.encode :244-282"""
    data = bytes(data)
    bs = _Bits()
    low_range_hits.clear()
    for start in range(0, len(data), chunk):
        end = min(start + chunk, len(data))
        clr = lr
        while clr > 8 and (1 << clr) > end - start:                            # :262-263
            clr -= 1
        low_range_hits.append(encode_chunk(bs, data[start:end], clr))
    return bs.bytes(), bs.n


def decode(data, nbits, count, chunk=DEFAULT_CHUNK_SIZE):
    """RangeDecoder.decode :254-292, decodeHeader :161-239, decodeByte :300-327"""
    src = bytes(data)
    big = int.from_bytes(src, "big") if src else 0
    total = len(src) * 8
    pos = 0

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
    low_range_hits.clear()
    stale_reads[0] = 0
    freqs = [0] * 256                                                           # the decoder object lives for one block
    cum = [0] * 257
    f2s = []                                                                    # new short[0] :149
    start = 0
    while start < count:
        end = min(start + chunk, count)
        # ---- decodeHeader :161-239 ----
        if read_bits(1) == 0:                                                   # EntropyUtils.decodeAlphabet
            alphabet = [] if read_bits(1) == 1 else list(range(256))
        else:
            last = read_bits(5)
            alphabet = []
            for i in range(last + 1):
                m = read_bits(8)
                alphabet += [(i << 3) + j for j in range(8) if m & (1 << j)]
        asz = len(alphabet)
        if asz == 0:                                                            # :164-165, :269-270
            return start, bytes(out), pos
        if asz != 256:
            freqs[:] = [0] * 256
        log_range = 8 + read_bits(3)
        scale = 1 << log_range
        s = 0
        chk = 8 if asz >= 64 else 6
        llr = 3
        while (1 << llr) <= log_range:
            llr += 1
        for i in range(1, asz, chk):
            log_max = read_bits(llr)
            if (1 << log_max) > scale:
                raise JavaException("BitStreamException: incorrect frequency size")
            for j in range(i, min(i + chk, asz)):
                fr = 1 if log_max == 0 else 1 + read_bits(log_max)
                if fr <= 0 or fr >= scale:
                    raise JavaException("BitStreamException: incorrect frequency")
                freqs[alphabet[j]] = fr
                s += fr
        if scale <= s:
            raise JavaException("BitStreamException: incorrect frequency (first symbol)")
        freqs[alphabet[0]] = scale - s
        if len(f2s) < scale:                                                    # :226-227: grows only, a new array is all zero
            f2s = [0] * scale
        for i in range(256):                                                    # :230-236
            cum[i + 1] = cum[i] + freqs[i]
            f2s[cum[i]:cum[i + 1]] = [i] * freqs[i]
        if asz == 1:                                                            # :272-279
            out[start:end] = bytes([alphabet[0]]) * (end - start)
            start = end
            continue
        rng, low, hits = TOP_RANGE, 0, 0                                       # :281-283
        code = read_bits(60)
        for i in range(start, end):                                             # decodeByte :300-327
            rng >>= log_range
            cnt = _i32(_jdiv(_s64(code - low), _s64(rng)))
            if not 0 <= cnt < len(f2s):
                raise JavaException("ArrayIndexOutOfBounds: f2s[%d]" % cnt)
            sym = f2s[cnt]
            if cnt >= scale:
                stale_reads[0] += 1
            c = cum[sym]
            f = cum[sym + 1] - c
            low = (low + c * rng) & M64
            rng = (rng * f) & M64
            passes = 0
            while True:
                if ((low ^ (low + rng)) & RANGE_MASK) != 0:
                    if _s64(rng) > BOTTOM_RANGE:
                        break
                    rng = (-low) & BOTTOM_RANGE
                    hits += 1
                passes += 1
                if passes > MAX_PASSES:                                         # the Java reads on to the end of the stream and throws
                    raise JavaException("BitStreamException: end of stream (range == 0)")
                code = ((code << 28) | read_bits(28)) & M64
                rng = (rng << 28) & M64
                low = (low << 28) & M64
            out[i] = sym
        low_range_hits.append(hits)
        start = end
    return count, bytes(out), pos
