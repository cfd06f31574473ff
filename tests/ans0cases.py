"""The deterministic case set of the device's ANS0 coder (kanzi_amd/csrc/kz_ans.hip): inputs chosen for what its kernels do with
them -- which branch of the data-parallel normalizeFrequencies a chunk takes, which header form it writes, how the four-lane
coding loop ends, where chunk bit strings meet in the spliced output, which event ends a decode -- not for what they hold.
tests/test_ans0_cases.py proves on the CPU that every seam named below is reached and that model and oracle agree on every
case; tests/test_gpu_ans0.py runs the set on the device, bit for bit against the CPU oracle.

No coder model of its own: ans1model.encode(data, 0, lr=...) / ans1model.decode(..., order=0) are ANS0, written from the Java.
chunk_facts() classifies a chunk by the reference's rules (a walk of katmodels._normalize that also says which way it went; the
test asserts both leave the same frequencies); chunk_code() is the bit string of one chunk alone.  At order 0 every chunk is
coded independently, so a block's stream is the concatenation of the streams of its chunks (a whole block of 32 bytes or fewer
is stored raw instead); block_layout() reads the per-chunk positions out of the oracle's stream, and the crafted decoder streams
are assembled from per-chunk bit strings with one or two chunks altered.

Seeded generators only.  A payload of 16384 bytes (a three-byte size varint) needs 8 bits per symbol or more: `exact`, 64 of each
of 256 symbols, costs exactly 8 bits a symbol at frequency 16 / 4096 and its four states give back what they took, 16384 bytes
to the byte; random uniform chunks stay some twenty bytes below (their histogram's entropy is that much under 8 bits), and
`varint_edge` -- half the symbols at 62, half at 66, the slow path lowering the 62s, the most the normalisation can add -- ends
at 16380.

slow- at the round limit is the reference's own defect, kept: the remainder is subtracted from the maximum although the sum was
short (EntropyUtils.java:248), the frequencies of `slow-_limit` sum to 3996, and the reference's decoder does not return the
chunk (test_ans0_cases.py::test_slow_minus_at_the_round_limit).  The device writes the same bits and decodes them the same way.

What cannot occur, so that no case stands for it:

 * Two branches of normalizeFrequencies at scale 4096 with at most 256 symbols (normalize_path marks both, and
   test_classifier_walks_normalize asserts that no chunk of the set takes them):
   "No symbol left to adjust" (a slow round that adjusts nothing) needs every frequency at 2 or below, a sum of 512 at most.  But
   every scaled frequency is within 1/2 below its true value (or raised to 1), so the scaled sum is at least 4096 - 128 = 3968;
   slow+ only removes the surplus above 4096 and slow- only adds: the sum never falls below 3968, the mean never below 15.
   The clamp max(freqs[idxMax] - delta, 1) needs the remainder R of five rounds to reach the maximum M (less the sixteenth taken
   first).  With E symbols above 2, each round takes E, and delta < (256 - E) + E / 2: a symbol raised to 1 adds less than 1, any
   other at most 1/2.  A symbol at 2 or below that adds 1/2 holds at most 1.5 of the 4096 and one that adds nearly 1 holds nearly
   nothing (holding more costs as much surplus as it takes from the rest, and the rest is shared by E), so the mean of the E
   symbols, and M, is at least (4096 - 1.5 (256 - E)) / E.  R < 256 - 5.5 E against 15/16 M > 3480 / E: E (256 - 5.5 E) peaks
   below 2980.  On the slow- side R < 128 - 5 E.  (slow+ at the round limit below: M = 672 - 42, R = 114.)
 * winOk false in k_ans_dec_chunk (the register window would read past the slot): see tests/test_gpu_ans0.py."""
import dataclasses
import functools

import numpy as np

import ans1model
import katmodels
import oracle

CHUNK = 16384
LR = 12


# ---- bit strings ------------------------------------------------------------------------------------------------------------
def bitstr(data, nbits):
    """'0' / '1' characters of the first nbits bits of data (MSB first)"""
    return format(int.from_bytes(data, "big"), "0%db" % (8 * len(data)))[:nbits] if nbits else ""


def pack(s):
    """-> (bytes, bits) of a '0' / '1' string, the last byte zero padded"""
    n = len(s)
    return (int(s + "0" * (-n % 8), 2).to_bytes((n + 7) // 8, "big") if n else b""), n


def _bits_of(value, count):
    return format(value, "0%db" % count) if count else ""


def varint(v):
    """EntropyUtils.writeVarInt as a bit string"""
    bs = ans1model._Bits()
    katmodels._write_varint(bs, v)
    return bitstr(bs.bytes(), bs.n)


def read_varint(s, pos):
    """EntropyUtils.readVarInt at bit pos of a bit string -> (value, bits read)"""
    v = int(s[pos:pos + 8], 2)
    sz, shift, used = v & 0x7F, 7, 8
    while v >= 128:
        v = int(s[pos + used:pos + used + 8], 2)
        used += 8
        sz |= (v & 0x7F) << shift
        if shift == 28:
            break
        shift += 7
    return sz, used


# ---- one chunk by the reference's rules --------------------------------------------------------------------------------------
def counts(chunk):
    return np.bincount(np.frombuffer(bytes(chunk), dtype=np.uint8), minlength=256).tolist()


def normalize_path(freqs, total, scale):
    """EntropyUtils.normalizeFrequencies :141-250 as katmodels._normalize walks it (freqs modified in place), and which way it went:
    -> (alphabet, facts).  path: shortcut (total == scale), one (a single symbol), exact (the scaled sum is the scale), fast+ / fast-
    (|delta| within a sixteenth of the maximum; + when the scaled sum is above the scale), slow+ / slow- (rounds over the alphabet);
    rounds: slow rounds run; limit: five rounds done and delta still positive, the remainder taken from the maximum."""
    facts = {"path": None, "rounds": 0, "limit": False, "tied": False, "max_groups": [], "first_max_group": None}
    alphabet = [i for i in range(256) if freqs[i]]
    if total == scale:
        facts["path"] = "shortcut"
        return alphabet, facts
    sum_scaled, idx_max = 0, alphabet[0]
    for i in alphabet:
        sf = freqs[i] * scale
        freqs[i] = 1 if sf <= total else (sf + (total >> 1)) // total
        sum_scaled += freqs[i]
    for i in alphabet:                                          # :184-185: the first symbol holding the maximum (strict >)
        if freqs[i] > freqs[idx_max]:
            idx_max = i
    holders = [i for i in alphabet if freqs[i] == freqs[idx_max]]
    facts["tied"] = len(holders) > 1
    facts["max_groups"] = sorted({i >> 6 for i in holders})
    facts["first_max_group"] = idx_max >> 6
    if len(alphabet) == 1:
        freqs[alphabet[0]] = scale
        facts["path"] = "one"
        return alphabet, facts
    if sum_scaled == scale:
        facts["path"] = "exact"
        return alphabet, facts
    delta = sum_scaled - scale
    sign = "+" if delta > 0 else "-"
    err_thr = freqs[idx_max] >> 4
    if abs(delta) <= err_thr:
        freqs[idx_max] -= delta
        facts["path"] = "fast" + sign
        return alphabet, facts
    facts["path"] = "slow" + sign
    if delta < 0:
        delta += err_thr
        freqs[idx_max] += err_thr
    else:
        delta -= err_thr
        freqs[idx_max] -= err_thr
    inc = -1 if delta > 0 else 1
    delta = abs(delta)
    rnd = 0
    while True:
        rnd += 1
        if not (rnd < 6 and delta > 0):
            break
        adjustments = 0
        for idx in alphabet:
            if freqs[idx] <= 2:
                continue
            freqs[idx] += inc
            adjustments += 1
            delta -= 1
            if delta == 0:
                break
        facts["rounds"] += 1
        if adjustments == 0:
            facts["no_symbol_left"] = True
            break
    facts["limit"] = rnd == 6 and delta > 0
    if freqs[idx_max] - delta < 1:
        facts["clamped"] = True
    freqs[idx_max] = max(freqs[idx_max] - delta, 1)
    return alphabet, facts


def _header(chunk, lr):
    """-> (_Bits holding the chunk's header, alphabet, normalised frequencies, path facts)"""
    f = counts(chunk)
    alphabet, facts = normalize_path(f, len(chunk), 1 << lr)
    bs = ans1model._Bits()
    bs.write(lr - 8, 3)                                         # ANSRangeEncoder.updateFrequencies :167
    katmodels._encode_alphabet(bs, alphabet)
    ans1model._header_freqs(bs, alphabet, f, lr)
    return bs, alphabet, f, facts


@functools.lru_cache(maxsize=None)
def chunk_code(chunk, lr=LR):
    """the bit string of one chunk (up to 16384 bytes) as ANSRangeEncoder.encode writes it inside a block of more than 32 bytes
    -> ('0' / '1' string, header bits, payload bytes).  The frequencies are katmodels._normalize's, the coding ans1model's."""
    chunk = bytes(chunk)
    assert 0 < len(chunk) <= CHUNK
    f = counts(chunk)
    alphabet = katmodels._normalize(f, len(chunk), 1 << lr)
    bs = ans1model._Bits()
    bs.write(lr - 8, 3)
    symbols = [ans1model._EncSymbol() for _ in range(256)]
    cum = 0
    for i in alphabet:
        symbols[i].reset(cum, f[i], lr)
        cum += f[i]
    katmodels._encode_alphabet(bs, alphabet)
    ans1model._header_freqs(bs, alphabet, f, lr)
    hb = bs.n
    if len(alphabet) > 1:
        ans1model._encode_chunk(bs, chunk, 0, len(chunk), 0, [symbols])
    s = bitstr(bs.bytes(), bs.n)
    return s, hb, (read_varint(s, hb)[0] if len(alphabet) > 1 else 0)


def chunk_facts(chunk, lr=LR, code=True):
    """What one chunk makes the encoder do, from the reference's rules.  code=False leaves out what needs the chunk coded by the
    Python model (payload, varint, total_bits)."""
    chunk = bytes(chunk)
    bs, alphabet, f, facts = _header(chunk, lr)
    n = len(alphabet)
    out = dict(facts)
    out["alphabet_size"] = n
    out["form"] = "256" if n == 256 else ("1" if n == 1 else "partial")
    out["last_mask"] = None if n == 256 else alphabet[-1] >> 3
    out["group"] = None if n <= 1 else (8 if n >= 64 else 6)
    groups = [] if n <= 1 else [alphabet[i:i + out["group"]] for i in range(1, n, out["group"])]
    out["logmax0"] = any(max(f[s] for s in g) == 1 for g in groups)
    out["last_group"] = len(groups[-1]) if groups else None
    out["len3"] = len(chunk) & 3
    out["dwords3"] = (len(chunk) >> 2) & 3
    out["header_bits"] = bs.n
    if code:
        s, hb, payload = chunk_code(chunk, lr)
        assert hb == bs.n
        out["payload"] = payload
        out["varint"] = 0 if n <= 1 else len(varint(payload)) // 8
        out["total_bits"] = len(s)
    return out


def chunks_of(data):
    return [bytes(data[i:i + CHUNK]) for i in range(0, len(data), CHUNK)]


def block_layout(data, stream=None):
    """per chunk (start_bit, header_bits, total_bits) of the block's ANS0 stream, read out of the oracle's encoder output (the
    header length from the reference's rules, the payload size from the varint behind it).  A block of 32 bytes or fewer is
    one raw piece without a header."""
    data = bytes(data)
    if stream is None:
        stream = oracle.entropy_encode("ANS0", data)
    bits, nbits = stream
    if len(data) <= 32:
        return [(0, 0, 8 * len(data))]
    big, total = int.from_bytes(bits, "big"), 8 * len(bits)

    def peek(pos, n):
        return (big >> (total - pos - n)) & ((1 << n) - 1)

    out, pos = [], 0
    for c in chunks_of(data):
        fc = chunk_facts(c, code=False)
        hb = fc["header_bits"]
        tb = hb
        if fc["alphabet_size"] > 1:
            p = pos + hb
            v = peek(p, 8)
            sz, shift, used = v & 0x7F, 7, 8
            while v >= 128:
                v = peek(p + used, 8)
                used += 8
                sz |= (v & 0x7F) << shift
                shift += 7
            tb = hb + used + 128 + 8 * sz
        out.append((pos, hb, tb))
        pos += tb
    assert pos == nbits, (pos, nbits)
    return out


def splice_facts(layout):
    """what a block's layout asks of k_ans_enc_concat: the residues mod 32 of the chunk start bits, whether a chunk shorter than
    32 bits lies wholly inside one output word, and the largest number of chunks with bits in one word"""
    res = {s & 31 for s, _, t in layout if t}
    inside = any(0 < t < 32 and (s >> 5) == ((s + t - 1) >> 5) for s, _, t in layout)
    words = {}
    for s, _, t in layout:
        if t:
            for w in {s >> 5, (s + t - 1) >> 5}:                 # (the words between them hold this chunk alone)
                words[w] = words.get(w, 0) + 1
    return res, inside, max(words.values()) if words else 0


# ---- generators ------------------------------------------------------------------------------------------------------------
def from_counts(cnt, seed):
    """bytes holding symbol s cnt[s] times (cnt: dict or list of (symbol, count)), shuffled"""
    items = sorted(cnt.items()) if isinstance(cnt, dict) else list(cnt)
    a = np.concatenate([np.full(c, s, dtype=np.uint8) for s, c in items])
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def even(n, syms, seed):
    """n bytes spread evenly over syms (the first n % len(syms) of them hold one more)"""
    syms = list(syms)
    k = len(syms)
    return from_counts([(s, n // k + (1 if i < n % k else 0)) for i, s in enumerate(syms)], seed)


def rnd(seed, n, alpha=256, base=0):
    return (np.random.default_rng(seed).integers(0, alpha, n, dtype=np.uint8) + base).astype(np.uint8).tobytes()


def geometric(seed, n, p=0.3, alpha=40):
    g = np.random.default_rng(seed).geometric(p, n) - 1
    return np.minimum(g, alpha - 1).astype(np.uint8).tobytes()


def whole_alphabet(seed, n, k, syms=None):
    """n random bytes over k symbols, every one of them present"""
    syms = list(range(k)) if syms is None else list(syms)
    a = np.array(syms, dtype=np.uint8)[np.random.default_rng(seed).integers(0, k, n)]
    a[:k] = np.array(syms, dtype=np.uint8)
    np.random.default_rng(seed + 1).shuffle(a)
    return a.tobytes()


def runs(symbols):
    """one 16 KiB run per symbol: each chunk is a header and nothing else (17 bits for a symbol below 8)"""
    return b"".join(bytes([s]) * CHUNK for s in symbols)


@dataclasses.dataclass(frozen=True)
class EncCase:
    name: str
    data: bytes
    model: bool = True         # short enough for the Python model: the concatenation of chunk_code() is compared with the oracle


FULL = geometric(7, CHUNK)                                      # the full chunk the short last chunks sit behind
TAIL_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17)
SLOW_MINUS = ((3000, 200), (7000, 200), (13000, 150), (9000, 200))


@functools.lru_cache(maxsize=None)
def encoder_cases():
    cs = []

    def add(name, data, model=True):
        cs.append(EncCase(name, bytes(data), model))

    # ---- normalisation ----
    add("slow+_limit", from_counts([(s, 1) for s in range(6, 256)] + [(s, 2689) for s in range(6)], 1))
    add("slow+_3rounds", from_counts([(s, 1) for s in range(56, 256)] + [(s, 289) for s in range(56)], 2))
    add("slow+_1round", rnd(100, CHUNK))
    for n, k in SLOW_MINUS:
        add("slow-_%d_over_%d" % (n, k), even(n, range(20, 20 + k), n))
    add("slow-_limit", from_counts([(s, 6) for s in range(6, 256)] + [(s, 1417) for s in range(6)], 13))
    add("fast+", geometric(8, 12345))
    add("fast-", geometric(18, 5000))
    add("exact", even(CHUNK, range(256), 5))
    add("exact_small", even(4000, range(8), 6))
    add("shortcut", even(4096, range(256), 9))
    add("shortcut_last", FULL + even(4096, range(256), 10))
    add("shortcut_skewed", whole_alphabet(11, 4096, 256))
    add("varint_edge", from_counts([(s, 62) for s in range(128)] + [(s, 66) for s in range(128, 256)], 12))
    # ---- header forms ----
    for k in (2, 63, 64, 65, 66, 255, 256):
        add("alphabet_%d" % k, whole_alphabet(20 + k, 4099, k))
    add("alphabet_below_8", whole_alphabet(30, 777, 5, (0, 2, 3, 6, 7)))
    add("alphabet_with_255", whole_alphabet(31, 1501, 7, (1, 9, 100, 101, 200, 254, 255)))
    add("alphabet_255_missing_0", whole_alphabet(32, 5000, 255, range(1, 256)))
    add("one_symbol_3_chunks", bytes([200]) * (2 * CHUNK + 77))
    add("logmax0_groups", from_counts([(s, 1) for s in range(100, 170)] + [(3, 6000), (250, 3000)], 33))
    # ---- a tied maximum whose first holder sits in group 1, 2 or 3 while a later group holds an equal one ----
    for g, (a, b) in enumerate(((70, 200), (130, 199), (192, 255)), 1):
        add("tied_max_group_%d" % g, from_counts(dict([(a, 1500), (b, 1500), (3, 500), (a + 1, 603)] + [(s, 7) for s in range(20, 50)]), 40 + g))
    add("tied_max_four_groups", from_counts(dict([(10, 900), (80, 900), (150, 900), (220, 900)] + [(s, 5) for s in range(30, 60)]), 44))
    # ---- the four-lane coding loop: short last chunks, blocks just past the raw limit ----
    for t in TAIL_LENGTHS:
        add("tail_%d" % t, FULL + rnd(50 + t, t, 3, 65))
    for n in (33, 34, 35, 36, 37, 40, 44, 48):
        add("block_%d" % n, rnd(60 + n, n, 5, 48))
    for n in (0, 1, 16, 32):
        add("raw_%d" % n, rnd(70 + n, n))
    # ---- the payload window of the decoder ----
    add("window_uniform", rnd(80, CHUNK) + rnd(81, 3001))
    add("window_two_symbols", from_counts({65: CHUNK - 16, 66: 16}, 82) + from_counts({0: 4995, 255: 5}, 83))
    # ---- splices ----
    add("runs_12", runs([i % 8 for i in range(12)][::-1]))
    add("runs_alternated", b"".join(bytes([i % 8]) * CHUNK if i % 2 == 0 else geometric(90 + i, CHUNK, 0.05 + 0.07 * i, 200) for i in range(12)), model=False)
    add("runs_33", runs([(5 * i) % 8 for i in range(33)]) + b"\x07" * 11)
    add("runs_behind_ordinary", geometric(95, CHUNK, 0.5) + runs((1, 6)) + rnd(96, 50, 4))
    return cs


def encoder_cases_by_name():
    return {c.name: c for c in encoder_cases()}


@functools.lru_cache(maxsize=None)
def scan_case():
    """one block of 65 chunks (1 MiB + 5 bytes, mixed content): the carry of k_ans_enc_scan crosses wave iterations.  Its
    expected bits are the oracle's (the Python model codes about 150 KB/s)."""
    parts = []
    for i in range(64):
        k = i % 4
        parts.append(geometric(200 + i, CHUNK, 0.02 + 0.015 * i, 256) if k == 0 else rnd(200 + i, CHUNK, 2 + 4 * i) if k == 1
                     else bytes([i]) * CHUNK if k == 2 else whole_alphabet(200 + i, CHUNK, 256))
    return b"".join(parts) + rnd(299, 5, 3)


# ---- crafted decoder streams ---------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class DecCase:
    name: str
    bits: bytes
    nbits: int
    count: int
    event: tuple               # (kind, chunk) the stream was built for: kind in "FAIL", "SKIP", "STOP"; chunk = the one that decides


def stop_long(s, hb, extra=2):
    """the chunk's size varint raised by `extra` with that many zero bytes appended to the payload: every byte still decodes, then
    the consumed count is not the size (decodeChunkV2 returns false, ANSRangeDecoder.java:439)"""
    sz, used = read_varint(s, hb)
    return s[:hb] + varint(sz + extra) + s[hb + used:] + "0" * (8 * extra)


def stop_short(s, hb, less=2):
    """the size lowered with the last payload bytes removed: the decoder runs into the zeroed rest of its buffer"""
    sz, used = read_varint(s, hb)
    assert sz > less
    return s[:hb] + varint(sz - less) + s[hb + used:len(s) - 8 * less]


def skip(s, hb):
    """the varint 80 80 80 40 = 2^27 = MAX_CHUNK_SIZE: decodeChunkV2 returns false before it reads anything else (:360-361)"""
    sz, used = read_varint(s, hb)
    return s[:hb] + bitstr(bytes([0x80, 0x80, 0x80, 0x40]), 32) + s[hb + used:]


def set_size(s, hb, new):
    sz, used = read_varint(s, hb)
    return s[:hb] + varint(new) + s[hb + used:]


def _alphabet_bits(chunk):
    bs = ans1model._Bits()
    katmodels._encode_alphabet(bs, [i for i in range(256) if counts(chunk)[i]])
    return bs.n


def bad_logmax(s, chunk):
    """the first frequency group's logMax field set to 13: 1 << 13 > scale"""
    at = 3 + _alphabet_bits(chunk)
    return s[:at] + "1101" + s[at + 4:]


EMPTY_ALPHABET = "100" + "01"                                  # lr 12, FULL_ALPHABET / ALPHABET_0


def sum_at_scale():
    """three symbols, the two written frequencies 2048 each: their sum is the scale, nothing is left for the first symbol"""
    return "100" + "1" + "00000" + "00000111" + "1100" + _bits_of(2047, 12) * 2 + varint(0) + "0" * 128


DEC_A = geometric(301, CHUNK, 0.2)
DEC_B = geometric(302, CHUNK, 0.4, 30)
DEC_C = whole_alphabet(303, CHUNK, 70)
DEC_T = geometric(304, 100, 0.3, 12)


@functools.lru_cache(maxsize=None)
def decoder_cases():
    A, B, C, T = (chunk_code(x)[0] for x in (DEC_A, DEC_B, DEC_C, DEC_T))
    hA, hB, hC, hT = (chunk_code(x)[1] for x in (DEC_A, DEC_B, DEC_C, DEC_T))
    szT = chunk_code(DEC_T)[2]
    assert szT < 256
    T300 = stop_long(T, hT, 300 - szT)                          # a 100-byte chunk that says 300 payload bytes, and holds them
    cs = []

    def add(name, parts, count, event, cut=None):
        s = "".join(parts)
        if cut is not None:
            s = s[:cut]
        b, n = pack(s)
        cs.append(DecCase(name, b, n, count, event))

    n3, n4 = 3 * CHUNK, 3 * CHUNK + 100
    add("stop_mid", [A, stop_long(B, hB), C], n3, ("STOP", 1))
    add("stop_short_mid", [A, stop_short(B, hB), C], n3, ("STOP", 1))
    add("stop_first", [stop_long(A, hA), B], 2 * CHUNK, ("STOP", 0))
    add("stop_last", [A, B, stop_long(T, hT)], 2 * CHUNK + 100, ("STOP", 2))
    add("skip_mid", [A, skip(B, hB), C], n3, ("SKIP", 1))
    add("skip_first", [skip(A, hA), B], 2 * CHUNK, ("SKIP", 0))
    add("skip_with_bad_header", [A, skip(bad_logmax(B, DEC_B), hB), C], n3, ("FAIL", 1))
    add("fail_empty_alphabet", [A, EMPTY_ALPHABET, C], n3, ("FAIL", 1))
    add("fail_logmax", [A, bad_logmax(B, DEC_B), C], n3, ("FAIL", 1))
    add("fail_sum_at_scale", [A, sum_at_scale(), C], n3, ("FAIL", 1))
    add("fail_cut_lr", [A, B], 2 * CHUNK, ("FAIL", 1), cut=len(A) + 2)
    add("fail_cut_masks", [A, B], 2 * CHUNK, ("FAIL", 1), cut=len(A) + 3 + 6 + 11)
    add("fail_cut_frequencies", [A, B], 2 * CHUNK, ("FAIL", 1), cut=len(A) + hB - 3)
    add("fail_cut_states", [A, B], 2 * CHUNK, ("FAIL", 1), cut=len(A) + hB + 16 + 70)
    add("fail_cut_payload", [A, B], 2 * CHUNK, ("FAIL", 1), cut=len(A) + len(B) - 9)
    add("fail_size_above_buffer", [set_size(A, hA, 2 * CHUNK + 1), B], 2 * CHUNK, ("FAIL", 0))
    add("fail_size_300_alone", [T300], 100, ("FAIL", 0))
    add("grown_buffer_takes_300", [A, T300], CHUNK + 100, ("STOP", 1))
    add("raw_cut", [bitstr(bytes(range(20)), 100)], 20, ("FAIL", 0))
    # two events in one block, in both orders: the lower chunk decides
    add("fail1_stop2_index", [A, EMPTY_ALPHABET, stop_long(C, hC), T], n4, ("FAIL", 1))
    add("fail1_stop2_chunk", [A, bad_logmax(B, DEC_B), stop_long(C, hC), T], n4, ("FAIL", 1))
    add("stop1_fail3_index", [A, stop_long(B, hB), C, EMPTY_ALPHABET], n4, ("STOP", 1))
    add("stop1_fail3_chunk", [A, stop_long(B, hB), C, bad_logmax(T, DEC_T)], n4, ("STOP", 1))
    add("stop1_skip2", [A, stop_long(B, hB), skip(C, hC), T], n4, ("STOP", 1))
    add("skip1_stop2", [A, skip(B, hB), stop_long(C, hC), T], n4, ("SKIP", 1))
    add("stop0_stop2", [stop_short(A, hA), B, stop_long(C, hC)], n3, ("STOP", 0))
    return cs


# ---- every lr the decoder accepts ------------------------------------------------------------------------------------------
LR_RANGE = tuple(range(8, 16))


@functools.lru_cache(maxsize=None)
def lr_inputs():
    return {"raw_limit_33": rnd(401, 33, 7, 97),
            "4099_over_40": whole_alphabet(402, 4099, 40),
            "chunk_and_37_over_256": whole_alphabet(403, CHUNK, 256) + rnd(404, 37),
            "three_chunks_skewed": geometric(405, 2 * CHUNK + 1000, 0.15, 100)}


@functools.lru_cache(maxsize=None)
def lr_stream(name, lr):
    """(bytes, bits) of the model's encoder at logRange lr (the device's and the oracle's encoders only write 12)"""
    return ans1model.encode(lr_inputs()[name], 0, lr=lr)


# ---- block streams (chain NONE, entropy ANS0) around a crafted entropy stream ---------------------------------------------------
def block_stream(count, bits, nbits):
    """EncodingTask.encodeBlock's frame for a block of `count` bytes (more than 15) whose one transform is NONE and whose entropy
    bits are given: mode byte, length, header checksum (CompressedOutputStream.java:866-905) -> (bytes, bits written)"""
    assert count > 15
    ds = 1 if count < 256 else ((count.bit_length() - 1) >> 3) + 1
    skip_flags = 0x7F                                            # the NONE transform "applies"
    mode = (((ds - 1) & 3) << 5) | (skip_flags >> 4)
    hsf = ((mode << 4) | 0x0F) & 0xFF
    written = 8 * (2 + ds) + nbits
    HASH = 0x1E35A7BD
    ck = (HASH * 0x01030507) & 0xFFFFFFFF
    for v in (mode, hsf, count, (written >> 32) & 0xFFFFFFFF, written & 0xFFFFFFFF):
        ck = katmodels._mix32(ck, HASH, v)
    ck = (ck >> 23) ^ (ck >> 3)
    return bytes([mode]) + count.to_bytes(ds, "big") + bytes([ck & 0xFF]) + bytes(bits), written


def small_event_blocks():
    """five single-chunk blocks of 33 .. 300 bytes with one crafted event each -> [(count, bits, nbits, kind)]"""
    out = []
    for i, (kind, n) in enumerate((("STOP", 150), ("SKIP", 222), ("FAIL", 64), ("FAIL", 299), ("FAIL", 97))):
        d = geometric(500 + i, n, 0.4, 9)
        s, hb, _ = chunk_code(d)
        if i == 0:
            s = stop_long(s, hb)
        elif i == 1:
            s = skip(s, hb)
        elif i == 2:
            s = EMPTY_ALPHABET + s[5:]
        elif i == 3:
            s = bad_logmax(s, d)
        else:
            s = s[:hb + 40]
        b, nb = pack(s)
        out.append((n, b, nb, kind))
    return out
