"""The deterministic case set of the device's inverse BWT (kanzi_amd/csrc/kz_bwt_inv.hip): framed BWT blocks chosen for what
its kernels do with them, not for what they hold.  tests/bwtinvmodel.py says what that is (parse verdict, grid, segment lengths,
splitters, chunk demand, stitched or fallback); tests/test_bwt_inverse_cases.py proves on the CPU that every seam named below is
reached; tests/test_gpu_bwt_inverse.py runs the set on the device against the oracle's inverse.

Seeded generators only; every forward transform is the oracle's.  A case is a frame (mode byte, primary indexes, payload) and,
where the frame is what an encoder writes for a text, that text.  Groups: "small" (up to 20 KB), "mid" (up to 300 KB) and
"large" (a megabyte; few, in tests of their own).

What the searches found, and what they did not:

 * One walker carries the block only when the text is P x R with R EQUAL to the grid spacing S (with R = 2 S there are two such
   walkers, and so on): the rows of period k are grid rows for one k in every S.  The rows below the primary index are shifted by
   one, so the grid periods are the first period for one part of the rotation classes and the last for the others, and the long
   walk covers n - 2 P bytes and a few gaps once P is large.
 * A block past the walk cap therefore needs (S - 2) P > 2^20: S = 128 and P >= 8323, that is n of 1 065 344 and more.  Such a
   block picks S = 128 by its own length.  The exact pair, a longest segment of cap + 1 links (stitched) and of cap + 2 (fallback):
   700 seeds of the period at P = 8321 gave cap - 2, cap - 1, cap and cap + 3 but neither member; with the period's first byte
   appended the longest walk is 126 P + 4 and up to 13 more, and at P = 8322 the seeds 1 and 2 give cap + 1 and cap + 2
   (PAIR_SEEDS; test_large_cases asserts both lengths).
 * Chunk pool: the least slack among periodic blocks whose walkers all stay short of the head is 13 chunks (63 x 64).  But a
   well-formed block CAN exceed the pool: when the text head sits on a grid row, the grid walker of that row and head 0 record
   the same bytes, and with a long segment behind that row the demand approaches 2 n / 128 against n / 128 + n / S.  126 x 128
   plus the period's first byte (n = 16129) asks for 47 chunks more than maxChunks; the block is marked suspect and decodes
   through the literal walkers: right bytes, at the fallback's speed.  It is in the set as `pool_overflow`.
 * Two paths cannot merge (every row is the link of at most one other row, see the model), so the issue's `two paths merge`
   damage does not exist; payload damage that moves heads into cycles stands in its place.

Measured on an MI355X (one block per call, kz_transform_inverse, whole call including copies): see LARGE_TIMES below.  All large
cases stay in the set: each takes under half a second."""
import dataclasses
import functools

import numpy as np

import bwtinvmodel as M
import oracle

# seconds per kz_transform_inverse call on one MI355X, host copies included.  A random block of the same size: 0.001.
# 2^20 dependent loads take 0.38 s, not the second the issue supposed; the literal walkers add 0.04 s.
LARGE_TIMES = {"neighbour_1051648": 0.001, "neighbour_1051649": 0.001, "stitched_long": 0.383, "past_cap": 0.424, "cap_plus_1": 0.381, "cap_plus_2": 0.421}

PAIR_P = 8322
PAIR_SEEDS = {1: 1, 2: 2}  # longest walk - cap -> seed of the period


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    frame: bytes
    text: object = None        # the text an encoder made the frame from; None: a frame no encoder writes
    group: str = "small"
    fallback: bool = False     # a well-formed block built to be finished by the literal walkers


def fwd(x):
    ok, f = oracle.transform_forward("BWT", bytes(x))
    assert ok
    return f


def rnd(seed, n, alpha=4):
    return np.random.default_rng(seed).integers(0, alpha, n, dtype=np.uint8).tobytes()


def split(frame):
    """-> (log2 of the index count, index size, stored indexes, payload)"""
    mode = frame[0]
    logc, ps = (mode >> 2) & 7, (mode & 3) + 1
    c = 1 << logc
    return logc, ps, [int.from_bytes(frame[1 + i * ps:1 + (i + 1) * ps], "big") for i in range(c)], frame[1 + c * ps:]


def join(logc, ps, stored, payload):
    return bytes([(logc << 2) | (ps - 1)]) + b"".join((v & ((1 << (8 * ps)) - 1)).to_bytes(ps, "big") for v in stored) + bytes(payload)


def periodic(P, R, seed=None, tail=0, alpha=256):
    rng = np.random.default_rng(P * 1000 + R if seed is None else seed)
    per = rng.integers(0, alpha, P, dtype=np.uint8)
    return np.concatenate([np.tile(per, R), rng.integers(0, alpha, tail, dtype=np.uint8)]).tobytes()


def _find(what, texts, pred, maxN=None):
    """the first text of a seeded sequence whose plan satisfies pred"""
    for label, x in texts:
        f = fwd(x)
        if pred(M.plan(f, maxN, want_bytes=False)):
            return label, x, f
    raise AssertionError("no case found for " + what)


def _has_segment(L):
    return lambda p: p.path == "stitched" and bool((p.seg_len[:p.G + 1] == L).any())


LENGTH_SEAMS = (0, 1, 2, 3, 254, 255, 256, 257, 263, 264, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193)
SEGMENT_LENGTHS = (7, 8, 9, 127, 128, 129, 256)
G_SEAMS = (960, 1088, 2048, 2049)                     # G = 15, 17 (16 is n = 1024), 32 and 33
NSP_SEAMS = ((255, 3952 * 64), (256, 3968 * 64), (257, 3968 * 64 + 1))


@functools.lru_cache(maxsize=None)
def cases():
    cs = []

    def add(name, frame, text=None, **kw):
        assert all(c.name != name for c in cs), name
        cs.append(Case(name, bytes(frame), None if text is None else bytes(text), **kw))

    def well(name, x, **kw):
        add(name, fwd(x), x, **kw)

    # ---- length seams ----
    for n in LENGTH_SEAMS:
        x = rnd(1000 + n, n, 7)
        if n == 0:
            add("len_0", b"", b"")
        elif n == 1:
            add("len_1", join(0, 1, [0], x), x)                   # (the forward declines one byte; the inverse takes the frame)
        else:
            well("len_%d" % n, x)
    well("len_70000_header_25", rnd(5, 70000, 16), group="mid")
    # ---- header forms ----
    x = rnd(11, 300)
    logc, ps, st, pay = split(fwd(x))
    for w in range(ps, 5):
        add("wide_index_%d_n300" % w, join(3, w, st, pay), x)
    x = rnd(12, 200)
    logc, ps, st, pay = split(fwd(x))
    assert (logc, ps) == (0, 1)
    for w in (2, 3, 4):
        add("wide_index_%d_n200" % w, join(0, w, st, pay), x)
    add("one_index_n300", join(0, 2, [5], split(fwd(rnd(11, 300)))[3]))
    add("eight_indexes_n200", join(3, 1, [5, 30, 60, 90, 120, 150, 180, 199], split(fwd(rnd(12, 200)))[3]))
    for lg in (4, 5, 6, 7):
        add("log_chunks_%d" % lg, bytes([lg << 2]) + rnd(20 + lg, (1 << lg) + 300))
        add("log_chunks_%d_short" % lg, bytes([lg << 2]) + rnd(30 + lg, 9))
    add("header_minus_1_one_index", bytes([0x01, 0x00]))
    add("header_minus_1_eight", bytes([0x0C | 0x01]) + bytes(15))
    for w in (1, 2, 3, 4):
        add("header_only_%d" % w, bytes([w - 1]) + bytes(w), b"")
    add("header_only_eight", bytes([0x0C]) + bytes(8))
    add("index_7fffffff_n200", join(0, 4, [0x7FFFFFFF], rnd(12, 200)))
    add("index_7ffffffe_n200", join(0, 4, [0x7FFFFFFE], rnd(12, 200)))
    x = rnd(11, 300)
    logc, ps, st, pay = split(fwd(x))
    add("index_7fffffff_k3_n300", join(3, 4, st[:3] + [0x7FFFFFFF] + st[4:], pay))
    # ---- scatter ----
    n = 5000
    uni = fwd(b"a" * n)
    add("one_symbol", uni, b"a" * n)
    logc, ps, st, pay = split(uni)
    for label, at in (("lane0", 64 * 3), ("lane63", 64 * 3 + 63), ("wave1", 1024), ("last", n - 1), ("first", 0)):
        q = bytearray(pay)
        q[at] = ord("b")
        add("one_symbol_foreign_" + label, join(logc, ps, st, q))
    add("distinct_in_every_row", join(logc, ps, st, bytes((37 * i) & 0xFF for i in range(n))))
    q = bytearray(rnd(40, 4096 + 100, 4))
    q[-1] = 0xEE
    add("symbol_in_last_partial_row_only", join(3, 2, [17, 600, 1200, 1800, 2400, 3000, 3600, 4100], q))
    x = bytearray(rnd(41, 4096 + 100, 4))
    x[-3] = 0xEE                                                  # its BWT byte lands in the last rows of the last tile or not: the model says
    well("rare_symbol_text", x)
    # ---- walk and chunks ----
    seeds = [("seed %d" % s, rnd(s, 1500)) for s in range(400)]
    for L in SEGMENT_LENGTHS:
        pool = seeds if L < 200 else [("seed %d" % s, rnd(s, 6000)) for s in range(400)]
        label, x, f = _find("segment of %d" % L, pool, _has_segment(L))
        add("segment_%d" % L, f, x)
    label, x, f = _find("head on the grid", seeds, lambda p: (p.prim[0] - 1) % p.S == 0)
    add("head_on_grid", f, x)
    label, x, f = _find("END by a grid walker's first step", seeds, lambda p: bool((p.start_link[:p.G] == M.END).any()))
    add("end_at_first_step", f, x)
    label, x, f = _find("row 0 a grid row's target", seeds, lambda p: bool((p.start_link[:p.G] == 0).any()))
    add("row0_is_grid_target", f, x)
    # ---- one walker carries the block ----
    for P, R in ((65, 64), (63, 64), (130, 64)):
        well("periodic_%dx%d" % (P, R), periodic(P, R))
    for P, R in ((65, 128), (66, 128)):
        well("periodic_%dx%d_s128" % (P, R), periodic(P, R))       # S = 128 only beside a neighbour of 1 051 649 bytes
    well("periodic_62x64_tail1_head_on_grid", periodic(62, 64, tail=1))
    # ---- pool at its bound ----
    per = np.random.default_rng(126 * 1000 + 128).integers(0, 256, 126, dtype=np.uint8)
    well("pool_overflow", np.tile(per, 129)[:126 * 128 + 1].tobytes(), fallback=True)
    # ---- resolve ----
    for n in G_SEAMS:
        well("grid_%d" % n, rnd(2000 + n, n, 5))
    for nsp, n in NSP_SEAMS:
        well("splitters_%d" % nsp, rnd(3000 + nsp, n, 6), group="mid")
    well("ramp_up", np.repeat(np.arange(256, dtype=np.uint8), 16).tobytes())
    well("ramp_down", np.repeat(np.arange(255, -1, -1, dtype=np.uint8), 16).tobytes())
    # ---- targeted damage ----
    x = rnd(77, 4200, 4)
    base = fwd(x)
    add("damage_base", base, x)
    logc, ps, st, pay = split(base)
    n = len(pay)
    for k in range(1, 8):
        add("index_%d_moved" % k, join(logc, ps, st[:k] + [(st[k] + 100 + k) % n] + st[k + 1:], pay))
    sw = list(st)
    sw[2], sw[5] = sw[5], sw[2]
    add("indexes_2_5_swapped", join(logc, ps, sw, pay))
    add("index_0_moved", join(logc, ps, [(st[0] + 1) % n] + st[1:], pay))
    add("index_0_last_row", join(logc, ps, [n - 1] + st[1:], pay))
    add("index_0_is_n", join(logc, ps, [n] + st[1:], pay))
    add("index_3_last_row", join(logc, ps, st[:3] + [n - 1] + st[4:], pay))
    add("index_3_is_n", join(logc, ps, st[:3] + [n] + st[4:], pay))
    add("index_3_is_n_plus_1", join(logc, ps, st[:3] + [n + 1] + st[4:], pay))
    for at in (0, 1, 2099, n - 1):
        q = bytearray(pay)
        q[at] ^= 1
        add("payload_byte_%d_changed" % at, join(logc, ps, st, q))
    add("cycle_without_splitter", _cycle_without_splitter(logc, ps, st, pay))
    add("last_byte_cut", base[:-1])
    x = rnd(78, 200, 4)
    f = fwd(x)
    add("small_index_moved", join(0, 1, [(split(f)[2][0] + 7) % 200], split(f)[3]))      # the 0xFF link behind row 0 is past the table
    add("small_last_byte_cut", f[:-1])
    return tuple(cs)


def _cycle_without_splitter(logc, ps, st, pay):
    """one payload byte changed so that a head among 1..7 lies on a cycle that holds grid rows but no splitter: the only way into the
    `steps > M` guard of k_bwti_resolve.  Bounded, deterministic search."""
    rng = np.random.default_rng(4242)
    for _ in range(3000):
        at = int(rng.integers(0, len(pay)))
        q = bytearray(pay)
        q[at] = (q[at] + 1 + int(rng.integers(0, 3))) & 3
        f = join(logc, ps, st, q)
        if M.plan(f, want_bytes=False).cycle_guard:
            return f
    raise AssertionError("no cycle without a splitter found")


def neighbour(size):
    """a well-formed block whose FRAME has exactly `size` bytes (header of 25): it sets the grid spacing of its batch"""
    x = rnd(size, size - 25, 16)
    f = fwd(x)
    assert len(f) == size
    return Case("neighbour_%d" % size, f, x, "large")


@functools.lru_cache(maxsize=None)
def large_cases():
    """blocks of a megabyte.  stitched_long: S = 128, the longest segment in (cap / 2, cap].  past_cap: the longest segment beyond
    cap + 1, a block an encoder made that the literal walkers finish.  cap_plus_1 / cap_plus_2: the exact pair, when PAIR_SEEDS
    holds the seeds the search found."""
    cs = [neighbour(1051648), neighbour(1051649)]
    x = periodic(8220, 128)
    cs.append(Case("stitched_long", fwd(x), x, "large"))
    x = periodic(8340, 128)
    cs.append(Case("past_cap", fwd(x), x, "large", True))
    for d, seed in sorted(PAIR_SEEDS.items()):
        x = periodic(PAIR_P, 129, seed=PAIR_P * 1000 + seed)[:PAIR_P * 128 + 1]
        cs.append(Case("cap_plus_%d" % d, fwd(x), x, "large", d == 2))
    return tuple(cs)


def by_name(name):
    for c in cases() + (large_cases() if name.startswith(("neighbour_", "stitched_long", "past_cap", "cap_plus_")) else ()):
        if c.name == name:
            return c
    raise KeyError(name)


EMPTY = Case("empty", b"", b"")


@functools.lru_cache(maxsize=None)
def batches():
    """name -> blocks of one kz_decode_blocks call.  Zero-length blocks stand in front of, between and behind the others, so the
    dense scratch index of a block is not its batch index."""
    small = [c for c in cases() if c.group == "small" and len(c.frame) > 0]
    mid = [c for c in cases() if c.group == "mid"]
    out = {}
    mixed = []
    for i, c in enumerate(small):
        if i % 9 == 0:
            mixed.append(EMPTY)
        mixed.append(c)
    out["small"] = tuple([EMPTY, EMPTY] + mixed + [EMPTY])
    out["small_reversed"] = tuple(reversed(out["small"]))
    out["mid"] = tuple([EMPTY] + mid[:2] + [EMPTY] + small[::7] + [EMPTY, EMPTY] + mid[2:] + [EMPTY])
    s128 = [c for c in small if c.name.startswith(("periodic_", "segment_", "head_on_grid", "index_", "len_4097", "pool_overflow", "cycle_"))]
    for size in (1051648, 1051649):
        out["beside_%d" % size] = tuple([EMPTY] + s128[:len(s128) // 2] + [neighbour(size)] + s128[len(s128) // 2:])
    x = [rnd(9000 + i, 300 - (i % 3), 4) for i in range(50)]
    many = [Case("many_%d" % i, fwd(t), t) for i, t in enumerate(x)]
    out["many"] = tuple(many[i % 50] for i in range(2000))
    return out


# ---- the block stream of a frame (entropy NONE): EncodingTask.encodeBlock's header around a transformed payload ----
def _mix32(ck, value):
    ck ^= (0x1E35A7BD * (~value & 0xFFFFFFFF)) & 0xFFFFFFFF
    ck = ((ck << 13) | (ck >> 19)) & 0xFFFFFFFF
    return (ck * 5 + 0x52DCE729) & 0xFFFFFFFF


def block_stream(frame):
    """the bits of one block of a `BWT & NONE` stream whose BWT stage put out `frame`: mode byte (transformed copy, BWT applied), the
    post-transform length, the header's check byte, the frame.  -> (bytes, bit count).  Written from the block layout of
    CompressedOutputStream.java:866-985; test_bwt_inverse_cases.py holds it against the oracle's encoder and decoder."""
    post = len(frame)
    assert post > 0
    size = 1 if post < 256 else ((post.bit_length() - 1) >> 3) + 1
    mode = 0x80 | 0x10 | ((size - 1) << 5) | 0x07
    written = 8 * (2 + size + post)
    ck = (0x1E35A7BD * 0x01030507) & 0xFFFFFFFF
    for v in (mode, ((mode << 4) | 0x0F) & 0xFF, post, (written >> 32) & 0xFFFFFFFF, written & 0xFFFFFFFF):
        ck = _mix32(ck, v)
    ck = (ck >> 23) ^ (ck >> 3)
    return bytes([mode]) + post.to_bytes(size, "big") + bytes([ck & 0xFF]) + bytes(frame), written
