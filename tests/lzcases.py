"""The deterministic case set of the device LZ / LZX parse (kanzi_amd/csrc/kz_lz.hip): small blocks built from parts to land on the
seams of k_lz_fwd's shortcuts (literal batch, early table reads of the lazy probes, 8-byte backward extension, 64-lane findMatch, the
two hash-fill forms, the frame's length and distance edges, the window switch) and of k_lz_inv (periodic / chunked copy, the 64-byte
register windows, readLength at the block end).  No GPU import: tests/test_lz_cases.py proves on the CPU, with the trace of
katmodels.lz_forward / lz_decode, that every case reaches what it was built for; tests/test_gpu_lz.py runs the set on the device.

Events (counted by katmodels.lz_forward(events=) unless they begin with inv_, which katmodels.lz_decode(events=) counts):
  lit_step_1 / _2 / _3plus      a literal step that advances by 1, 2, 3 or more (1 + (srcInc >> 6))
  lit_run_cross_64 / _128       srcInc reaches 64 / 128 within one literal run
  lit_peer_equal / _differs     a step with srcInc >= 2 whose table entry was stored by a step of the same run (itself at srcInc >= 2:
                                both sit in literal batches of k_lz_fwd) fewer than 64 steps earlier; its 4 bytes equal ours / differ
  lit_end_rep0 / _rep1 / _table / _srcend   what ends a literal run that has reached srcInc >= 2
  lazy_h1_eq_h0, lazy_h2_eq_h1, lazy_h2_eq_h0 (h2 != h1)   the lazy probes' slots coincide with slots stored earlier in the same step
  lazy_*_win                    ... and the probe wins with the position stored earlier in the same step as its candidate
  lazy_p1_win / lazy_p2_win     the +1 / +2 probe wins with a candidate from before the step
  bwd_len_0 / 1_7 / 8 / 9_15 / 16 / 17plus   total backward extension of a table match
  bwd_stop_byte / _anchor / _minref          the one bound that stopped it while the other two would have let it go on
                                (_minref: with minRef > 0, the window's edge; bwd_stop_block_start: ref reached 0)
  bwd_end_ref_lt8               it ended with ref < 8 (bwd_end_ref_lt8_after_8: after 9 bytes or more, so both forms of the loop ran)
  bwd_clamp                     best > MAX_MATCH after the extension
  rep_found_ext_back / _no_ext  a repeat match found at srcIdx + 1, extended one byte back or not;  rep_max_match: best >= MAX_MATCH there
  fm_0_3, fm_4_7, fm_8, fm_504_519, fm_1016_1031   a findMatch result;  fm_cut_mod<k>: it ran into maxMatch (result = maxMatch & ~7 >= 8)
                                with maxMatch % 8 == k
  dist_1, 2_63, 64, 65_255, 255, 256, 65533, 65535, 65536, gt_65536   the distance of a new-distance token
  reject_minref                 a table candidate with 4 equal bytes refused because ref == minRef;  win_flag_0 / _1: the window flag
  mlen_rep_<v> / mlen_new_<v>   the match-length code mLen - threshold (3 for repeat tokens, 7 for new distances) is v
  lit_loop_<v> / lit_final_<v>  the literal length of an in-loop token / of the final token is v
  nfill_<n>                     positions the hash fill covers (0, 1, 16, 17, 63, 64, 65, 129plus, other);  fill_dup_hash: two positions of one
                                64-position round of the fill share a slot
  applied, declined_ge_count, declined_1pct, count_lt_24   how the block ends
  inv_copy_near / far _ short / long   dist < 64 / >= 64 with mLen <= 64 / > 64
  inv_dist2_straddle64 / inv_dist3_straddle64   a 2- / 3-byte distance whose bytes lie on both sides of a multiple of 64 of its stream
  inv_token_idx_mult64          a token read at a multiple of 64 of the token stream
  inv_lit_code_3byte / _4byte, inv_mlen_code_3byte / _4byte   the long forms of readLength in the two streams

Not in the set: the reference's fixed token buffer (max(count / 5, 256) tokens; one more ends the block with ERR_PROCESS_BLOCK, the
device's d_flag = -1).  Every token covers at least minMatch bytes and all but the 4-byte matches that a hash collision yields cover 5
or more, so a block that overflows it must consist almost entirely of such matches; no short construction is known."""
import collections
import functools

import numpy as np

MAX_MATCH = 65535 + 254 + 4
M64 = (1 << 64) - 1
SEED = 0x1E35A7BD

Case = collections.namedtuple("Case", "name data codecs dtype events")    # codecs: tuple of "LZ" / "LZX"; dtype: "UNDEFINED" / "DNA"
BOTH = ("LZ", "LZX")

# Events of the issue's list that the format's own arithmetic rules out, at most three entries: class -> (event names, why).
# tests/test_lz_cases.py asserts the inequalities and that none of these events ever occurs.
UNREACHED = {
    "a match beyond MAX_MATCH's reach": (
        ("rep_max_match", "mlen_rep_65789", "mlen_rep_65790", "mlen_new_65789", "mlen_new_65790"),
        "findMatch returns at most maxMatch & ~7 = 65792 < MAX_MATCH = 65793, so a repeat match at srcIdx + 1 never has best >= MAX_MATCH "
        "(only the backward extension of a table match passes it, and is clamped); and a token's length code is at most MAX_MATCH - "
        "minMatch - threshold = 65786 (repeat) / 65782 (new distance), below 65789: the match-length stream never holds a 4-byte code"),
    "a final literal run under 18": (
        ("lit_final_6", "lit_final_7"),
        "every match ends at or before srcEnd = count - 18, so the final token carries at least 18 literals: its short form is dead code"),
    "a hash fill under 3": (
        ("nfill_0", "nfill_1"),
        "the fill covers bestLen - 1 positions and bestLen >= minMatch >= 4"),
}

FORWARD_EVENTS = (
    "lit_step_1 lit_step_2 lit_step_3plus lit_run_cross_64 lit_run_cross_128 lit_peer_equal lit_peer_differs "
    "lit_end_rep0 lit_end_rep1 lit_end_table lit_end_srcend "
    "lazy_h1_eq_h0 lazy_h1_eq_h0_win lazy_p1_win "
    "bwd_len_0 bwd_len_1_7 bwd_len_8 bwd_len_9_15 bwd_len_16 bwd_len_17plus bwd_stop_byte bwd_stop_anchor bwd_stop_minref bwd_end_ref_lt8 bwd_clamp "
    "rep_found_ext_back rep_found_no_ext rep_max_match "
    "fm_0_3 fm_4_7 fm_8 fm_504_519 fm_1016_1031 fm_cut_mod0 fm_cut_mod1 fm_cut_mod2 fm_cut_mod3 fm_cut_mod4 fm_cut_mod5 fm_cut_mod6 fm_cut_mod7 "
    "dist_1 dist_2_63 dist_64 dist_65_255 dist_255 dist_256 dist_65533 dist_65535 dist_65536 dist_gt_65536 reject_minref win_flag_0 win_flag_1 "
    "mlen_rep_252 mlen_rep_253 mlen_rep_254 mlen_rep_65789 mlen_rep_65790 mlen_new_252 mlen_new_253 mlen_new_254 mlen_new_65789 mlen_new_65790 "
    "lit_loop_6 lit_loop_7 lit_loop_260 lit_loop_261 lit_loop_65796 lit_loop_65797 "
    "lit_final_6 lit_final_7 lit_final_260 lit_final_261 lit_final_65796 lit_final_65797 "
    "nfill_0 nfill_1 nfill_16 nfill_17 nfill_63 nfill_64 nfill_65 nfill_129plus fill_dup_hash applied").split()
LZX_ONLY_EVENTS = "lazy_h2_eq_h1 lazy_h2_eq_h1_win lazy_h2_eq_h0 lazy_h2_eq_h0_win lazy_p2_win".split()
OUTCOME_EVENTS = "declined_ge_count declined_1pct count_lt_24".split()      # reached by cases that are, by definition, not applied
BIG_ONLY_EVENTS = "dist_65535 dist_65536 dist_gt_65536 win_flag_1".split()  # exist from count 262154 on
# the decoder's events, over the oracle's frames of the applied cases; a 4-byte code in the match-length stream is in no frame a
# forward pass writes (UNREACHED, first entry): recoded_frame() supplies one
INVERSE_EVENTS = ("inv_copy_near_short inv_copy_near_long inv_copy_far_short inv_copy_far_long inv_dist2_straddle64 inv_dist3_straddle64 "
                  "inv_token_idx_mult64 inv_lit_code_3byte inv_lit_code_4byte inv_mlen_code_3byte").split()


# ---- parts ---------------------------------------------------------------------------------------------------------------------
def hash5(a, log):
    """the parse's hash (K/transform/LZCodec.java:904-911) of rows of 5 bytes -> slots of a 2^log table"""
    a = np.asarray(a, dtype=np.uint64)
    v = a[:, 0] | (a[:, 1] << np.uint64(8)) | (a[:, 2] << np.uint64(16)) | (a[:, 3] << np.uint64(24)) | (a[:, 4] << np.uint64(32))
    return ((v << np.uint64(24)) * np.uint64(SEED)) >> np.uint64(64 - log)


@functools.lru_cache(maxsize=None)
def colliding_pair(log, seed=1):
    """two 5-byte strings of letters that share a slot of the 2^log table and differ in their first four bytes"""
    a = np.random.default_rng(seed).integers(0x61, 0x7B, (1 << (log // 2 + 4), 5), dtype=np.uint8)
    hv = hash5(a, log)
    order = np.argsort(hv, kind="stable")
    same = np.flatnonzero(hv[order][1:] == hv[order][:-1])
    for k in same:
        x, y = a[order[k]].tobytes(), a[order[k + 1]].tobytes()
        if x[:4] != y[:4] and x[0] != y[0]:
            return x, y
    raise AssertionError("no pair")


@functools.lru_cache(maxsize=None)
def self_colliding(log, shift, seed=2):
    """5 + shift letters whose first five and last five bytes share a slot (shift 1: h1 == h0, shift 2: h2 == h0) and are no period"""
    a = np.random.default_rng(seed).integers(0x61, 0x7B, (1 << (log + 3), 5 + shift), dtype=np.uint8)
    hit = np.flatnonzero((hash5(a[:, :5], log) == hash5(a[:, shift:], log)) & (a[:, 0] != a[:, shift]))
    for k in hit:
        s = a[k].tobytes()
        if shift == 1 or hash5(a[k:k + 1, 1:6], log)[0] != hash5(a[k:k + 1, :5], log)[0]:
            return s
    raise AssertionError("no string")


class Build:
    """a block grown from parts; every part draws from the case's own generator"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.b = bytearray()
        self.fresh = iter(range(0x80, 0x100))                   # byte values kept for resets: random parts use 0x00..0x7F only

    def __len__(self):
        return len(self.b)

    def rnd(self, n, first_not=None):
        """n random bytes below 0x80 (to drive the skip step, or as a word to plant)"""
        w = bytearray(self.rng.integers(0, 0x80, n, dtype=np.uint8).tobytes())
        if n and first_not is not None and w[0] == first_not:
            w[0] ^= 1
        return bytes(w)

    def add(self, part):
        self.b += part
        return len(self.b) - len(part)                          # where it went

    def reset(self, n=12):
        """a run of a byte value used nowhere else: wherever the parse stands, two visited positions of the run match, the match ends
        at the run's end, and the next step starts there with srcInc = 0 and anchor = srcIdx (n >= 3 steps + 8)"""
        return self.add(bytes([next(self.fresh)]) * n)

    def copy(self, src, n):
        """n bytes again from position src (overlapping allowed)"""
        at = len(self.b)
        for i in range(n):
            self.b.append(self.b[src + i])
        return at

    def pad_to(self, n, value=None):
        """fill up to n bytes: with a run of `value`, or with random bytes"""
        k = n - len(self.b)
        assert k >= 0, (n, len(self.b))
        return self.add(bytes([value]) * k if value is not None else self.rnd(k))

    def bytes(self):
        return bytes(self.b)


def visited(e, upto):
    """the positions a literal run that starts at e with srcInc = 0 visits (and stores), up to `upto`: each step advances by
    1 + (srcInc >> 6)"""
    out, p, inc = [], e, 0
    while p <= upto:
        out.append(p)
        p += 1 + (inc >> 6)
        inc += 1
    return out


def plant_in_run(b, e, lit_len, j, dist=None, near=None, wlen=8, exact=False):
    """b holds a literal run that began at e (srcInc = 0 there) and is to go on with random bytes; a word W of j + wlen bytes is
    written so that the run's first visited position inside its second copy W' is W'[j] and the table holds W[j] for it: the parse
    finds the match j bytes late and extends it backwards.  W' starts about lit_len bytes behind e (exact: just there, with the least
    j' >= j that serves).  W goes where a visited position of the early run serves, at least `near` bytes behind e; or, with dist
    given, W' lies dist behind W, and W in the run's first 64 positions (all visited).  Fills b up to the end of W'; returns (start of
    W, start of W', j)."""
    vis = visited(e, e + lit_len + 400)
    prev = {v: u for u, v in zip(vis, vis[1:])}
    first = lambda v, k: v in prev and prev[v] < v - k           # v is the first visited position of a word that starts k in front of it
    if exact:
        j = next(k for k in range(j, 64) if first(e + lit_len + k, k))
        vt = e + lit_len + j
    elif dist is None:
        vt = next(v for v in vis if v - j >= e + lit_len and first(v, j))
    else:
        vt = next(v for v in vis if v - j >= e + lit_len and first(v, j) and j <= v - dist - e <= 63 - wlen)
    vs = vt - dist if dist is not None else next(v for v in vis if v - j >= e + near)
    ws, wt = vs - j, vt - j
    assert e <= ws and len(b) <= ws and ws + j + wlen <= wt, (e, len(b), ws, wt)
    b.pad_to(ws)
    w = b.rnd(j + wlen)
    b.add(w)
    b.pad_to(wt)
    if b.b[wt - 1] == b.b[ws - 1]:
        b.b[wt - 1] ^= 1                                          # the byte in front differs: the extension stops at W'
    b.add(w)
    return ws, wt, j


def _c(name, b, common, lz=(), lzx=(), codecs=BOTH, dtype="UNDEFINED"):
    common = set(common.split()) if isinstance(common, str) else set(common)
    ev = {"LZ": common | set(lz), "LZX": common | set(lzx)}
    return Case(name, b.bytes() if isinstance(b, Build) else bytes(b), tuple(codecs), dtype, {k: frozenset(v) for k, v in ev.items() if k in codecs})


def _tail(b, zeros=300, rnd=30):
    """a run that pays for the literals (the block applies) and a random end (the last literal run meets srcEnd)"""
    b.add(bytes(zeros))
    b.add(b.rnd(rnd))


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _skip_steps():
    b = Build(101)
    b.add(b.rnd(700))
    b.reset(40)
    b.add(b.rnd(40))
    _tail(b, 400)
    return _c("skip steps 1, 2, 3+", b, "lit_step_1 lit_step_2 lit_step_3plus lit_run_cross_64 lit_run_cross_128 lit_end_table lit_end_srcend applied")


def _peers(codec):
    log = 16 if codec == "LZ" else 19
    x, y = colliding_pair(log)
    b = Build(102 + log)
    b.reset()
    at = b.add(b.rnd(64))
    b.b[at + 10:at + 15] = x                                     # two positions of one batch share a slot, their bytes differ
    b.b[at + 30:at + 35] = y
    b.reset()
    at = b.add(b.rnd(64))
    b.b[at + 30:at + 35] = b.b[at + 10:at + 15]                  # ... and here they are equal: the run ends on a store of its own batch
    _tail(b)
    return _c("same slot inside a literal batch, " + codec, b, "lit_peer_differs lit_peer_equal lit_end_table fm_4_7 applied", codecs=(codec,))


def _rep_ends():
    b = Build(103)
    b.reset()
    a = b.add(b.rnd(16))
    b.add(b.rnd(5))
    bb = b.add(b.rnd(16))
    z = b.reset()
    b2 = b.copy(bb, 16)                                          # new distance dB
    assert z == bb + 16
    a2 = b.copy(a, 16)                                           # new distance dA, found at the anchor
    d_b, d_a = b2 - bb, a2 - a
    b.copy(len(b) - d_b, 12)                                     # goes on at distance dB (the run's bytes): repeat match at srcIdx + 1, one byte back
    b.add(b.rnd(6, first_not=b.b[len(b) - d_a]))
    b.copy(len(b) - d_a, 12)                                     # a literal run, then the second repeat candidate
    b.add(b.rnd(6, first_not=b.b[len(b) - d_a]))
    b.copy(len(b) - d_a, 12)                                     # ... and the first
    _tail(b)
    return _c("literal runs ended by the repeat candidates", b, "rep_found_ext_back rep_found_no_ext lit_end_rep0 lit_end_rep1 applied")


def _lazy_runs():
    b = Build(104)
    b.reset()
    sep = lambda: b.rnd(10) + b.rnd(3) * 5 + b.rnd(2) + b.rnd(5) * 3 + b.rnd(2) + b"Z"    # two tokens: the repeat distances are 5 and 3 behind it
    b.add(b"Q" + b"a" * 20 + b"Y" + sep() + b"a" * 40 + b.rnd(8))          # h1 == h0: the second run's +1 probe finds the step's own store
    b.add(b"bccccc" + b"Y" + sep() + b"b" + b"c" * 30 + b.rnd(8))            # h2 == h1
    b.add(b"dedede" + b"Y" + sep() + b"de" * 20 + b.rnd(8))                  # h2 == h0
    _tail(b)
    return _c("lazy probes meet the step's own stores (runs, period 2)", b, "lazy_h1_eq_h0 lazy_h1_eq_h0_win dist_1 applied",
              lzx="lazy_h2_eq_h1 lazy_h2_eq_h1_win lazy_h2_eq_h0 lazy_h2_eq_h0_win".split())


def _lazy_collide(codec):
    log = 16 if codec == "LZ" else 19
    b = Build(105 + log)
    words = [self_colliding(log, 1) + b.rnd(8)] + ([self_colliding(log, 2) + b.rnd(8)] if codec == "LZX" else [])
    # such a word's second slot-mate would overwrite the first: its first copy lies where the literal run visits w[0] and skips
    # w[1] (steps of 2) or w[2] (steps of 3)
    e = b.reset() + 12
    for w, at in zip(words, (e + 70, e + 204)):
        assert at in visited(e, at) and at + len(w) - 5 not in visited(e, at + 8)
        b.pad_to(at)
        b.add(w)
    b.add(b.rnd(5))
    for w in words:
        b.reset(30)
        b.add(w)
    # plain wins: the match at p is 5 long, the one at p + 1 (p + 2) is longer and comes from elsewhere
    for k in (1, 2):
        u = b.rnd(14)
        b.reset()
        b.add(u[:5] + b.rnd(3, first_not=u[5]) + u[k:] + b.rnd(3))
        b.reset()
        b.add(u)
    _tail(b)
    return _c("lazy probes: colliding slots, plain wins, " + codec, b, "lazy_h1_eq_h0 lazy_p1_win applied", lzx="lazy_h2_eq_h0 lazy_p2_win".split(), codecs=(codec,))


def _bwd_lengths():
    b = Build(106)
    b.add(b.rnd(2))
    plant_in_run(b, 0, 5200, 12, near=2)                         # W at 2: the extension ends with ref = 2, its first round took 8 bytes
    for j, run in ((8, 2500), (16, 9000), (3, 400), (0, 30)):
        e = b.reset(60) + 60
        plant_in_run(b, e, run, j, near=8)
    _tail(b, 600)
    return _c("backward extension of 12, 8, 16, 3 and 0 bytes", b, "bwd_len_0 bwd_len_1_7 bwd_len_8 bwd_len_9_15 bwd_len_16 bwd_stop_byte bwd_end_ref_lt8 "
              "bwd_end_ref_lt8_after_8 applied")


def _bwd_anchor():
    b = Build(107)
    b.reset()
    z = next(b.fresh)
    w = b.rnd(12)
    b.add(b.rnd(4) + bytes([z]) + w + b.rnd(6))
    b.add(bytes([z]) * 12 + w)                                   # a run of the byte in front of W ends where W' begins: anchor = srcIdx
    _tail(b)
    return _c("backward extension held by the anchor", b, "bwd_stop_anchor bwd_len_0 applied")


def _fm_lengths():
    b = Build(108)
    b.reset()
    words = [(b.rnd(n + 1), n) for n in (8, 510, 1020)]
    for w, n in words:
        b.add(w)
    for w, n in words:
        b.reset(100)
        b.add(w[:n] + bytes([w[n] ^ 1]))
    _tail(b)
    return _c("findMatch results 8, 510, 1020", b, "fm_8 fm_504_519 fm_1016_1031 applied")


def _fm_cut(k):
    b = Build(109 + k)
    b.reset()
    w = b.add(b.rnd(64))
    at = b.reset()
    n = 120 + k                                                  # maxMatch = srcEnd - srcIdx = n - 18
    b.copy(w, n)
    assert (len(b) - 18 - (at + 12)) % 8 == (n - 18) % 8
    return _c("match cut by srcEnd, maxMatch %% 8 = %d" % ((n - 18) % 8), b, ["fm_cut_mod%d" % ((n - 18) % 8), "applied"])


def _fm_short():
    b = Build(120)
    b.reset()
    w = b.rnd(5)
    b.add(w + b.rnd(20))
    b.add(bytes(200))
    b.reset()
    b.add(b.rnd(10) + w + b.rnd(18))                             # 5 bytes again, 5 positions in front of srcEnd: maxMatch 5, result 0
    return _c("a candidate under srcEnd: maxMatch below 8", b, "fm_0_3 applied")


def _distances():
    b = Build(121)
    for d in (20, 64, 65, 255, 256):
        b.reset()
        w = b.rnd(16)
        if d < 64:                                               # the first 64 positions of a literal run are all visited
            b.add(w + b.rnd(d - 16) + w)
            continue
        b.add(w + b.rnd(d - 16 - 12))
        b.reset()
        b.add(w)
    _tail(b)
    return _c("distances 20, 64, 65, 255, 256", b, "dist_1 dist_2_63 dist_64 dist_65_255 dist_255 dist_256 applied")


def _mlen_codes():
    b = Build(122)
    b.reset()
    words = [b.rnd(300) for _ in range(3)]
    long = b.rnd(830)
    for w in words:
        b.add(w)
    lw = b.add(long)
    for w, n in zip(words, (263, 264, 265)):                    # new distance: length 4 + 7 + 252 / 253 / 254
        b.reset(100)
        b.add(w[:n] + bytes([w[n] ^ 1]))
    b.reset(100)
    t = b.copy(lw, 30)
    d = t - lw
    for n in (259, 260, 261):                                    # repeat distance: one differing byte, then 4 + 3 + 252 / 253 / 254 more
        b.add(bytes([b.b[len(b) - d] ^ 1]))
        b.copy(len(b) - d, n)
    b.add(bytes([b.b[len(b) - d] ^ 1]))
    _tail(b)
    return _c("match-length codes 252, 253, 254", b, "mlen_new_252 mlen_new_253 mlen_new_254 mlen_rep_252 mlen_rep_253 mlen_rep_254 rep_found_no_ext applied")


def _nfill():
    b = Build(123)
    b.reset()
    ns = (17, 18, 64, 65, 66, 130, 200)
    words = [b.rnd(n + 1) for n in ns]
    for w in words:
        b.add(w)
    for w, n in zip(words, ns):
        b.reset(100)
        b.add(w[:n] + bytes([w[n] ^ 1]))
    _tail(b)
    return _c("hash fill of 16, 17, 63, 64, 65, 129, 199 positions", b, "nfill_16 nfill_17 nfill_63 nfill_64 nfill_65 nfill_129plus applied")


def _fill_dup(codec):
    log = 16 if codec == "LZ" else 19
    x, y = colliding_pair(log)
    b = Build(124 + log)
    b.reset()
    w = b.rnd(3) + x + b.rnd(12) + y + b.rnd(20)                 # one fill round stores x's and y's position in one slot
    b.add(w)
    b.reset()
    b.add(w)
    b.reset()
    b.add(y + b.rnd(8, first_not=w[25]))                         # must find y in the copy, the higher position; nothing behind it matches
    _tail(b)
    return _c("hash fill: one slot twice in a round, " + codec, b, "fill_dup_hash applied", codecs=(codec,))


def _lit_small():
    b = Build(125)
    w0 = b.add(b.rnd(8))
    plant_in_run(b, 0, 260, 0, near=8, exact=True)
    e = b.reset(30) + 30
    plant_in_run(b, e, 261, 0, near=8, exact=True)
    for n in (6, 7):                                             # the first 64 positions of a run are all visited: the block's first 8 bytes again
        b.reset(30)
        b.add(b.rnd(n, first_not=b.b[w0]))
        b.copy(w0, 8)
    _tail(b)
    return _c("literal runs of 260, 261, 6, 7", b, "lit_loop_260 lit_loop_261 lit_loop_6 lit_loop_7 applied")


def _lit_final(n):
    b = Build(126 + n)
    b.reset()
    b.add(b.rnd(20))
    b.add(bytes(300))
    b.add(b.rnd(n, first_not=0))
    return _c("final literal run of %d" % n, b, ["lit_final_%d" % n, "applied"])


def _lit_big(n):
    b = Build(127 + n)
    plant_in_run(b, 0, n, 20, near=340, wlen=12, exact=True)
    b.add(bytes(3000))
    b.add(b.rnd(n, first_not=0))
    return _c("literal runs of %d, in the loop and final" % n, b, ["lit_loop_%d" % n, "lit_final_%d" % n, "bwd_len_17plus", "applied"])


def _window_edge():
    b = Build(130)
    e = b.reset() + 12
    ws, wt, _ = plant_in_run(b, e, 65530, 6, dist=65530)         # 4 of the 6 bytes in front: ref reaches minRef
    # after the match every position is visited: distance 65533 is the largest the small window takes, 65534 sits on minRef.  The
    # two words are the run's own bytes at two of its visited (stored) positions.
    vis = visited(e, e + 400)
    s2 = next(v for v in vis if v + 65533 > len(b) + 2)
    s3 = next(v for v in vis if v > s2 + 20)
    b.add(b.rnd(s2 + 65533 - len(b), first_not=b.b[ws + 14]))
    b.copy(s2, 12)
    b.add(b.rnd(s3 + 65534 - len(b), first_not=b.b[s2 + 12]))
    b.copy(s3, 12)
    _tail(b, 2500)
    return _c("the small window's edge: distances 65530, 65533, 65534", b, "bwd_stop_minref dist_65533 reject_minref win_flag_0 applied")


def _clamp():
    b = Build(131)
    b.add(b.rnd(290, first_not=0))
    vis = visited(0, 400)
    p1 = next(v for v in vis if v >= 300)                        # the run of zeros begins two positions in front of a visited one
    b.pad_to(p1 - 2)
    b.b[p1 - 3] |= 1
    b.add(bytes(MAX_MATCH + 300))
    b.add(b.rnd(30, first_not=0))
    return _c("a table match extended beyond MAX_MATCH and clamped", b, "bwd_clamp fm_cut_mod1 nfill_129plus fill_dup_hash applied")


def _dna():
    rng = np.random.default_rng(132)
    words = [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(rng.integers(5, 40)))]) for _ in range(40)]
    data = b"".join(words[int(i)] for i in rng.integers(0, 40, 400))[:6000]
    return _c("DNA: minMatch 6", data, "applied", dtype="DNA")


def _patterns(b, n):
    """n tokens with new one-byte distances 3, 4, 5, 3, ...: runs of period 3, 4, 5 over fresh random bytes (never one of the two
    repeat distances, nor a multiple of one)"""
    for i in range(n):
        p = i % 3 + 3
        b.add(b.rnd(p) * (15 // p + 1))
        b.add(b.rnd(2))


def _many_tokens():
    b = Build(133)
    b.reset()
    w = b.add(b.rnd(16))
    b.add(b.rnd(300))
    _patterns(b, 61)
    b.reset()
    b.copy(w, 16)
    _tail(b)
    return _c("more than 64 tokens, a 2-byte distance across offset 64", b, "inv_token_idx_mult64 inv_dist2_straddle64 applied")


def _big(count):
    b = Build(134)
    b.reset()
    s = b.add(b.rnd(16) + b.rnd(16) + b.rnd(16))
    _patterns(b, 59)
    b.add(b.rnd(1, first_not=0))
    b.pad_to(s + 65535 - 12, 0)
    b.reset()
    for k in range(3):                                           # 17 bytes apart, their first copies 16: distances 65535, 65536, 65537
        b.copy(s + 16 * k, 16)
        b.add(bytes([b.b[s + 16 * k + 16] ^ 1]))
    b.pad_to(count - 40, 0)
    b.add(b.rnd(40, first_not=0))
    return b


def _big_cases():
    return [_c("count 262153: the small window", _big(262153), "win_flag_0 applied"),
            _c("count 262154: the large window, distances 65535, 65536, 65537", _big(262154), "win_flag_1 dist_65535 dist_65536 dist_gt_65536 inv_dist3_straddle64 inv_copy_far_long applied")]


def _outcomes():
    b = Build(135)
    out = [_c("23 bytes", bytes(23), "count_lt_24"), _c("24 zeros", bytes(24), "declined_ge_count"), _c("300 random bytes", b.rnd(300), "declined_ge_count")]
    b = Build(136)
    b.add(b.rnd(1500))
    b.add(bytes(40))
    b.add(b.rnd(1500, first_not=0))
    out.append(_c("saves less than 1 %", b, "declined_1pct"))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = [_skip_steps(), _peers("LZ"), _peers("LZX"), _rep_ends(), _lazy_runs(), _lazy_collide("LZ"), _lazy_collide("LZX"), _bwd_anchor(),
           _fm_lengths(), _fm_short(), _distances(), _mlen_codes(), _nfill(), _fill_dup("LZ"), _fill_dup("LZX"), _lit_small(),
           _lit_final(260), _lit_final(261), _dna(), _many_tokens()]
    out += [_fm_cut(k) for k in range(8)]
    out += _outcomes()
    out += [_bwd_lengths(), _clamp(), _window_edge(), _lit_big(65796), _lit_big(65797)]
    out += _big_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ---- frames ------------------------------------------------------------------------------------------------------------------------
Token = collections.namedtuple("Token", "tk_at lit lit_at lit_code kind dist dist_at dist_bytes mlen mlen_at mlen_code dst_at")


def frame_tokens(frame):
    """walk a valid LZ / LZX frame (the layout is in katmodels.lz_decode) -> (flag byte, [Token]): for every token where its byte, its
    literal-length code, its distance bytes and its match-length code lie in the frame (kind: "rep0", "rep1", "new", or "end" for the
    final, literal-only token), and dst_at, the output position of its match"""
    tk = int.from_bytes(frame[0:4], "little")
    mi = tk + int.from_bytes(frame[4:8], "little")
    ml = mi + int.from_bytes(frame[8:12], "little")
    mm = ((frame[12] >> 1) & 7) + 2
    pos, out, dst = 13, [], 0
    repd = [len(frame), len(frame)]

    def code(p):
        n = 1 if frame[p] < 254 else 3 if frame[p] == 254 else 4
        v = frame[p] if n == 1 else frame[p] + int.from_bytes(frame[p + 1:p + n], "big")
        return v, n

    while True:
        tk_at, token = tk, frame[tk]
        tk += 1
        lit, lit_at, lit_code = token >> 5, None, 0
        if token >= 0xE0:
            lit_at = pos
            v, lit_code = code(pos)
            lit, pos = 7 + v, pos + lit_code
        pos += lit
        dst += lit
        if token >= 32 and pos >= int.from_bytes(frame[0:4], "little") - 13:
            out.append(Token(tk_at, lit, lit_at, lit_code, "end", None, None, 0, None, None, 0, dst))
            return frame[12], out
        f = token & 0x18
        th = 3 if f == 0 else 7
        mlen, mlen_at, mlen_code = token & th, None, 0
        if mlen == th:
            mlen_at = ml
            v, mlen_code = code(ml)
            mlen, ml = th + v, ml + mlen_code
        mlen += mm
        if f == 0:
            kind, dist, dist_at, nb = ("rep0", repd[0], None, 0) if (token & 4) == 0 else ("rep1", repd[1], None, 0)
        else:
            nb = f >> 3
            kind, dist, dist_at = "new", int.from_bytes(frame[mi:mi + nb], "big"), mi
            mi += nb
        repd = [dist, repd[0]]
        out.append(Token(tk_at, lit, lit_at, lit_code, kind, dist, dist_at, nb, mlen, mlen_at, mlen_code, dst))
        dst += mlen


def recode_mlen_4byte(frame):
    """the same frame with its first 3-byte match-length code of 255 or more written in the 4-byte form (one byte longer; the
    match-length stream is the frame's last, no header field changes) -- the one readLength form no forward pass produces"""
    for t in frame_tokens(frame)[1]:
        if t.mlen_code == 3:
            v = frame[t.mlen_at] + int.from_bytes(frame[t.mlen_at + 1:t.mlen_at + 3], "big")
            if v >= 255:
                return frame[:t.mlen_at] + bytes([255]) + (v - 255).to_bytes(3, "big") + frame[t.mlen_at + 3:]
    raise AssertionError("no 3-byte code of 255 or more")


def surgery(frame, big_frame):
    """one edit each to a valid frame -> [(label, bytes)]: `frame` ends its match-length stream with a 3-byte code and begins with a
    new-distance token; big_frame (small window) has a 2-byte distance at an output position of 65535 or more.  All of them end in
    the reference's decoder, most by a refusal."""
    out = []
    toks = frame_tokens(frame)[1]
    last = [t for t in toks if t.mlen_code][-1]
    assert last.mlen_code == 3 and last.mlen_at + 3 == len(frame)
    out.append(("length code cut at the stream's end", frame[:-1]))
    t = next(t for t in toks if t.kind == "new")
    put = lambda f, t, d: f[:t.dist_at] + d.to_bytes(t.dist_bytes, "big") + f[t.dist_at + t.dist_bytes:]
    out.append(("distance 0", put(frame, t, 0)))
    assert t.dst_at + 1 < 256
    out.append(("distance dstIdx + 1", put(frame, t, t.dst_at + 1)))
    assert (big_frame[12] & 1) == 0
    t = next(t for t in frame_tokens(big_frame)[1] if t.kind == "new" and t.dist_bytes == 2 and t.dst_at >= 65535)
    out.append(("distance maxDist + 1 in the small window", put(big_frame, t, 65535)))
    out.append(("distance maxDist in the small window", put(big_frame, t, 65534)))
    out.append(("token-stream length count + 1", frame[:4] + (len(frame) + 1).to_bytes(4, "little") + frame[8:]))
    return out


SURGERY_CASES = ("findMatch results 8, 510, 1020", "the small window's edge: distances 65530, 65533, 65534")


def event_table(codec):
    """event -> names of the applied cases of this codec that produce it (the decline exits: of the cases that take them); the
    decoder's events are read from the model's own frame, which tests/test_lz_cases.py holds equal to the oracle's"""
    import katmodels
    table = collections.defaultdict(list)
    for c in cases():
        if codec in c.codecs:
            ev = collections.Counter()
            ok, enc = katmodels.lz_forward(c.data, codec == "LZX", c.dtype, events=ev)
            if ok:
                katmodels.lz_decode(enc, len(c.data), ev)
            for e in ev:
                if ok or e in OUTCOME_EVENTS:
                    table[e].append(c.name)
    return dict(table)


if __name__ == "__main__":
    for codec in BOTH:
        for e, names in sorted(event_table(codec).items()):
            print("%-4s%-26s%3d  %s" % (codec, e, len(names), "; ".join(names[:4]) + (" ..." if len(names) > 4 else "")))
