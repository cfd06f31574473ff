"""The case set of tests/ans0cases.py is what it claims (CPU only): every seam of kanzi_amd/csrc/kz_ans.hip that
tests/test_gpu_ans0.py means to cross is reached by a named case, the Python model (ans1model at order 0) and the CPU oracle
agree on every stream the GPU tests expect answers for, and a block's stream is the concatenation of its chunks' streams.  The
coverage sets below are the condition that keeps the GPU tests from passing vacuously: each is asserted by name."""
import functools

import ans0cases as C
import ans1model
import katmodels
import oracle

NO_ROUND_TRIP = {"slow-_limit"}         # the reference's own decoder does not return these inputs (see test_slow_minus_at_the_round_limit)


@functools.lru_cache(maxsize=None)
def _facts():
    """{case name: [chunk_facts of every chunk]} (without the coded sizes: those come from the layouts)"""
    return {c.name: [C.chunk_facts(x, code=False) for x in C.chunks_of(c.data)] if len(c.data) > 32 else [] for c in C.encoder_cases()}


@functools.lru_cache(maxsize=None)
def _streams():
    return {c.name: oracle.entropy_encode("ANS0", c.data) for c in C.encoder_cases()}


@functools.lru_cache(maxsize=None)
def _layouts():
    return {c.name: C.block_layout(c.data, _streams()[c.name]) for c in C.encoder_cases()}


def _all_facts():
    return [(name, f) for name, fs in _facts().items() for f in fs]


def _have(pred):
    return sorted({name for name, f in _all_facts() if pred(f)})


def test_classifier_walks_normalize(built):
    """normalize_path leaves the frequencies of katmodels._normalize on every chunk of the set, and never takes one of the two
    branches the module docstring argues away"""
    for c in C.encoder_cases():
        for x in C.chunks_of(c.data):
            a, b = C.counts(x), C.counts(x)
            alphabet, facts = C.normalize_path(a, len(x), 4096)
            assert alphabet == katmodels._normalize(b, len(x), 4096) and a == b, c.name
            assert "no_symbol_left" not in facts and "clamped" not in facts, c.name


def test_a_block_is_the_concatenation_of_its_chunks(built):
    """the model's bit string of every chunk alone, joined, is the oracle's stream of the block; block_layout() reads the same
    positions out of the oracle's stream; a block of 32 bytes or fewer is stored raw"""
    checked = 0
    for c in C.encoder_cases():
        bits, nbits = _streams()[c.name]
        if len(c.data) <= 32:
            assert (bits, nbits) == (c.data, 8 * len(c.data)), c.name
            continue
        if not c.model:
            continue
        codes = [C.chunk_code(x) for x in C.chunks_of(c.data)]
        assert C.pack("".join(s for s, _, _ in codes)) == (bits, nbits), c.name
        pos = 0
        for (s, hb, _), lay in zip(codes, _layouts()[c.name]):
            assert lay == (pos, hb, len(s)), c.name
            pos += len(s)
        checked += 1
    assert checked >= 50


def test_oracle_round_trip(built):
    for c in C.encoder_cases():
        bits, nbits = _streams()[c.name]
        r, out, pos = oracle.entropy_decode("ANS0", bits, nbits, len(c.data))
        assert r == len(c.data) and (pos == nbits or not c.data), c.name
        assert (out == c.data) == (c.name not in NO_ROUND_TRIP), c.name


def test_slow_minus_at_the_round_limit(built):
    """slow- at the round limit is the reference's own defect: after five rounds that raised six symbols each, the remainder is
    SUBTRACTED from the maximum (freqs[idxMax] - delta, EntropyUtils.java:248) although the sum was short, the frequencies sum to
    3996, and the decoder, which gives the first symbol what the others leave, decodes other bytes and ends the chunk with its
    byte count off.  The encoder's bits are still the reference's bits: the device must write them, and decode them as the
    oracle does."""
    c = [c for c in C.encoder_cases() if c.name == "slow-_limit"][0]
    f = C.counts(c.data)
    katmodels._normalize(f, len(c.data), 4096)
    assert sum(f) == 3996
    bits, nbits = _streams()[c.name]
    r, out, pos = oracle.entropy_decode("ANS0", bits, nbits, len(c.data))
    m = ans1model.decode(bits, nbits, len(c.data), 0)
    assert m == (r, out, pos, False) and out != c.data


def test_normalisation_paths_are_reached(built):
    for path in ("shortcut", "one", "exact", "fast+", "fast-", "slow+", "slow-"):
        assert _have(lambda f: f["path"] == path), "no case takes the normalisation path " + path
    assert _have(lambda f: f["path"] == "slow+" and f["rounds"] == 1 and not f["limit"]), "no slow+ chunk of one round"
    assert _have(lambda f: f["path"] == "slow+" and f["rounds"] >= 3 and not f["limit"]), "no slow+ chunk of three rounds or more inside the limit"
    assert _have(lambda f: f["path"] == "slow+" and f["limit"]), "no slow+ chunk at the round limit"
    assert _have(lambda f: f["path"] == "slow-" and f["rounds"] == 1), "no slow- chunk of one round"
    assert _have(lambda f: f["path"] == "slow-" and f["limit"]), "no slow- chunk at the round limit"
    names = dict(_all_facts_by_name())
    for n, k in C.SLOW_MINUS:
        assert names["slow-_%d_over_%d" % (n, k)]["path"] == "slow-", (n, k)
    for name in ("fast+", "fast-", "exact", "shortcut"):
        assert names[name]["path"] == name, name
    assert [f["path"] for f in _facts()["shortcut_last"]] == ["fast+", "shortcut"]
    # the maximum: tied, its first holder in group g and an equal one in a later group (g = 1, 2), tied inside group 3, and tied
    # across all four groups -- on a path that adjusts the maximum
    uses = ("fast+", "fast-", "slow+", "slow-")
    for g in (1, 2):
        f = names["tied_max_group_%d" % g]
        assert f["path"] in uses and f["tied"] and f["first_max_group"] == g and max(f["max_groups"]) > g, g
        assert _have(lambda f: f["path"] in uses and f["tied"] and f["first_max_group"] == g and max(f["max_groups"]) > g), "no tied maximum first held in group %d" % g
    assert _have(lambda f: f["path"] in uses and f["tied"] and f["max_groups"] == [3]), "no tied maximum inside group 3"
    assert _have(lambda f: f["path"] in uses and f["tied"] and f["max_groups"] == [0, 1, 2, 3]), "no maximum tied across the four groups"
    assert _have(lambda f: f["path"] in uses and not f["tied"] and f["first_max_group"] == 3), "no single maximum in group 3"


def _all_facts_by_name():
    return [(name, fs[0]) for name, fs in _facts().items() if fs]


def test_header_forms_are_reached(built):
    assert _have(lambda f: f["form"] == "256"), "no alphabet of 256"
    assert _have(lambda f: f["form"] == "1"), "no alphabet of one symbol"
    names = dict(_all_facts_by_name())
    assert (names["alphabet_below_8"]["form"], names["alphabet_below_8"]["last_mask"]) == ("partial", 0)
    assert (names["alphabet_with_255"]["form"], names["alphabet_with_255"]["last_mask"]) == ("partial", 31)
    for lm in (0, 31):
        assert _have(lambda f: f["form"] == "partial" and f["last_mask"] == lm), "no partial alphabet with lastMask %d" % lm
    for size, group in ((2, 6), (63, 6), (64, 8), (65, 8), (255, 8), (256, 8)):
        assert _have(lambda f: f["alphabet_size"] == size and f["group"] == group), "no alphabet of %d symbols in groups of %d" % (size, group)
    assert _have(lambda f: f["logmax0"]), "no frequency group with logMax == 0"
    assert _have(lambda f: f["last_group"] == 1 and f["group"] == 6), "no last group of one symbol (groups of 6)"
    assert _have(lambda f: f["last_group"] == 1 and f["group"] == 8), "no last group of one symbol (groups of 8)"
    assert _have(lambda f: f["last_group"] == f["group"]), "no full last group"


def test_coding_loop_lengths_are_reached(built):
    coded = [(n, f) for n, f in _all_facts() if f["alphabet_size"] > 1]
    for r in range(4):
        assert any(f["len3"] == r for _, f in coded), "no coded chunk with len & 3 == %d" % r
        assert any(f["dwords3"] == r for _, f in coded), "no coded chunk with (len >> 2) & 3 == %d" % r
    tails = {len(C.chunks_of(c.data)[-1]) for c in C.encoder_cases() if c.name.startswith("tail_")}
    assert tails == set(C.TAIL_LENGTHS), "a short last chunk is missing"
    assert _facts()["tail_1"][1]["form"] == "1"                       # one byte: one symbol, no payload
    for t in (2, 3):                                                  # two symbols: a payload of 2 or 3 tail bytes, no dword to code
        lay = _layouts()["tail_%d" % t][1]
        assert _facts()["tail_%d" % t][1]["alphabet_size"] == 2 and lay[2] - lay[1] == 8 + 128 + 8 * t, t
    assert {len(c.data) for c in C.encoder_cases() if c.name.startswith("block_")} >= {33, 34, 35, 36}


def test_varint_lengths(built):
    """payload sizes of one, two and three varint bytes are in the set: three bytes take a payload of 16384 bytes, 8 bits per symbol,
    which the chunk holding every symbol 64 times reaches to the byte (and nothing in the set exceeds)"""
    sizes = {}
    for name, lay in _layouts().items():
        for (s, hb, tb), f in zip(lay, _facts()[name]):
            if f["alphabet_size"] > 1:
                coded = (tb - hb - 128) // 8                          # varint bytes + payload bytes
                sizes[(name, s)] = coded - (1 if coded - 1 < 128 else 2 if coded - 2 < 16384 else 3)
    assert any(v < 128 for v in sizes.values()), "no payload of a one-byte varint"
    assert any(128 <= v < 16384 for v in sizes.values()), "no payload of a two-byte varint"
    assert any(v >= 16384 for v in sizes.values()), "no payload of a three-byte varint"
    assert sizes[("exact", 0)] == 16384 == max(sizes.values())
    assert C.chunk_facts(C.encoder_cases_by_name()["exact"].data)["varint"] == 3
    edge = C.chunk_facts(C.encoder_cases_by_name()["varint_edge"].data)
    assert edge["path"] == "slow+" and edge["varint"] == 2 and 16370 < edge["payload"] < 16384, edge["payload"]


def test_splices_are_reached(built):
    res, inside, most = set(), False, 0
    for name, lay in _layouts().items():
        r, i, m = C.splice_facts(lay)
        res |= r
        inside |= i
        most = max(most, m)
    for r in range(32):
        assert r in res, "no chunk starts at bit %d mod 32" % r
    assert inside, "no chunk under 32 bits inside one word"
    assert most >= 3, "no word holding bits of three chunks"
    assert C.splice_facts(_layouts()["runs_33"])[0] == set(range(32))
    assert all(t == 17 for _, _, t in _layouts()["runs_12"]) and len(_layouts()["runs_12"]) == 12
    alt = _layouts()["runs_alternated"]
    assert [t == 17 for _, _, t in alt] == [i % 2 == 0 for i in range(12)]


def test_scan_case(built):
    data = C.scan_case()
    assert len(data) == (1 << 20) + 5
    lay = C.block_layout(data)
    assert len(lay) == 65 and lay[64][0] > 0 and lay[64][2] > lay[64][1]          # the 65th chunk is coded, behind a carry
    assert len({t for _, _, t in lay}) > 30


def test_window_cases(built):
    """renormalisations per step of four symbols: the uniform chunk refills nearly four states a step (2 bytes each: a payload of
    about the chunk's size), the two-symbol chunk almost none (the 16-byte window slides a few times in 4096 steps)"""
    uni, two = _layouts()["window_uniform"][0], _layouts()["window_two_symbols"][0]
    assert (uni[2] - uni[1]) // 8 > 16000
    assert (two[2] - two[1]) // 8 < 100


def _model_decode(bits, nbits, count):
    try:
        return ans1model.decode(bits, nbits, count, 0)
    except katmodels.JavaException:
        return -1, None, None, True


def test_crafted_decoder_streams(built):
    """every crafted stream ends the way it was built to, in the model and in the oracle: the verdict (decode() == count), the bytes
    with their zero tail from where the reference stops writing, and the bits consumed.  Model and oracle agree on the bit position
    after STOP and SKIP in every case, so the GPU test asserts it there; after FAIL only the verdict exists (the model throws,
    the oracle's position is where its reader happened to be)."""
    kinds = set()
    for d in C.decoder_cases():
        r, out, pos = oracle.entropy_decode("ANS0", d.bits, d.nbits, d.count)
        m = _model_decode(d.bits, d.nbits, d.count)
        kind, chunk = d.event
        kinds.add(kind)
        assert (r == d.count) == (kind != "FAIL") == (m[0] == d.count), d.name
        if kind == "FAIL":
            continue
        assert m[:3] == (r, out, pos) and m[3] is False, d.name                # `clean` False: decodeChunkV2 returned false
        written = min((chunk + (kind == "STOP")) * C.CHUNK, d.count)
        assert out[written:] == bytes(d.count - written), d.name
        assert any(out[max(written - 64, 0):written]) or written == 0, d.name
        assert pos < d.nbits or d.name in ("stop_last", "grown_buffer_takes_300"), d.name
    assert kinds == {"FAIL", "SKIP", "STOP"}
    names = {d.name for d in C.decoder_cases()}
    for need in ("stop_mid", "skip_mid", "fail_empty_alphabet", "fail_logmax", "fail_sum_at_scale", "fail_cut_frequencies", "fail_size_above_buffer",
                 "fail_size_300_alone", "grown_buffer_takes_300", "fail1_stop2_index", "fail1_stop2_chunk", "stop1_fail3_index", "stop1_fail3_chunk"):
        assert need in names, need


def test_every_lr(built):
    """the model's streams at logRange 8 .. 15 decode in the oracle to the input, every bit consumed; at 12 they are the oracle's
    encoder's"""
    for name, data in C.lr_inputs().items():
        for lr in C.LR_RANGE:
            bits, nbits = C.lr_stream(name, lr)
            assert oracle.entropy_decode("ANS0", bits, nbits, len(data)) == (len(data), data, nbits), (name, lr)
            if len(data) > 32:
                assert C.bitstr(bits, 3) == format(lr - 8, "03b")
        assert C.lr_stream(name, 12) == oracle.entropy_encode("ANS0", data), name
    assert len(C.lr_inputs()["raw_limit_33"]) == 33 and len(C.chunks_of(C.lr_inputs()["three_chunks_skewed"])) == 3


def test_block_frames(built):
    """block_stream() is the frame the oracle reads: an untouched entropy stream comes back as the block, and the five small
    crafted blocks end as built (a block that fails is refused; one that stops or skips is returned with its zero tail)"""
    data = C.geometric(600, 200, 0.4, 9)
    s, _, _ = C.chunk_code(data)
    bits, nbits = C.pack(s)
    stream, w = C.block_stream(len(data), bits, nbits)
    assert (stream, w) == oracle.encode_block("NONE", "ANS0", data)[:2]
    assert oracle.decode_block("NONE", "ANS0", 512, stream, w, 512) == (len(data), data)
    kinds = []
    for n, b, nb, kind in C.small_event_blocks():
        stream, w = C.block_stream(n, b, nb)
        r, out = oracle.decode_block("NONE", "ANS0", 512, stream, w, 512)
        assert (r == n) == (kind != "FAIL"), (n, kind, r)
        if kind == "SKIP":
            assert out == bytes(n)
        kinds.append(kind)
    assert sorted(set(kinds)) == ["FAIL", "SKIP", "STOP"]
