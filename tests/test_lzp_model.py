"""LZP's CPU model (tests/lzpmodel.py, a restatement of LZCodec.LZPCodec, K/transform/LZCodec.java:973-1287) against vectors worked
out by hand from the Java, its round trip on the reference's own test inputs, damaged input, a seeded fuzz whose counters show that
every branch is reached, and the ids / sizes the library reports for LZP.  No GPU needed."""
import kanzi_amd as kz
import lzpcases
import lzpmodel
import refinputs

FC, FE, FF = lzpcases.FC, lzpcases.FE, lzpcases.FF


def _vec(label):
    for lab, data, want in lzpcases.hand_vectors():
        if lab == label:
            return data, want
    raise KeyError(label)


def test_zeros():
    """5 000 x 00: dstEnd = 5 000 - 78 (:1053).  Bytes 0..3 are copied, ctx = 0 (:1057-1061).  Position 4: slot h(0) = 0 is empty, a
    literal.  Position 5: ctx is still 0, ref = 4, the ints at +60 agree, findMatch (:1257-1273) steps 8 bytes while
    bestLen + 8 <= 4 995: 4 992.  4 992 - 64 = 4 928 = 19 x 254 + 102: `fc`, 19 x `fe`, `66` (:1096-1111).  srcIdx = 4 997 is past
    srcEnd - 64: the tail loop (:1114-1128) copies the last three bytes.  4 + 1 + 21 + 3 = 29 bytes."""
    data, want = _vec("zeros")
    assert lzpmodel.forward(data) == (True, want) and len(want) == 29
    assert lzpmodel.inverse(want, len(data)) == (True, data)


def test_flags():
    """5 000 x fc: the same parse with ctx = fcfcfcfc.  Position 4 finds its slot empty, so its fc is NOT escaped (:1084); the three
    bytes of the tail loop find ref = 5 and are `fc ff` each (:1122-1126).  4 + 1 + 21 + 6 = 32 bytes."""
    data, want = _vec("flags")
    assert lzpmodel.forward(data) == (True, want) and len(want) == 32
    st = lzpmodel.new_stats()
    assert lzpmodel.inverse(want, len(data), st) == (True, data)
    assert st["fc_plain"] == 1 and st["fc_escaped"] == 3 and st["overlapping"] == 1 and st["chained"] == 1


def test_abc():
    """6 000 bytes of abcabc...: ctx is the little-endian read of `abca` at position 4 and shifts a byte in per literal (:1081), so
    the contexts of positions 4..9 are 61636261, 63626162, 62616263, 61626361, 62636162, 63616263: six different ones, six
    literals.  Position 10 has 61626361 again, ref = 7, and findMatch runs to the last whole step below 5 990: 5 984.  5 984 - 64 =
    5 920 = 23 x 254 + 78: `fc`, 23 x `fe`, `4e`; srcIdx = 5 994, the tail loop copies `abcabc`.  10 + 25 + 6 = 41 bytes."""
    data, want = _vec("abc")
    assert lzpmodel.forward(data) == (True, want) and len(want) == 41
    assert lzpmodel.inverse(want, len(data)) == (True, data)


def test_unit_of_300_bytes_repeated():
    """30 x a 300-byte unit u without fc: position 304 has the big-endian value of u[0..3] as ctx, position 4 had the LITTLE-endian one
    (:1061): no match there, nor at 305..307, whose counterparts 5..7 mixed both orders.  Position 308 repeats position 8's ctx (the
    big-endian u[4..7]): ref = 8, findMatch stops at the last whole step below 9 000 - 308 = 8 692: 8 688.  8 688 - 64 = 8 624 =
    33 x 254 + 242: `fc`, 33 x `fe`, `f2`; srcIdx = 8 996, four bytes for the tail loop.  308 + 35 + 4 = 347 bytes."""
    data, want = _vec("unit300")
    assert lzpmodel.forward(data) == (True, want) and len(want) == 347
    assert lzpmodel.inverse(want, len(data)) == (True, data)


def test_band_of_one_byte():
    """one match of L bytes costs two (`fc`, L - 64) and saves L: 4 096 - 67 + 2 = 4 031 < dstEnd = 4 032 applies, 4 096 - 66 + 2 =
    4 032 reaches dstEnd and declines (:1132)"""
    a, b = lzpcases.band_pair()
    assert FC not in a and FC not in b
    assert lzpmodel.forward(a) == (True, a[:2004] + FC + b"\x03" + a[2071:])
    ok, out = lzpmodel.forward(b)
    assert not ok and len(out) == 4032


def test_collision_pair():
    for c in lzpcases.COLLIDING:
        assert ((lzpmodel.HASH_SEED * c) & 0xFFFFFFFF) >> 16 == lzpcases.COLLIDING_SLOT
    a, b = lzpcases.collision_block(True), lzpcases.collision_block(False)
    st = lzpmodel.new_stats()
    ok, out = lzpmodel.forward(a, stats=st)
    assert ok and st["fc_escaped"] == 1 and st["fc_plain"] == 0 and out[304:306] == FC + FF
    st = lzpmodel.new_stats()
    ok2, out2 = lzpmodel.forward(b, stats=st)
    assert ok2 and st["fc_escaped"] == 0 and st["fc_plain"] == 1 and len(out2) == len(out) - 1
    assert lzpmodel.inverse(out, len(a)) == (True, a) and lzpmodel.inverse(out2, len(b)) == (True, b)


def test_forward_rules():
    assert lzpmodel.forward(b"") == (True, b"")                                          # :1024-1025
    assert lzpmodel.forward(bytes(127)) == (False, b"")                                  # :1038-1039
    assert lzpmodel.forward(bytes(128))[0] is True
    assert lzpmodel.forward(bytes(5000), 5000 + 77) == (False, b"")                      # :1034-1035
    assert lzpmodel.forward(bytes(5000), 5000 + 78)[0] is True
    assert lzpmodel.forward(bytes(1024), 1039) == (False, b"") and lzpmodel.forward(bytes(1024), 1040)[0]


def _round_trip(items):
    applied = declined = 0
    for data in items:
        data = bytes(data)
        if len(data) == 0:
            continue
        ok, out = lzpmodel.forward(data)
        if not ok:
            declined += 1
            continue
        applied += 1
        assert len(out) < len(data) - (len(data) >> 6)
        assert lzpmodel.inverse(out, len(data)) == (True, data)
        assert lzpmodel.inverse(out, len(data) - 1)[0] is False
    return applied, declined


def test_round_trip_on_the_reference_inputs():
    assert _round_trip(refinputs.transform_inputs())[0] == 45
    assert _round_trip(refinputs.edge_inputs())[0] == 5


def test_inverse_on_damaged_input():
    data, coded = lzpcases.short_coded_block()
    got = {lab: lzpmodel.inverse(c, n) for lab, c, n in lzpcases.damaged_inputs()}
    # a cut block decodes to a prefix unless the cut falls inside a code: behind the fc of a match or an escape, or behind its fe
    m1, m2, esc = 400, coded.index(FC + FE), coded.rindex(FC + FF)
    assert coded[m1] == 0xFC and coded[m2 + 2] not in (0xFE, 0xFF)
    fails = [k for k in range(len(coded) + 1) if not got["cut%d" % k][0]]
    assert fails == [1, 2, 3, m1 + 1, m2 + 1, m2 + 2, esc + 1]
    for k in range(len(coded) + 1):
        ok, out = got["cut%d" % k]
        if ok:
            assert data.startswith(out), k
    assert got["cut0"] == (True, b"") and got["cut4"] == (True, data[:4])
    assert got["fe_to_end"][0] is False and got["fe_to_end_long"][0] is False            # :1216-1222
    assert got["flag_last"][0] is False                                                  # :1199-1200
    assert got["one_short"][0] is False and got["exact"] == (True, data) and got["roomy"] == (True, data)   # :1227-1228
    assert got["dst_below_count"] == (False, b"")                                        # :1163-1164
    assert [got["count%d" % n][0] for n in range(5)] == [True, False, False, False, True]
    assert got["count4_flags"] == (True, FC * 4) and got["count5_flag"] == (True, b"abcd" + FC)   # ref == 0: a plain literal (:1186)
    # a literal past dstEnd (:1187-1188), an escape past dstEnd (:1203-1204)
    assert lzpmodel.inverse(b"abcdef", 6) == (True, b"abcdef") and lzpmodel.inverse(b"abcdefg", 7)[0]
    esc = lzpmodel.forward(FC * 5000)[1]
    assert lzpmodel.inverse(esc, 4999)[0] is False and lzpmodel.inverse(esc, 4998)[0] is False


def test_fuzz_reaches_every_branch():
    fwd, inv = lzpmodel.new_stats(), lzpmodel.new_stats()
    applied = 0
    for seed in range(6):
        d = lzpcases.fuzz_block(seed)
        ok, out = lzpmodel.forward(d, stats=fwd)
        applied += ok
        if ok:
            assert lzpmodel.inverse(out, len(d), inv) == (True, d), seed
    assert applied == 6
    for key in ("matches", "chained", "fc_escaped", "fc_plain", "fc_escaped_near", "fc_plain_near"):
        assert fwd[key] >= 20, (key, fwd)
    assert fwd["matches"] > fwd["chained"]                       # lengths with and without a 0xFE
    for key in ("matches", "chained", "overlapping", "fc_escaped", "fc_plain"):
        assert inv[key] >= 20, (key, inv)
    assert inv["matches"] > inv["overlapping"]
    assert (inv["matches"], inv["chained"], inv["fc_escaped"], inv["fc_plain"]) == (fwd["matches"], fwd["chained"], fwd["fc_escaped"], fwd["fc_plain"])


def test_seam_inputs_are_what_they_claim():
    """the inputs tests/test_gpu_lzp.py builds for the device parse, checked against the model alone"""
    w = 64
    for at in range(5, 4 + 2 * w + 1, 7):
        d = lzpcases.match_at(at)
        ok, out = lzpmodel.forward(d)
        assert ok and out[:at] == d[:at] and out[at] == 0xFC, at
    st = lzpmodel.new_stats()
    for off in range(0, 2 * w, 5):
        assert lzpmodel.forward(lzpcases.late_match(off, 6), stats=st)[0]
    assert st["matches"] == 26 and st["fc_escaped"] >= 26 and st["fc_plain"] >= 26
    cuts = 0
    for n in (1000, 1003):
        for k in range(10):
            d = lzpcases.match_to_end(k, n)
            ok, out = lzpmodel.forward(d)
            room, equal = n - 600, n - 600 - k
            # findMatch (:1260-1270) finds the first differing byte only if the 8-byte step that holds it still fits
            length = equal if equal // 8 * 8 + 8 <= room else room // 8 * 8
            cuts += length < equal
            assert ok and out == d[:600] + FC + FE + bytes([length - 64 - 254]) + d[600 + length:], (n, k)
    assert cuts == 3                                             # 1 003: the matches that end 0, 1 and 2 bytes before the end stop at 400
    for lab, d in lzpcases.dst_end_cases():
        ok, out = lzpmodel.forward(d)
        assert not ok and len(out) == len(d) - (len(d) >> 6), lab
        assert lab == "literal" or out[-1:] == {"escape": FC, "chain": FE}[lab]
    st = lzpmodel.new_stats()
    assert lzpmodel.forward(lzpcases.broken_runs(), stats=st)[0] and st["matches"] == 1 and st["fc_escaped"] > 500
    assert lzpmodel.forward(lzpcases.broken_runs(False))[0] is False


def test_library_knows_lzp():
    lib = kz.load_library()
    for n, want in ((128, 144), (1024, 1040), (1025, 1041), (4 << 20, (4 << 20) + 65536)):   # :1284-1286
        assert lib.kz_transform_max_encoded_len(14, n) == want, n
        assert lzpmodel.max_encoded_length(n) == want
    assert kz.TRANSFORM_IDS["LZP"] == 14 and kz.LZP_TYPE == 14 and kz.LZPCodec.TYPE == 14
    assert kz.transform_type("LZP+ZRLT") == (14 << 42) | (6 << 36)
