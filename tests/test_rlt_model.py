"""RLT's CPU model (tests/rltmodel.py, a line-by-line restatement of K/transform/RLT.java) against vectors worked out by hand from
the Java, its round trip on the reference's own test inputs, and the ids / sizes the library reports for RLT.  No GPU needed."""
import kanzi_amd as kz
import refinputs
import rltmodel

TAIL = bytes(range(10, 30))                   # twenty distinct bytes: the end of the block never touches the run under test
TAIL_HEX = TAIL.hex()


def fwd(data, dst_len=None, **kw):
    ok, out, _ = rltmodel.forward(data, len(data) + 32 if dst_len is None else dst_len, **kw)
    return ok, out.hex()


def test_run_that_fills_the_block():
    """80 000 x 07 under NONE: escape fb (:38,:105-107); header `fb 07` (:154-155); the first segment counts 73 472 repeats of byte 0
    (run starts at 0 and stops at the first multiple of four >= MAX_RUN4 = 73 469, :178): `07 fb` + length 73 472 - 3 - 7 936 = 65 533 =
    `ff fffd` (:283-286); the second one starts at byte 73 473 with run = 1 and is closed when srcIdx reaches srcEnd4 = 79 996 (:178):
    1 + 4 x 1 631 = 6 525 bytes, 6 522 - 224 = 6 298 = 0x189a -> `f8 9a` (:280-282); the last two bytes are copied (:226-257)."""
    assert fwd(b"\x07" * 80000) == (True, "fb0707fbfffffd07fbf89a0707")


def test_block_that_starts_with_the_escape():
    """byte 0 = fb goes out as `fb fb 00` (:154-158); 01 02 are copies; 30 x 09 -> `09 fb 1b` (30 - 3 = 27, :277,:290)"""
    assert fwd(b"\xfb\x01\x02" + b"\x09" * 30 + TAIL) == (True, "fbfb00010209fb1b" + TAIL_HEX)


def test_escape_inside_and_outside_a_coded_run():
    """a lone fb is `fb 00` (:206-215); ten of them are `fb 00 fb 07`: the value, its 0, the mark, 10 - 3 (:191-197)"""
    assert fwd(b"\x01\x02\xfb\x03" + b"\xfb" * 10 + TAIL) == (True, "fb0102fb0003fb00fb07" + TAIL_HEX)


def test_length_code_boundaries():
    """emitRunLength (:276-292) codes run - 3: below 224 in one byte, below 7 936 as 224 + (r - 224 >> 8), (r - 224) & 255, else ff and
    r - 7 936 in two bytes.  A run that starts behind byte 0 is counted from 1 (:220), so `run` is its whole length."""
    for run, code in ((226, "df"), (227, "e000"), (7938, "fe1f"), (7939, "ff0000"), (73469, "fffffa")):
        assert fwd(b"\x01\x02" + b"\x09" * run + TAIL) == (True, "fb010209fb" + code + TAIL_HEX), run


def test_long_run_is_cut_into_pieces_of_max_run4():
    """2 x 73 469 + 2 bytes from byte 2 on: the loop stops at run >= MAX_RUN4 (:178) twice, each piece `09 fb ff fffa`; the two bytes
    left are copies (run <= RUN_THRESHOLD, :198-205).  2 + 1 + 5 + 5 + 2 + 20 = 35 bytes."""
    ok, out = fwd(b"\x01\x02" + b"\x09" * (2 * 73469 + 2) + TAIL)
    assert ok and out == "fb0102" + "09fbfffffa" * 2 + "0909" + TAIL_HEX and len(out) == 70


def band_example():
    d = bytearray((7 * i) % 200 for i in range(1000))
    d[993:998] = bytes([201]) * 5
    return bytes(d)


def test_the_array_length_decides_in_a_narrow_band():
    """dstEnd is dst.length (:115).  993 copies make dstIdx 994 at the coded run of 201s: 994 + 6 >= 1 000 fails (:186-189), with one
    more byte in the array it is coded and the block comes out one byte shorter than it went in."""
    d = band_example()
    ok, out, _ = rltmodel.forward(d, 1000)
    assert not ok
    ok, out, _ = rltmodel.forward(d, 1001)
    assert ok and len(out) == 999
    assert rltmodel.inverse(out, 1000) == (True, d)


def test_context_rules():
    d = bytes([65, 67, 71, 84] * 8)
    # a context that says DNA / BASE64 / UTF8 declines whatever the coder (:97-99)
    for dt in ("DNA", "BASE64", "UTF8"):
        for e in ("NONE", "FPAQ"):
            assert rltmodel.forward(b"\x07" * 100, 132, e, dt) == (False, b"", dt)
    # the type is only looked for when the escape is searched (:117-132): detected DNA is stored back and declines
    assert rltmodel.forward(d, 64, "FPAQ") == (False, b"", "DNA")
    assert rltmodel.forward(d, 64, "FPAQ", have_ctx=False) == (False, b"", "UNDEFINED")
    assert rltmodel.forward(d, 64, "NONE")[2] == "UNDEFINED"
    # the escape is the lowest symbol of minimal frequency (:134-148): 0 when it is absent
    ok, out, _ = rltmodel.forward(b"\x01\x02" + b"\x09" * 30 + TAIL, 100, "FPAQ")
    assert ok and out.hex() == "00010209001b" + TAIL_HEX
    assert rltmodel.forward(b"\x07" * 15, 64) == (False, b"", "UNDEFINED")               # :78-79
    assert rltmodel.forward(b"", 0) == (True, b"", "UNDEFINED")                          # :70-71


def test_inverse_failure_rules():
    inv = rltmodel.inverse
    assert inv(bytes.fromhex("fbfb05"), 100) == (False, b"")                             # starts with a run :324-329
    assert inv(bytes.fromhex("fbfb00"), 100) == (True, b"\xfb")
    assert inv(bytes.fromhex("fb0102fb"), 100)[0] is False                               # escape as the last byte :348-351
    assert inv(bytes.fromhex("fb01fbe0"), 100)[0] is False                               # two-byte length cut short :376-379
    assert inv(bytes.fromhex("fb01fbff00"), 100000)[0] is False                          # three-byte length cut short :367-370
    assert inv(bytes.fromhex("fb01fbff"), 100000)[0] is False
    assert inv(bytes.fromhex("fb01fb05"), 8) == (True, b"\x01" * 8)                      # 1 + (5 + 2)
    assert inv(bytes.fromhex("fb01fb05"), 7)[0] is False                                 # a run past dstEnd :387
    assert inv(bytes.fromhex("fb0102"), 1)[0] is False                                   # a literal at dstEnd :339-340, :406
    assert inv(bytes.fromhex("fb01fb00"), 1) == (True, b"\x01")                          # an escape literal at dstEnd is read and dropped :358-359
    assert inv(bytes.fromhex("fb01fb0002"), 1)[0] is False
    assert inv(bytes.fromhex("fb01fb00fb03"), 100) == (True, b"\x01\xfb" + b"\xfb" * 5)  # a run repeats the last byte PRODUCED :353
    assert inv(bytes.fromhex("fb01fb02fb03"), 100) == (True, b"\x01" * 10)


def _round_trip(items, have_ctx):
    applied = declined = 0
    for data in items:
        data = bytes(data)
        ok, out, _ = rltmodel.forward(data, len(data) + 32, "NONE", "UNDEFINED", have_ctx)
        if not ok:
            declined += 1
            continue
        applied += 1
        assert len(out) < len(data)
        assert rltmodel.inverse(out, len(data)) == (True, data)
    return applied, declined


def test_round_trip_on_the_reference_inputs():
    assert _round_trip(refinputs.transform_inputs(), False) == (49, 2)      # TestTransforms.java builds `new RLT()`
    assert _round_trip(refinputs.edge_inputs(), True) == (31, 24)


def test_library_knows_rlt():
    lib = kz.load_library()
    for n, want in ((16, 48), (512, 544), (513, 513), (4 << 20, 4 << 20)):                # RLT.java:419-421
        assert lib.kz_transform_max_encoded_len(5, n) == want, n
        assert rltmodel.max_encoded_length(n) == want
    assert kz.TRANSFORM_IDS["RLT"] == 5 and kz.RLT_TYPE == 5 and kz.RLT.TYPE == 5
    assert kz.transform_type("RLT+BWT") == (5 << 42) | (1 << 36)
