"""The case set of tests/lzcases.py on the CPU: every case gives the same parse in the oracle and in katmodels.lz_forward, produces the
events it was built for (read from the model's trace, never from a label), the set as a whole reaches every seam listed in lzcases for
LZ and for LZX, and it tells each single-line mutant of the model from the reference.  tests/test_gpu_lz.py runs the same cases
through kanzi_amd/csrc/kz_lz.hip."""
import collections
import functools

import pytest

import katmodels
import lzcases
import oracle


@functools.lru_cache(maxsize=None)
def _oracle(name, codec):
    c = _by_name()[name]
    ok, out, _ = oracle.transform_forward(codec, c.data, data_type=oracle.DT[c.dtype])
    return ok, out


@functools.lru_cache(maxsize=None)
def _by_name():
    return {c.name: c for c in lzcases.cases()}


@functools.lru_cache(maxsize=None)
def _traces():
    """(case name, codec) -> (applied, bytes, forward events, decoder events of the oracle's frame)"""
    out = {}
    for c in lzcases.cases():
        for codec in c.codecs:
            ev, iv = collections.Counter(), collections.Counter()
            ok, enc = katmodels.lz_forward(c.data, codec == "LZX", c.dtype, events=ev)
            ok_o, enc_o = _oracle(c.name, codec)
            if ok_o:
                assert katmodels.lz_decode(enc_o, len(c.data), iv) == c.data, (c.name, codec)
                assert katmodels.lz_decode(enc_o, len(c.data)) == c.data and katmodels.lz_decode(enc_o, len(c.data) - 1) is None
            out[c.name, codec] = (ok, enc, ev, iv)
    return out


def test_form_of_the_set():
    cs = lzcases.cases()
    assert cs is lzcases.cases() and len(cs) >= 30
    sizes = sorted(len(c.data) for c in cs)
    assert sizes[-2:] == [262153, 262154] and sizes[-3] < 140 << 10 and sizes[len(sizes) * 2 // 3] < 8 << 10
    for c in cs:
        assert set(c.codecs) <= {"LZ", "LZX"} and c.codecs and c.dtype in ("UNDEFINED", "DNA") and set(c.events) == set(c.codecs), c.name
    assert {c.dtype for c in cs} == {"UNDEFINED", "DNA"}
    for log in (16, 19):
        x, y = lzcases.colliding_pair(log)
        assert x[:4] != y[:4] and int(lzcases.hash5([list(x)], log)[0]) == int(lzcases.hash5([list(y)], log)[0])
        for shift in (1, 2):
            s = lzcases.self_colliding(log, shift)
            assert s[0] != s[shift] and int(lzcases.hash5([list(s[:5])], log)[0]) == int(lzcases.hash5([list(s[shift:])], log)[0])


def test_model_has_the_same_parse_and_the_trace_changes_nothing():
    """(a) the same (applied, bytes) from the model and from the oracle; the model's decoder returns the input from the oracle's frame
    (in _traces); passing a Counter changes no byte"""
    for (name, codec), (ok, enc, ev, iv) in _traces().items():
        ok_o, enc_o = _oracle(name, codec)
        assert ok == ok_o, (name, codec)
        if ok_o:
            assert enc == enc_o, (name, codec)
        c = _by_name()[name]
        if len(c.data) < 20000:
            assert katmodels.lz_forward(c.data, codec == "LZX", c.dtype) == (ok, enc), (name, codec)


def test_every_case_produces_its_events():
    """(b)"""
    for (name, codec), (ok, enc, ev, iv) in _traces().items():
        want = _by_name()[name].events[codec]
        assert want, name
        assert want <= set(ev) | set(iv), (name, codec, sorted(want - set(ev) - set(iv)))
        assert ("applied" in want) == ok or not want & {"applied", "declined_ge_count", "declined_1pct", "count_lt_24"}, (name, codec)


def _unreached_events():
    return {e for names, why in lzcases.UNREACHED.values() for e in names}


def test_unreached_table():
    """(d) at most three entries, each ruled out by arithmetic that is restated here, none of them ever seen"""
    assert len(lzcases.UNREACHED) <= 3
    assert _unreached_events() <= set(lzcases.FORWARD_EVENTS)
    mm, mx = 4, lzcases.MAX_MATCH
    assert mx & ~7 < mx                                            # findMatch's largest result is below MAX_MATCH
    assert mx - mm - 3 < 65789 and mx - mm - 7 < 65789             # the largest length codes
    assert mm - 1 >= 3                                             # the smallest hash fill
    for (name, codec), (ok, enc, ev, iv) in _traces().items():     # (the final run: every match ends at srcEnd = count - 18 or before)
        assert not set(ev) & _unreached_events(), (name, codec, sorted(set(ev) & _unreached_events()))
        if ok:
            assert lzcases.frame_tokens(enc)[1][-1].lit >= 18, (name, codec)


@pytest.mark.parametrize("codec", ["LZ", "LZX"])
def test_the_set_reaches_every_seam(codec):
    """(c) every listed event in at least one APPLIED case of this codec; the decline exits in cases that take them"""
    where = collections.defaultdict(list)
    for (name, cd), (ok, enc, ev, iv) in _traces().items():
        if cd == codec:
            for e in list(ev) + list(iv):
                if ok or e in lzcases.OUTCOME_EVENTS:
                    where[e].append(name)
    want = set(lzcases.FORWARD_EVENTS) | set(lzcases.INVERSE_EVENTS) | set(lzcases.OUTCOME_EVENTS) | (set(lzcases.LZX_ONLY_EVENTS) if codec == "LZX" else set())
    missing = sorted(want - set(where) - _unreached_events())
    assert not missing, (codec, missing)
    big = {c.name for c in lzcases.cases() if len(c.data) >= 262153}
    for e in lzcases.BIG_ONLY_EVENTS:
        assert set(where[e]) <= big, e
    # the sharper forms some seams were built for
    assert where["bwd_end_ref_lt8_after_8"] and where["inv_copy_far_long"] and where["inv_copy_near_long"]


def test_recoded_and_edited_frames():
    """the 4-byte length code in the match-length stream, which no forward pass writes: a frame recoded by hand decodes to the same
    bytes, in the model and in the oracle.  And the edited frames of lzcases.surgery: the reference's decoder ends on each, refusing
    all but the one whose distance stays inside the window."""
    small, big = (_by_name()[n] for n in lzcases.SURGERY_CASES)
    for codec in ("LZ", "LZX"):
        frame = _oracle(small.name, codec)[1]
        recoded = lzcases.recode_mlen_4byte(frame)
        iv = collections.Counter()
        assert len(recoded) == len(frame) + 1 and katmodels.lz_decode(recoded, len(small.data), iv) == small.data and iv["inv_mlen_code_4byte"] == 1
        assert oracle.transform_inverse(codec, recoded, len(small.data)) == (True, small.data)
        verdicts = {}
        for label, bad in lzcases.surgery(frame, _oracle(big.name, codec)[1]):
            cap = len(big.data) if "window" in label else len(small.data)
            verdicts[label] = oracle.transform_inverse(codec, bad, cap)[0]
        assert len(verdicts) == 6 and not any(v for k, v in verdicts.items() if k != "distance maxDist in the small window"), verdicts


@pytest.mark.parametrize("mutant", katmodels.LZ_MUTANTS)
def test_mutants_are_caught(mutant):
    """(e) each mutant of the model -- a shortcut of k_lz_fwd going wrong in one line -- changes the bytes of at least one case"""
    caught = []
    for c in sorted(lzcases.cases(), key=lambda c: len(c.data)):
        for codec in c.codecs:
            ok, enc, ev, iv = _traces()[c.name, codec]
            try:
                got = katmodels.lz_forward(c.data, codec == "LZX", c.dtype, mutate=mutant)
            except (katmodels.JavaException, IndexError):
                got = None
            if got != (ok, enc):
                caught.append((c.name, codec))
        if caught:
            break
    assert caught, mutant
