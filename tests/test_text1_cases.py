"""tests/text1cases.py against the two CPU references of TextCodec1's forward: the oracle's C port and the Python model written from
the Java (tests/katmodels.py).  Every case has the same verdict, bytes and "dataType" entry in both, does what its name says, and
every case marked for the device lies inside what the device form accepts (kz_text_fwd_gpu.hip)."""
import pytest

import katmodels
import oracle
import text1cases
from test_oracle import _text_static_words

SIZES = (32768, 1 << 20, 4 << 20)
_CACHE = {}


def _cases(bs):
    if bs not in _CACHE:
        _CACHE[bs] = text1cases.cases(bs)
    return _CACHE[bs]


def _ids():
    return [(bs, i) for bs in SIZES for i in range(len(_cases(bs)))]


class _Learns:
    """counts the words TextCodec1 / 2 learn in the model's walk, and whether the word list wrapped: the model asks expand() every
    time the next number reaches the list's size, and restarts the numbering when expand() refuses at 2^19"""

    def __init__(self, monkeypatch):
        self.sizes, self.wrapped = [], False
        real = katmodels._TextCodecModel.expand
        me = self

        def expand(m):
            me.sizes.append(m.dict_size)
            r = real(m)
            me.wrapped |= not r
            return r

        monkeypatch.setattr(katmodels._TextCodecModel, "expand", expand)


def _words(out):
    """(escape byte, word number, bytes of the number) of every reference in a TextCodec1 output"""
    i, refs = 1, []
    while i < len(out):
        c = out[i]
        i += 1
        if c not in (0x0E, 0x0F):
            continue
        v, k = out[i], 1
        if v >= 128:
            v &= 0x7F
            b2 = out[i + 1]
            k = 2
            if b2 & 0x80:
                v = ((v & 0x1F) << 7) | (b2 & 0x7F)
                b2 = out[i + 2] & 0x7F
                k = 3
            v = (v << 7) | b2
        i += k
        refs.append((c, v, k))
    return refs


@pytest.mark.parametrize("bs,i", _ids(), ids=lambda v: str(v))
def test_case_against_oracle_and_model(built, bs, i, monkeypatch):
    c = _cases(bs)[i]
    d = c.block
    sd = katmodels.text_static_dictionary(_text_static_words())
    tag = text1cases.writer_tag(d)
    learns = _Learns(monkeypatch)
    ok_m, out_m, dt_m = katmodels.text_forward(d, 1, bs, sd, tag)
    oracle.set_transform_ctx("FPAQ", bs)
    ok_o, out_o, dt_o = oracle.transform_forward("TEXT", d, data_type=oracle.DT[tag])
    if len(d) < 1 << 18 or c.name in ("big_ragged_english", "big_utf8", "big_random"):   # (the Python model takes seconds per MiB: TextCodec2 from it for the small blocks and three large ones)
        sd2 = katmodels.text_static_dictionary(_text_static_words())
        ok2, out2, dt2 = katmodels.text_forward(d, 2, bs, sd2, tag)
    else:
        oracle.set_transform_ctx("ANS0", bs)
        ok2, out2, dt2 = oracle.transform_forward("TEXT", d, data_type=oracle.DT[tag])
        dt2 = katmodels._DATA_TYPES[dt2]
    oracle.set_transform_ctx("NONE", 4 << 20)
    assert (ok_m, oracle.DT[dt_m]) == (ok_o, dt_o), (c, ok_m, ok_o, dt_m, dt_o)
    if ok_o:
        assert out_m == out_o, (c, len(out_m), len(out_o))
        assert out_o[0] & 0x10 == 0                                                   # the mode byte without the codec bit
    n = len(d)
    strict_text = not (katmodels.text_compute_stats(d, True)[0] & 0x80) if n else False
    if c.device:
        assert strict_text and katmodels.magic_type(d) == 0 and 1024 <= n < (1 << 24), c
        assert ok_o and len(out_o) <= n - 8, (c, len(out_o))
        assert not learns.wrapped and (1 << 19) not in learns.sizes, (c, learns.sizes)   # the word numbers never reached 2^19
    else:
        assert c.why, c
    # ---- the case does what its name says ----
    refs = _words(out_o) if ok_o else []
    nm = c.name
    if nm == "capitalised_words":
        assert sum(1 for r in refs if r[0] == 0x0E) > len(refs) // 2
    if nm.startswith("esc_at_seams") or nm.startswith("esc_around") or nm.endswith("last_byte") or nm == "esc_every_12th":
        lit = sum(1 for r in refs if r[1] in (1024, 1025)) if ok_o else d.count(0x0E) + d.count(0x0F)
        assert lit == d.count(0x0E) + d.count(0x0F) and lit > 0 and all(r[2] == 2 for r in refs if r[1] in (1024, 1025))
    if nm in ("ascii_at_the_edge", "ascii_past_the_edge"):
        ascii_ = sum(1 for x in d if x < 128)
        assert (ascii_ // 95 == n // 100) == (nm == "ascii_at_the_edge") and (ascii_ + (nm != "ascii_at_the_edge")) // 95 == n // 100
        assert ok_o == (nm == "ascii_at_the_edge") and ok2
    if nm in ("nuls_below_1_percent", "nuls_at_1_percent"):
        assert d.count(0) == n // 100 - (nm == "nuls_below_1_percent") and ok_o == (nm == "nuls_below_1_percent") and ok2
    if nm == "lf_for_spaces":
        assert ok_o and not ok2 and d.count(b" ") == 0
    if nm == "pk_magic_english":
        assert tag == "BIN" and ok_o and dt_m == "TEXT" and not ok2
    if nm == "bm_magic_english":
        assert tag == "MULTIMEDIA" and not ok_o and dt_m == "MULTIMEDIA"
    if nm.startswith("slot0_word"):
        W = text1cases.SLOT0[13 if bs == 32768 else 17]
        assert text1cases.word_hash(W) & ((1 << (13 if bs == 32768 else 17)) - 1) == 0 and 5 <= len(W) <= 8
        assert W == text1cases.slot0_word(13 if bs == 32768 else 17) or bs != 32768
        head1, head2 = out_o[1:1 + 8 * len(W) + 24], out2[1:1 + 8 * len(W) + 24]
        if nm == "slot0_word_first":
            # TextCodec1: the escape word holds slot 0, nothing is learned: six times plain; TextCodec2 learns W at once: five references
            assert out_o[1:1 + 6 * (len(W) + 1)] == (b" " + W) * 6 and head2.count(W) == 1
        else:
            # another word was learned first: slot 0 is free, W is learned at its first occurrence under both codecs
            assert head1.count(W) == 1 and head2.count(W) == 1
    if nm == "many_words":
        ks = [r[2] for r in refs]
        assert ks.count(1) > 0 and ks.count(2) > 0 and ks.count(3) > 0, (ks.count(1), ks.count(2), ks.count(3))
        assert max(r[1] for r in refs) >= 16384
    if nm in ("esc_every_4th",) or (nm == "esc_every_12th" and bs == 32768):
        assert not ok_o and strict_text                                                # text, and the output outgrows the block
    if nm == "len_1023" or nm == "len_15" or nm == "spaces_only":
        assert not ok_o
    if nm == "big_many_words":
        assert learns.sizes[-1] == 1 << 17 and len(d) - len(out_o) == 2265                 # the list grew to 2^18 entries, no wrap
        a, b = text1cases.COLLIDE                                                        # what keeps it from the device: one hash, one length
        assert text1cases.word_hash(a) == text1cases.word_hash(b) and len(a) == len(b) and b" " + a + b" " in d and b" " + b + b" " in d


def test_the_case_set_is_what_the_device_tests_expect():
    for bs in SIZES:
        cs = _cases(bs)
        assert len({c.name for c in cs}) == len(cs)
        assert sum(c.device for c in cs) >= (6 if bs == 4 << 20 else 15)
        assert all(c.device or c.why for c in cs)
