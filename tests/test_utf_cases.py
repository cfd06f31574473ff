"""The case set of tests/utfcases.py against the oracle and katmodels.utf_forward, on the CPU: every case is what its label says (TEXT
declines it as UTF8, or leaves the stated other type), the oracle and the model agree on every taken block, and the set reaches what
it was built for -- read from the oracle's output header or from the walk, never from a label.  tests/test_gpu_utf_forward.py runs
the same batches through kanzi_amd/csrc/kz_utf_fwd_gpu.hip."""
import collections
import functools

import numpy as np
import pytest

import katmodels
import oracle
import utfcases

UTF8 = oracle.DT["UTF8"]


def _unique_taken():
    seen = {}
    for cases in utfcases.batches().values():
        for c in cases:
            if c.kind == "taken":
                seen.setdefault(c.block, c.label)
    return seen


@functools.lru_cache(maxsize=None)
def _oracle_utf(block):
    return oracle.transform_forward("UTF", block, data_type=UTF8)


def test_every_case_is_what_its_label_says():
    """TEXT declines every taken case and leaves UTF8 (so kz_encode_blocks hands it to the device UTF forward); the other cases keep
    the type their label states, which is not UTF8"""
    n = 0
    for name, cases in utfcases.batches().items():
        assert len({c.bs for c in cases}) == 1 and max(len(c.block) for c in cases) <= cases[0].bs, name
        for c in cases:
            oracle.set_transform_ctx("NONE", c.bs)
            ok, _, dt = oracle.transform_forward("TEXT", c.block, data_type=0)
            if c.kind == "taken":
                assert len(c.block) >= 1024 and not ok and dt == UTF8, (name, c.label, ok, dt)
            else:
                assert c.kind != "UTF8" and dt == oracle.DT[c.kind] and ok == (c.kind == "TEXT" or not c.block), (name, c.label, ok, dt)
            n += 1
    assert n == sum(len(v) for v in utfcases.batches().values())
    blocks, bs = utfcases.race_batch()
    oracle.set_transform_ctx("NONE", bs)
    for i, b in enumerate(blocks):
        ok, _, dt = oracle.transform_forward("TEXT", b, data_type=0)
        assert len(b) == bs and not ok and dt == UTF8, i


@pytest.mark.parametrize("name", sorted(utfcases.batches()))
def test_oracle_and_model_agree(name):
    """verdict and bytes of oracle/kzo_utf.c and katmodels.utf_forward on every taken block; the walk of utfcases.analyse gives the
    same verdict, header and length"""
    for c in utfcases.batches()[name]:
        if c.kind != "taken":
            continue
        ok_o, enc_o, dt_o = _oracle_utf(c.block)
        ok_m, enc_m, dt_m = katmodels.utf_forward(c.block, "UTF8")
        assert ok_o == ok_m and dt_o == UTF8 and dt_m == "UTF8", c.label
        a = utfcases.analyse(c.block)
        assert ok_o == (a["exit"] is None), (c.label, a)
        if ok_o:
            assert enc_o == enc_m, c.label
            assert (enc_o[0], enc_o[1], (enc_o[2] << 8) | enc_o[3], len(enc_o)) == (a["start"], a["adjust"], a["ns"], a["outlen"]), c.label
        cls = utfcases.expected_class(c.block)
        assert not (cls == "finish" and not ok_o) and not (cls == "decline" and ok_o), (c.label, cls)


def _applied_headers():
    """(start, adjust, ns) from the output header of every taken block the oracle applies UTF to"""
    out = {}
    for block, label in _unique_taken().items():
        ok, e, _ = _oracle_utf(block)
        if ok:
            out[label] = (e[0], e[1], (e[2] << 8) | e[3])
    return out


def test_reach_symbol_bands_front_and_tail():
    heads = _applied_headers()
    ns = {h[2] for h in heads.values()}
    applied_bands = [n for n in utfcases.BAND_NS if n < 32768]
    assert set(applied_bands) <= ns, sorted(set(applied_bands) - ns)
    # 32768 symbols: the reference's loop stops at the 32768th (:153); the walk counts them
    a = [utfcases.analyse(b) for b, l in _unique_taken().items() if l == "band ns=32768"]
    assert len(a) == 1 and a[0]["ns"] == 32768 and a[0]["ref_stop"] == "n32768"
    assert {h[0] for h in heads.values()} == {0, 1, 2, 3, 4}          # 4: four continuation bytes in front (the header byte the inverse masks)
    assert {h[1] for h in heads.values()} == {0, 1, 2, 3}
    by = {l: b for b, l in _unique_taken().items()}
    assert by["byte order mark"][:3] == b"\xef\xbb\xbf" and heads["byte order mark"][0] == 3
    assert "byte order mark, continuation byte" not in heads
    assert heads["adjust 2: three units from n - 5"][1] == 2


def test_reach_decline_exits_on_both_sides():
    a = {l: utfcases.analyse(b) for b, l in _unique_taken().items() if l.startswith("exit ")}
    assert len(a) == len(utfcases.EXITS)
    margin_map = sorted(3 * x["ns"] + 6 - x["max_target"] for x in a.values() if x["max_target"] == 924)
    assert margin_map == [-3, 0, 3]
    assert [x["exit"] for x in a.values() if x["max_target"] == 924] == ["length", "map", "map"]
    est = sorted((x["estimate"] - x["max_target"], x["exit"]) for l, x in a.items() if l.startswith("exit estimate"))
    assert est == [(-1, "length"), (0, "estimate"), (1, "estimate")]
    ln = sorted((x["outlen"] - x["max_target"], x["exit"], x["adjust"]) for l, x in a.items() if l.startswith("exit length"))
    # - 1 applies; + 0 and + 2 pass the early test of map + aliases + one tail byte and are declined once written (k_uf_scan); + 3 is
    # declined before (k_uf_syms)
    assert ln == [(-1, None, 0), (0, "length", 0), (2, "length", 0), (3, "length", 0)]
    for l, x in a.items():
        assert (x["exit"] is None) == _oracle_utf({v: k for k, v in _unique_taken().items()}[l])[0], l


def test_reach_classes_and_ties():
    """how many taken blocks of each class the batches hold (a property of the builder alone), and the tie at the alias step"""
    count = {}
    for name, cases in utfcases.batches().items():
        count[name] = collections.Counter(utfcases.expected_class(c.block) for c in cases if c.kind == "taken")
    total = sum(count.values(), collections.Counter())
    assert set(total) == {"finish", "decline", "host"}
    assert count["bands big"] == {"finish": 2, "host": 4}              # 16385, 20000, 32767 apply on the host; 32768 the host declines
    assert count["four units"] == {"host": 3, "decline": 2}
    assert count["exits"] == {"finish": 1, "decline": 9}
    assert count["mutations"] == {"decline": 9}
    assert count["seams"] == {"finish": 8} and count["lengths big"] == {"finish": 3}
    for name in utfcases.MIXED:
        assert min(count[name][k] for k in ("finish", "decline", "host")) >= 2, (name, count[name])
        cases = utfcases.batches()[name]
        longest = max(cases, key=lambda c: len(c.block))
        assert (longest.kind == "taken") == (name == "mixed, longest taken")
        assert {len(c.block) for c in cases if c.kind != "taken"} >= {0, 15, 1023}
    assert len(utfcases.batches()["many small"]) == 300 and min(count["many small"][k] for k in ("finish", "decline", "host")) >= 5
    tie = [l for b, l in _unique_taken().items() if utfcases.analyse(b)["c127"] is not None and utfcases.analyse(b)["c127"] == utfcases.analyse(b)["c128"] and _oracle_utf(b)[0]]
    assert "flat: 600 symbols x 8" in tie and "two levels: 127 symbols x 9, the rest x 6" in tie
    step = utfcases.analyse({l: b for b, l in _unique_taken().items()}["two levels: 128 symbols x 9, the rest x 6"])
    assert (step["c127"], step["c128"], step["exit"]) == (9, 6, None)


def test_race_batch():
    blocks, bs = utfcases.race_batch()
    assert len(blocks) == 48 and bs == 512 << 10
    for i, b in enumerate(blocks):
        v = np.frombuffer(b, dtype=np.uint8)
        at = np.flatnonzero(v >= 0xF0)
        assert len(at) == 1 and int(at[0]) // utfcases.TILE == (0, 64, 127)[i % 3], i
        assert int(np.count_nonzero(v >= 0xE0)) > bs // 8                # many three-unit code points
        ok, e, _ = _oracle_utf(b)
        assert ok and (e[2] << 8 | e[3]) > 128, i                         # valid: the reference applies UTF (on the device: the host stage)
    for b in blocks[:3]:
        assert utfcases.expected_class(b) == "host"
