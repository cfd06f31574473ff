"""kz_knz_splice (host memory, no GPU) on the case set of tests/knzsplice.py, against the Python model of a splice,
knz_assemble([extract_bits ...]), and against the streams and the data each plan stands for; its refusals; and the coverage the
set is meant to have, computed from the plans.  Streams are built by the oracle.  The texts of the refusals belong to the device
form, which has a context to keep them in (tests/test_gpu_knz_splice.py); here the codes are checked, and that dst stays as it was."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import knzrange
import knzsplice as ks
import oracle


def _compress(chain, ent, bs, data, checksum):
    return oracle.compress(chain, ent, bs, data, jobs=2, checksum=checksum)


def _encode_block(chain, ent, bs, block, checksum):
    s, w, _, _ = oracle.encode_block(chain, ent, block, checksum=checksum, block_size=bs)
    return s, w


@pytest.fixture(scope="module")
def cases(built):
    return ks.cases(_compress, _encode_block)


@pytest.fixture(scope="module")
def results(cases):
    """name -> the result of kz_knz_splice with the bound as capacity"""
    return {c.name: splice(c, ks.bound(c))[1] for c in cases}


def splice(case, cap, **override):
    """kz_knz_splice of a case into a poisoned destination of cap bytes (16 more behind it) -> (rc, dst[0 .. max(rc, 0)), all of dst)"""
    L = kz.load_library()
    src, offs = ks.pack(case.sources)
    dst = np.full(max(cap, 0) + 16, ks.POISON, dtype=np.uint8)
    rc = ks.call(L.kz_knz_splice, (), src.ctypes.data, offs, case.lens, case.pieces, case.input_size, dst.ctypes.data, cap, **override)
    return rc, dst[:max(rc, 0)].tobytes(), dst


def test_the_binding_declares_the_three_calls(built):
    L = ctypes.CDLL(kz.LIB_PATH)
    for name in ("kz_knz_splice_bound", "kz_knz_splice", "kz_knz_splice_device"):
        assert name in kz.ABI_SYMBOLS and hasattr(L, name), name
    for name in ("knz_splice", "knz_splice_device", "knz_splice_bound", "splice_concat", "splice_slice", "splice_replace"):
        assert hasattr(kz, name), name
    assert kz.load_library().kz_abi_version() == 3


def test_every_result_is_the_model(cases):
    for c in cases:
        cap = ks.bound(c)
        rc, got, dst = splice(c, cap)
        want = ks.model(c)
        assert rc == len(want) and got == want, (c.name, rc, len(want))
        assert rc <= cap, (c.name, rc, cap)
        assert bool((dst[rc:] == ks.POISON).all()), (c.name, "bytes behind the stream")
        # dstCap exact succeeds, one byte less is refused and nothing is written
        rc2, got2, dst2 = splice(c, rc)
        assert rc2 == rc and got2 == want and bool((dst2[rc:] == ks.POISON).all()), (c.name, "exact capacity")
        rc3, _, dst3 = splice(c, rc - 1)
        assert rc3 == -12 and bool((dst3 == ks.POISON).all()), (c.name, "one byte less", rc3)


def test_results_equal_the_streams_they_stand_for(cases, results):
    stated = [c for c in cases if c.equals is not None]
    kinds = {c.name.split("-", 2)[-1] for c in stated}
    assert {"identity", "slice-2+3", "slice-4+9", "replace-1", "append", "concat-whole"} <= kinds, kinds
    for c in stated:
        assert results[c.name] == c.equals, c.name


def test_results_decode_to_the_blocks_they_name(cases, results):
    stated = [c for c in cases if c.decoded is not None]
    assert any("reverse" in c.name for c in stated) and any("repeats" in c.name for c in stated) and any("interleave-3" in c.name for c in stated)
    assert any("concat-ragged" in c.name for c in stated)
    for c in stated:
        assert oracle.decompress(results[c.name], len(c.decoded) + 16) == c.decoded, c.name


def test_no_pieces_give_header_and_end_marker(cases, results):
    empties = [c for c in cases if not c.pieces]
    assert len(empties) == len(ks.SETTINGS)
    for c in empties:
        idx = kz.knz_index(results[c.name])
        src = ks.head(c.sources[0])
        assert idx["blocks"] == [] and len(results[c.name]) == 21 and results[c.name][20] == 0, c.name
        assert {k: idx[k] for k in ("transform", "entropy", "blockSize", "checksum")} == {k: src[k] for k in ("transform", "entropy", "blockSize", "checksum")}


def test_header_parameters_are_carried_over(cases, results):
    seen = set()
    for c in cases:
        idx, src = kz.knz_index(results[c.name]), ks.head(c.sources[0])
        assert (idx["transform"], idx["entropy"], idx["blockSize"], idx["checksum"]) == (src["transform"], src["entropy"], src["blockSize"], src["checksum"]), c.name
        assert idx["inputSize"] == c.input_size and [w for _, w in idx["blocks"]] == c.bits(), c.name
        seen.add(idx["checksum"])
    assert seen == {0, 32, 64}


def test_the_python_form_and_the_planners(cases):
    for c in cases:
        if c.lens == [len(s) for s in c.sources]:
            assert kz.knz_splice(c.sources, c.pieces, c.input_size) == ks.model(c), c.name
    # sizes: known where every block but the last is whole, unknown (0) otherwise
    chain, ent, bs, chk = ks.SETTINGS[0]
    D = ks._data(bs, 3, 10)
    idx = kz.knz_index(_compress(chain, ent, bs, D, chk))
    assert kz.splice_slice(idx, 1, 2)[1] == 2 * bs and kz.splice_slice(idx, 2, 5)[1] == bs + 10 and kz.splice_slice(idx, 4, 2) == ([], 0)
    assert kz.splice_concat([idx, idx])[1] == 2 * len(D)
    short = kz.knz_index(_compress(chain, ent, bs, D[:7], chk))
    assert kz.splice_replace(idx, 3, 1, short)[1] == 3 * bs + 7 and kz.splice_replace(idx, 4, 1, short)[1] == 0      # (an append behind a short block)
    assert kz.splice_replace(idx, 1, 1, short)[1] == 0                                                                 # a short block in the middle
    nosize = dict(idx, inputSize=0)
    assert kz.splice_concat([idx, nosize])[1] == 0 and kz.splice_slice(nosize, 0, 2)[1] == 0
    with pytest.raises(IndexError):
        kz.splice_replace(idx, 5, 1, short)
    with pytest.raises(kz.KanziError) as e:
        kz.knz_splice([_compress(chain, ent, bs, D, chk)], [(0, 5, 5)], 0)
    assert e.value.code == 18
    assert kz.knz_splice_bound([]) == 27 and kz.knz_splice_bound([9]) == 26 + 4
    with pytest.raises(kz.KanziError):
        kz.knz_splice_bound([-1])


def test_refusals(built):
    refs, base = ks.refusals(_compress)
    assert splice(base, ks.bound(base))[0] > 0                                  # the calls the refusals are made from succeed
    assert {r.code for r in refs} >= {-18, -12, -15, -16, -3, -2, -19}
    for r in refs:
        cap = ks.bound(base) if r.cap is None else r.cap
        rc, _, dst = splice(r.case, cap, **r.override)
        assert rc == r.code, (r.name, rc, r.code)
        assert bool((dst == ks.POISON).all()), (r.name, "dst written")


def test_coverage_of_the_case_set(cases):
    cov = ks.coverage(cases)
    assert cov["phase pairs"] == 64, cov
    for k in ("three pieces in a unit", "three payloads of real blocks in a unit", "unit inside a payload", "last bits of a source", "W >= 2^16", "seam inside a byte", "seam on a byte"):
        assert cov[k], (k, cov)
    # blocks of 1 to 5 data bytes, assembled as knzrange.Stream(lens=...) does
    tiny = [c for c in cases if c.name.startswith("tiny")]
    assert tiny and all(max(c.bits()) <= 8 * 8 for c in tiny)
    # the cut source ends with its last piece's last bit, and behind it nothing is the caller's
    (lb,) = [c for c in cases if c.name == "last-bits"]
    assert max(off + w for _, off, w in lb.pieces) == 8 * lb.lens[0] == 8 * len(lb.sources[0])
