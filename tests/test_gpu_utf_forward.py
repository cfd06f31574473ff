"""The device UTF forward (kanzi_amd/csrc/kz_utf_fwd_gpu.hip) against the oracle on the deterministic case set of tests/utfcases.py
(checked on the CPU by tests/test_utf_cases.py): every batch goes through kz_encode_blocks with the device TEXT forward on, so the
blocks TEXT declines as UTF8 reach k_uf_*.  Per block: status, bits, skip flags, length and stream bytes are oracle.encode_block's,
and kz_decode_blocks returns what oracle.decode_block returns for that stream.  Per batch: the "[utffwd] took A blocks, finished D,
declined N" trace line equals the counts utfcases.expected_class gives (the host stage's share is A - D - N), so a path that did not
run fails the test.  With KZ_UTF_FWD_GPU=0 the streams are the same and the line is absent."""
import functools

import numpy as np
import pytest
import torch

import kanzi_amd as kz
import oracle
import utfcases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return kz.Context(0)


@pytest.fixture(autouse=True)
def device_text_forward(ctx, monkeypatch):
    monkeypatch.setenv("KZ_TEXT_FWD_GPU", "1")
    monkeypatch.setenv("KZ_TEXT_GPU_TRACE", "1")
    monkeypatch.delenv("KZ_UTF_FWD_GPU", raising=False)           # (conftest.py: the live contexts read the switches again)


@functools.lru_cache(maxsize=None)
def _want(chain, ent, block, bs):
    so, w, sf, pl = oracle.encode_block(chain, ent, block, block_size=bs)
    r, back = oracle.decode_block(chain, ent, bs, so, w, bs)
    return so, w, sf, pl, r, back


def _trace(err):
    return [(int(x[2]), int(x[5].rstrip(",")), int(x[7])) for x in (l.split() for l in err.splitlines() if l.startswith("[utffwd] took"))]


def _expected_trace(cases):
    cls = [utfcases.expected_class(c.block) for c in cases if c.kind == "taken"]
    return [(len(cls), cls.count("finish"), cls.count("decline"))] if cls else []


def _encode(ctx, capfd, cases, chain, ent, device=False):
    """one kz_encode_blocks call -> (results, output rows, the [utffwd] lines it printed)"""
    bs = cases[0].bs
    B = len(cases)
    ctx.set_block_size(bs)
    inp = np.zeros((B, bs), dtype=np.uint8)
    lens = np.array([len(c.block) for c in cases], dtype=np.int32)
    for i, c in enumerate(cases):
        inp[i, :len(c.block)] = np.frombuffer(c.block, dtype=np.uint8)
    ostride = kz.max_block_stream_bytes(bs)
    capfd.readouterr()
    if device:
        d_in = torch.from_numpy(inp).cuda()
        d_out = torch.zeros((B, ostride), dtype=torch.uint8, device="cuda")
        res = kz.encode_blocks(ctx, chain, ent, d_in.data_ptr(), bs, lens, d_out.data_ptr(), ostride, kz.MEM_DEVICE)
        out = d_out.cpu().numpy()
    else:
        out = np.zeros((B, ostride), dtype=np.uint8)
        res = kz.encode_blocks(ctx, chain, ent, inp, bs, lens, out, ostride)
    return res, out, _trace(capfd.readouterr().err)


def _check(ctx, capfd, cases, chain, ent, device=False):
    bs = cases[0].bs
    res, out, lines = _encode(ctx, capfd, cases, chain, ent, device)
    for i, c in enumerate(cases):
        so, w, sf, pl, _, _ = _want(chain, ent, c.block, bs)
        if not c.block:                                             # no stream, and no transform ran: kz_encode_blocks reports every skip bit set, the oracle none
            assert (w, pl) == (0, 0)
            sf = 0xFF
        assert res[i].status == 0 and (res[i].bits, res[i].skipFlags, res[i].length) == (w, sf, pl), (chain, ent, c.label)
        assert out[i, :(w + 7) // 8].tobytes() == so, (chain, ent, c.label)
    assert lines == _expected_trace(cases), (chain, ent)
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(cases), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, chain, ent, bs, np.ascontiguousarray(out), out.shape[1], bits, dec, bs)
    for i, c in enumerate(cases):
        _, _, _, _, r, back = _want(chain, ent, c.block, bs)
        if not c.block:                                             # (nothing to give the oracle's decoder)
            assert res2[i].status == 0 and res2[i].length == 0, (chain, ent, c.label)
            continue
        if r < 0:
            assert res2[i].status != 0, (chain, ent, c.label)
            continue
        assert res2[i].status == 0 and res2[i].length == r and dec[i, :r].tobytes() == back, (chain, ent, c.label)
    return res, out


def _check_host_utf_is_the_same(ctx, capfd, monkeypatch, cases, chain, ent, res, out):
    monkeypatch.setenv("KZ_UTF_FWD_GPU", "0")
    res0, out0, lines = _encode(ctx, capfd, cases, chain, ent)
    assert lines == []
    for i, c in enumerate(cases):
        assert (res0[i].status, res0[i].bits, res0[i].skipFlags, res0[i].length) == (res[i].status, res[i].bits, res[i].skipFlags, res[i].length), c.label
        assert np.array_equal(out0[i, :(res[i].bits + 7) // 8], out[i, :(res[i].bits + 7) // 8]), c.label


@pytest.mark.parametrize("name", [n for n in sorted(utfcases.batches()) if n not in utfcases.MIXED])
def test_case_classes(ctx, capfd, monkeypatch, name):
    """one class of the case set per batch, TEXT+UTF & NONE: the symbol-count bands (alias width, the sort's padding, UF_MAXSYM and
    the host stage above it), the order of the map under ties, code points over thread / wave / tile seams, the lengths (UF_MIN_BLOCK,
    one tile and its neighbours, 256 and 257 tiles, 2 MiB + 12345), start and adjust, the three decline exits on both sides, the
    walk-breaking bytes, four-unit code points, 300 small blocks"""
    cases = utfcases.batches()[name]
    res, out = _check(ctx, capfd, cases, "TEXT+UTF", "NONE")
    _check_host_utf_is_the_same(ctx, capfd, monkeypatch, cases, "TEXT+UTF", "NONE", res, out)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("chain,ent", [("TEXT+UTF", "NONE"), ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0")])
@pytest.mark.parametrize("name", utfcases.MIXED)
def test_mixed_batches(ctx, capfd, monkeypatch, name, chain, ent, device):
    """taken blocks between English prose, binary, a 15-byte copy block, an empty block and 1023 bytes of UTF-8, which the device UTF
    forward must not touch; the longest block (maxTiles follows the longest TAKEN one) is a prose block in one batch and a taken one
    in the other; host and device-resident buffers"""
    cases = utfcases.batches()[name]
    res, out = _check(ctx, capfd, cases, chain, ent, device)
    if not device:
        _check_host_utf_is_the_same(ctx, capfd, monkeypatch, cases, chain, ent, res, out)


def test_four_unit_verdict_survives_many_tiles(ctx, capfd):
    """48 blocks of 512 KiB (128 tiles each, 6144 workgroups in k_uf_pass<0>: late ones start while early ones write), valid UTF-8
    with mostly three-unit code points and one four-unit code point each, in the first, the middle or the last tile; encoded three
    times.  Every stream is the oracle's with UTF applied (by the host stage), and each call's trace says 48 taken, 0 finished, 0
    declined.

    What is true of this test: k_uf_pass<0> used to leave on info[2], a word that other workgroups of the same launch write, so
    waves of one workgroup could disagree, the ones that stayed parsed a half-loaded tile, and their plain store of the "bad" bit
    erased the four-unit bit -- the block was then reported declined and its stream was no longer the reference's.  That is a race:
    this test can pass on the old code, and a failure is always a real one.  The fix stands on reading the code (the exit tests
    info[6], which only earlier launches write; the "bad" bit is set with atomicOr), not on this test."""
    blocks, bs = utfcases.race_batch()
    cases = [utfcases.Case("block %d" % i, b, bs, "taken") for i, b in enumerate(blocks)]
    for c in cases:
        so, w, sf, pl, _, _ = _want("TEXT+UTF", "NONE", c.block, bs)
        assert (sf & 0x40) == 0 and pl < bs - bs // 10                  # the oracle applied UTF (the second transform's skip bit is clear)
    for run in range(3):
        res, out, lines = _encode(ctx, capfd, cases, "TEXT+UTF", "NONE")
        assert lines == [(48, 0, 0)], run
        for i, c in enumerate(cases):
            so, w, sf, pl, _, _ = _want("TEXT+UTF", "NONE", c.block, bs)
            assert res[i].status == 0 and (res[i].bits, res[i].skipFlags, res[i].length) == (w, sf, pl), (run, i)
            assert out[i, :(w + 7) // 8].tobytes() == so, (run, i)
