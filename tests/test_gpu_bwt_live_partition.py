"""The bucket partition of the forward BWT's doubling rounds straight from the rank array (k_live_hist / k_live_scatter,
kz_bwt_fwd.hip) against the text-order list it replaces (KZ_BWT_LIVEPART=0: k_live_emit, k_msd_hist, k_msd_scatter) and against the
oracle: the BWT is unique, so both paths must give the oracle's bytes.  The path needs a round that starts with at least 4096 live
suffixes in some block of the call; the shapes are the smallest that put the seams of the two kernels under it: ragged last sort
tiles (16384 text positions) and sub-tiles (4096), dead sub-tiles and a dead sort tile, keys past the end of the text, an oversized
bucket next to small ones, blocks whose round 0 stored no ranks, and a batch whose grid thins between the rounds."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import datagen
import oracle

pytestmark = pytest.mark.gpu


def _fwd(ctx, tid, data):
    cap = ctx.lib.kz_transform_max_encoded_len(tid, len(data))
    out = np.zeros(cap + 64, dtype=np.uint8)
    p = ctypes.c_int32(0)
    a = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    rc = ctx.lib.kz_transform_forward(ctx.h, tid, a.ctypes.data, len(data), out.ctypes.data, cap, ctypes.addressof(p))
    assert rc >= 0, ctx.error()
    assert not out[cap:].any(), "kz_transform_forward wrote behind dstCap"
    return rc == 1, out[:p.value].tobytes()


BOTH = ["unset", "0"]
_rng = np.random.default_rng(77)
NOISE = _rng.integers(0, 256, 300001, dtype=np.uint8).tobytes()


def _planted(n, length, at):
    """noise of n bytes with the same `length` random bytes at every position of `at`: only those suffixes stay live after round 0"""
    a = np.frombuffer(NOISE[:n], dtype=np.uint8).copy()
    rep = np.frombuffer(NOISE[200000:200000 + length], dtype=np.uint8)
    for p in at:
        a[p:p + length] = rep
    return a.tobytes()


def _twice(nchunks, clen, seed):
    """`nchunks` random chunks of `clen` bytes, then the same chunks in another order: every suffix is live after round 0 and
    matches run for up to clen bytes (and a little more by chance): clen = 300 keeps the block in the rounds up to h = 192"""
    r = np.random.default_rng(seed)
    c = r.integers(0, 256, (nchunks, clen), dtype=np.uint8)
    return c.reshape(-1).tobytes() + c[r.permutation(nchunks)].reshape(-1).tobytes()


def _inputs():
    ins = {}
    for n in (65536, 65537, 81920 + 1, 3 * 16384 - 1):               # ragged last sort tile / last sub-tile
        ins["noise3-%d" % n] = datagen.block(3, n, 3).tobytes()
        ins["text-%d" % n] = datagen.block(0, n, 0).tobytes()
        ins["ab-%d" % n] = (b"ab" * (n // 2 + 1))[:n]
        ins["abc-%d" % n] = np.random.default_rng(n).integers(97, 100, n, dtype=np.uint8).tobytes()
    # live suffixes only in the last sub-tile of a sort tile and the first of the next one, twice (6000 >= 4096: the bucket path)
    ins["straddle"] = _planted(6 * 16384, 6000, (2 * 16384 - 3000, 4 * 16384 - 3000))
    # noise, repeat, noise: the sort tiles 2 and 3 hold no live suffix
    ins["dead-tile"] = _planted(6 * 16384 + 5, 8192, (16384 + 100, 4 * 16384 + 100))
    # keys past the end of the text: the block ends in a run longer than h = 6, 12, 24, ... (the n - s branch in several rounds)
    ins["zeros-then-1"] = bytes(99999) + b"\x01"
    ins["ff-run-noise"] = b"\xff" * 150000 + NOISE[:50000]
    ins["noise-ff-run"] = NOISE[:50000] + b"\xff" * 150000
    # one oversized bucket (BK_BIG: the window, through the key trie round or the LSD passes) next to small ones
    ins["zeros-300000"] = bytes(300000)
    ins["zeros-in-text"] = datagen.block(0, 100000, 0).tobytes() + bytes(120000) + datagen.block(0, 42147, 0).tobytes()
    # lazy ranks: round 0 with and without stored ranks
    ins["lazy-twice"] = NOISE[:150000] * 2
    ins["lazy-tail7"] = NOISE[:262147] + NOISE[:7]
    return ins


def _batch():
    """9 blocks of one call, 64 KiB .. 1 MiB and two short ones: two are done after round 0, two stay to h = 192"""
    return [datagen.block(0, 1 << 20, 0).tobytes(), NOISE[:65536], _twice(250, 300, 1), b"", datagen.block(3, 100000, 3).tobytes(),
            _twice(437, 300, 2), b"short block", _planted(6 * 16384, 6000, (2 * 16384 - 3000, 4 * 16384 - 3000)), bytes(300000)]


@pytest.fixture(scope="module")
def want():
    """the oracle's forward BWT of every input, computed once"""
    return {k: (d, oracle.transform_forward("BWT", d)) for k, d in _inputs().items()}


@pytest.fixture(scope="module")
def want_batch():
    return [(d, oracle.encode_block("BWT", "NONE", d) if len(d) else None) for d in _batch()]


def _set(monkeypatch, livepart, extra=None):
    if livepart != "unset":
        monkeypatch.setenv("KZ_BWT_LIVEPART", livepart)
    if extra:
        k, v = extra.split("=")
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("livepart", BOTH)
@pytest.mark.parametrize("name", sorted(_inputs()))
def test_single_blocks_match_the_oracle(ctx, monkeypatch, want, name, livepart):
    _set(monkeypatch, livepart)
    d, (ok_o, enc_o) = want[name]
    ok_g, enc_g = _fwd(ctx, kz.BWT_TYPE, d)
    assert ok_g == ok_o and enc_g == enc_o, (name, livepart, len(d))


@pytest.mark.parametrize("livepart", BOTH)
@pytest.mark.parametrize("name,switch", [("zeros-300000", "KZ_BWT_TRIEWIN=0"), ("zeros-in-text", "KZ_BWT_TRIEWIN=0"),
                                         ("lazy-twice", "KZ_BWT_LAZYRANK=0"), ("lazy-tail7", "KZ_BWT_LAZYRANK=0"),
                                         ("text-81921", "KZ_BWT_TRIE=0")])
def test_single_blocks_under_the_other_switches(ctx, monkeypatch, want, name, switch, livepart):
    """the window of oversized buckets through the LSD passes, round 0 with every rank stored, round 0 as an LSD round"""
    _set(monkeypatch, livepart, switch)
    d, (ok_o, enc_o) = want[name]
    ok_g, enc_g = _fwd(ctx, kz.BWT_TYPE, d)
    assert ok_g == ok_o and enc_g == enc_o, (name, switch, livepart, len(d))


@pytest.mark.parametrize("name", ["text-81921", "dead-tile", "zeros-in-text"])
def test_both_paths_in_one_run(ctx, monkeypatch, want, name):
    """KZ_BWT_LIVEPART=N: the ranks while more than 1 / N of the block is live, the text-order list below (N = 3: the hand-over)"""
    monkeypatch.setenv("KZ_BWT_LIVEPART", "3")
    d, (ok_o, enc_o) = want[name]
    ok_g, enc_g = _fwd(ctx, kz.BWT_TYPE, d)
    assert ok_g == ok_o and enc_g == enc_o, (name, len(d))


def _encode_batch(ctx, blocks, bs):
    B = len(blocks)
    inp = np.zeros((B, bs), dtype=np.uint8)
    lens = np.array([len(d) for d in blocks], dtype=np.int32)
    for i, d in enumerate(blocks):
        inp[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((B, ostride), dtype=np.uint8)
    return kz.encode_blocks(ctx, "BWT", "NONE", inp, bs, lens, out, ostride), out


@pytest.mark.parametrize("livepart", BOTH)
@pytest.mark.parametrize("retire", ["unset", "KZ_BWT_RETIRE=0"])
def test_ragged_batch_matches_the_oracle(ctx, monkeypatch, want_batch, retire, livepart):
    """blocks leave the later rounds' grids as they finish (rows = blocks still live), or ride through every round"""
    _set(monkeypatch, livepart, None if retire == "unset" else retire)
    res, out = _encode_batch(ctx, [d for d, _ in want_batch], 1 << 20)
    for i, (d, o) in enumerate(want_batch):
        if o is None:
            continue
        so, w, sf, pl = o
        assert res[i].status == 0 and (res[i].bits, res[i].skipFlags, res[i].length) == (w, sf, pl), (i, len(d))
        assert out[i, :(w + 7) // 8].tobytes() == so, (i, len(d))


def _launches(ctx, d):
    """the block through the batched encode call (it collects the kernel timers): (bits, bytes), launches per kernel id"""
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        res, out = _encode_batch(ctx, [d], 1 << 17)
        times = ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()
    assert res[0].status == 0
    return (res[0].bits, out[0, :(res[0].bits + 7) // 8].tobytes()), {k: v["launches"] for k, v in times.items()}


def test_the_new_path_is_taken(ctx, monkeypatch, want):
    """the bucket rounds of the default path do not write the text-order list: fewer launches under k_live_emit's id than with
    KZ_BWT_LIVEPART=0 (it still writes the list of the last rounds, below 4096 live suffixes), and none under k_msd_hist's id less;
    k_live_scatter runs under k_msd_scatter's id, so that id shows launches either way"""
    d = want["text-81921"][0]
    so, w, _, _ = oracle.encode_block("BWT", "NONE", d)
    enc_new, new = _launches(ctx, d)
    monkeypatch.setenv("KZ_BWT_LIVEPART", "0")
    enc_old, old = _launches(ctx, d)
    assert enc_new == enc_old == (w, so)
    assert old.get("k_msd_scatter", 0) > 0 and new.get("k_msd_scatter", 0) == old["k_msd_scatter"], (new, old)
    assert new.get("k_live_emit", 0) < old.get("k_live_emit", 0), (new, old)
    assert new.get("k_msd_hist", 0) >= old.get("k_msd_hist", 0), (new, old)
