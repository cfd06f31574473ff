"""The device's inverse BWT (kanzi_amd/csrc/kz_bwt_inv.hip) on the case set of tests/bwtinvcases.py, byte for byte against the CPU
oracle: one block at a time through kz_transform_inverse (a destination of exactly n and of n + 1 bytes, poisoned, with guard bytes
behind it), the ragged batches of the set through kz_decode_blocks("BWT", "NONE") (poisoned stream tails, strides that are no
multiple of 16, empty blocks that shift the dense scratch index, damaged blocks beside well-formed ones, 2000 blocks in one call,
small blocks beside the neighbour that moves the grid to S = 128), the well-formed cases inside BWT+RANK+ZRLT & ANS0 batches under
every decoder schedule, and the blocks of a megabyte (one walker carries the block; past the walk cap the literal walkers finish a
block an encoder made).  What each case makes the kernels do is proven on the CPU in tests/test_bwt_inverse_cases.py.

Expected bytes are the oracle's inverse of the frame, never the model's; for well-formed cases they are the text as well."""
import ctypes
import functools
import time

import numpy as np
import pytest

import bwtinvcases as C
import kanzi_amd as kz
import oracle

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 64


@functools.lru_cache(maxsize=None)
def _want(frame, cap):
    """the oracle's inverse of a frame into cap bytes, computed once: (applied, bytes; none where it refuses)"""
    if not frame:
        return True, b""
    ok, out = oracle.transform_inverse("BWT", frame, cap)
    return ok, out if ok else b""


def _inverse_one(ctx, frame, cap):
    """kz_transform_inverse into a poisoned destination of cap bytes with GUARD bytes behind it -> (applied, bytes)"""
    src = np.frombuffer(frame, dtype=np.uint8).copy()
    dst = np.full(cap + GUARD, POISON, dtype=np.uint8)
    produced = ctypes.c_int32(0)
    rc = ctx.lib.kz_transform_inverse(ctx.h, kz.BWTBlockCodec.TYPE, src.ctypes.data, len(src), dst.ctypes.data, cap, ctypes.addressof(produced))
    ctx.check(rc)
    assert dst[cap:].tobytes() == bytes([POISON]) * GUARD, "bytes behind dstCap were written"
    if rc == 0:
        return False, b""
    assert 0 <= produced.value <= cap
    assert bool((dst[produced.value:cap] == POISON).all()), "bytes behind the block were written"
    return True, dst[:produced.value].tobytes()


def _check_one(ctx, c):
    n = len(_want(c.frame, max(len(c.frame), 1))[1])
    for cap in (max(n, 1), n + 1):
        want = _want(c.frame, cap)
        assert _inverse_one(ctx, c.frame, cap) == want, (c.name, cap)
        if c.text is not None:
            assert want == (True, c.text), c.name


@pytest.mark.parametrize("group", ["small", "mid"])
def test_single_blocks(ctx, group):
    cs = [c for c in C.cases() if c.group == group and c.frame]
    assert len(cs) >= (90 if group == "small" else 4)
    for c in cs:
        _check_one(ctx, c)


def _decode_batch(ctx, blocks):
    """the blocks' frames as `BWT & NONE` block streams, every stream followed by poison, both strides odd -> [(status, length, bytes)]"""
    streams = [C.block_stream(c.frame) if c.frame else (b"", 0) for c in blocks]
    bs = max(max(len(c.frame) for c in blocks), 64)
    istride = (max(len(s) for s, w in streams) + 64) | 1
    ostride = (bs + 16) | 1
    inp = np.full((len(blocks), istride), POISON, dtype=np.uint8)
    for i, (s, w) in enumerate(streams):
        inp[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    bits = np.array([w for s, w in streams], dtype=np.int64)
    dec = np.full((len(blocks), ostride), POISON, dtype=np.uint8)
    res = kz.decode_blocks(ctx, "BWT", "NONE", bs, inp, istride, bits, dec, ostride)
    return [(res[i].status, res[i].length, dec[i, :max(res[i].length, 0)].tobytes(), dec[i, max(res[i].length, 0):]) for i in range(len(blocks))], bs


def _check_batch(ctx, blocks):
    got, bs = _decode_batch(ctx, blocks)
    bad = []
    for i, c in enumerate(blocks):
        ok, out = _want(c.frame, bs + max(512, bs >> 4))          # (the decoder's working size, CompressedInputStream.java:694-695)
        st, ln, by, rest = got[i]
        if ok != (st == 0) or (ok and (ln != len(out) or by != out)) or (ok and c.text is not None and by != c.text):
            bad.append((i, c.name, st, ln))
        elif ok and not bool((rest == POISON).all()):
            bad.append((i, c.name, "bytes behind the block"))
    assert not bad, bad[:8]


@pytest.mark.parametrize("name", ["small", "small_reversed", "mid", "many"])
def test_ragged_batches(ctx, name):
    """every case in one kz_decode_blocks call with its neighbours: block i's status, length and bytes are what the oracle gives block
    i alone.  `many`: 2000 blocks, the second pass of k_bwti_ord's loop."""
    _check_batch(ctx, C.batches()[name])


@pytest.mark.parametrize("size", [1051648, 1051649])
def test_small_blocks_beside_the_neighbour_that_sets_the_grid(ctx, size):
    """the longest block of a batch picks the grid spacing for all of them: S = 64 up to 1 051 648 framed bytes, S = 128 from
    1 051 649 on.  The periodic blocks whose one walker carries them at S = 128, the damaged blocks and the pool's overflow case
    decode beside either neighbour, and so does the neighbour."""
    _check_batch(ctx, C.batches()["beside_%d" % size])


SCHEDULES = (("staged", "1000000", None, None), ("overlapped", "8", "1", "1"), ("overlapped3", "8", "1", "0"),
             ("first", "8", None, "1"), ("first3", "8", None, "0"))


def test_decoder_schedules(ctx, monkeypatch):
    """the well-formed cases of 300 bytes to 64 KiB as blocks of one BWT+RANK+ZRLT & ANS0 batch (the oracle's block streams), empty
    blocks among them, under the staged decoder and the overlapped ones (views of the batch with masked lengths): every schedule
    returns every text"""
    bs = 65536
    texts = [c.text for c in C.cases() if c.text is not None and 300 <= len(c.text) <= bs]
    assert len(texts) >= 30
    texts.insert(7, b"")
    texts.insert(0, b"")
    texts.append(b"")
    chain = "BWT+RANK+ZRLT"
    enc = [oracle.encode_block(chain, "ANS0", t, block_size=bs) if t else (b"", 0, 0, 0) for t in texts]
    istride = (max(len(e[0]) for e in enc) + 64) | 1
    inp = np.full((len(texts), istride), POISON, dtype=np.uint8)
    for i, e in enumerate(enc):
        inp[i, :len(e[0])] = np.frombuffer(e[0], dtype=np.uint8)
    bits = np.array([e[1] for e in enc], dtype=np.int64)
    want = [(0, len(t), t) for t in texts]
    for mode, fuse, nosf, wide in SCHEDULES:
        monkeypatch.setenv("KZ_FUSE_MIN_BLOCKS", fuse)
        for key, val in (("KZ_NO_SFIRST", nosf), ("KZ_WIDE_QUEUES", wide)):
            if val:
                monkeypatch.setenv(key, val)
            else:
                monkeypatch.delenv(key, raising=False)
        dec = np.full((len(texts), bs + 1), POISON, dtype=np.uint8)
        res = kz.decode_blocks(ctx, chain, "ANS0", bs, inp, istride, bits, dec, bs + 1)
        got = [(res[i].status, res[i].length, dec[i, :max(res[i].length, 0)].tobytes()) for i in range(len(texts))]
        assert got == want, (mode, [i for i in range(len(texts)) if got[i] != want[i]][:8])


def test_large_blocks(ctx):
    """a megabyte each, one block per call: the long walk inside the cap is stitched, the walk of cap + 1 links is stitched, the
    walks of cap + 2 links and more leave a block that an encoder made to the literal walkers.  Measured times per call (copies
    included) are in bwtinvcases.LARGE_TIMES; a walk of 2^20 dependent loads is the whole of it."""
    for c in C.large_cases():
        t0 = time.perf_counter()
        got = _inverse_one(ctx, c.frame, len(c.text))
        dt = time.perf_counter() - t0
        print("%s: n = %d, %.3f s" % (c.name, len(c.text), dt))
        assert got == (True, c.text), c.name
