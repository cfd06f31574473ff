"""Which byte a row of k_sbrt_inverse sees and which it writes (kz_sbrt.hip): block lengths around one row of 64 ranks, around
1 KiB (16 rows) and its small multiples, every row form on each side of such a border, one to eight waves per workgroup, blocks
that end exactly where their neighbour begins, and the decoder's schedules (views of one batch with masked lengths).  Written
with a chunked form of the kernel's input and output (1 KiB chunks through LDS, two chunks ahead; measured and not kept,
DESIGN 5); the sizes are the ones at which any batching of its loads and stores would go wrong.

Any byte string is a valid rank string.  Expected bytes are the CPU oracle's inverse of the rank string; the batched path frames
that inverse with encode_blocks (entropy NONE: the payload is the forward's output, which is the rank string again), the
single-block path (kz_transform_inverse) takes the rank string as it is."""
import functools

import numpy as np
import pytest

import datagen
import kanzi_amd as kz
import oracle

pytestmark = pytest.mark.gpu

CHUNK = 1024          # 16 rows of 64 ranks
AHEAD = 2             # chunks a batched input would run ahead
CHAINS = (("RANK", 2), ("MTFT", 1))
FORMS = ("zero", "uniform", "low", "few_high")


def _stretch(form, n, rng):
    """n ranks of one row form: all zero (zero runs only), uniform 0..255 (the interleaved keyed rows), values below 64 (dense rows,
    keyed by position), values below 64 with three ranks >= 64 in every 64 (the row-spanning stubs)"""
    if form == "zero":
        return np.zeros(n, dtype=np.uint8)
    if form == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    a = rng.integers(0, 64, n, dtype=np.uint8)
    if form == "few_high":
        for r in range(0, n, 64):
            w = min(64, n - r)
            a[r + rng.integers(0, w, 3)] = rng.integers(64, 256, 3, dtype=np.uint8)
    return a


def _ranks(n, seed, stretch=CHUNK, shift=0, forms=FORMS):
    """n ranks: stretches of `stretch` bytes that cycle through `forms` (the order depends on the seed), the whole string moved
    `shift` bytes to the left, so that the borders between forms fall `shift` bytes in front of the multiples of `stretch`"""
    rng = np.random.Generator(np.random.PCG64(seed))
    order = rng.permutation(len(forms))
    parts, total, k = [], 0, 0
    while total < n + shift:
        parts.append(_stretch(forms[order[k % len(forms)]], stretch, rng))
        total += stretch
        k += 1
    return np.concatenate(parts)[shift:shift + n].tobytes()


@functools.lru_cache(maxsize=None)
def _inverse(name, ranks):
    """the oracle's inverse of a rank string, computed once per string"""
    if not ranks:
        return b""
    ok, x = oracle.transform_inverse(name, ranks, len(ranks))
    assert ok and len(x) == len(ranks)
    return x


def _gpu_inverse_one(ctx, mode, ranks):
    src = kz.SliceByteArray(np.frombuffer(ranks, dtype=np.uint8).copy())
    dst = kz.SliceByteArray(np.full(len(ranks) + 64, 0xA5, dtype=np.uint8), length=len(ranks))
    assert kz.SBRT(ctx, mode).inverse(src, dst)
    assert dst.index == len(ranks)
    assert dst.array[len(ranks):].tobytes() == b"\xA5" * 64
    return dst.array[:len(ranks)].tobytes()


def _decode_batch(ctx, name, xs, stride=None):
    """frames the blocks xs with encode_blocks(name & NONE) and returns what decode_blocks makes of them: [(status, length, bytes)]"""
    B = len(xs)
    lens = np.array([len(x) for x in xs], dtype=np.int32)
    bs = int(stride or max(int(lens.max()), 1))
    inp = np.zeros((B, bs), dtype=np.uint8)
    for i, x in enumerate(xs):
        inp[i, :len(x)] = np.frombuffer(x, dtype=np.uint8)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((B, ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, name, "NONE", inp, bs, lens, out, ostride)
    assert all(r.status == 0 for r in res)
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.full((B, bs), 0xA5, dtype=np.uint8)
    r2 = kz.decode_blocks(ctx, name, "NONE", bs, out, ostride, bits, dec, bs)
    return [(r2[i].status, r2[i].length, dec[i, :max(r2[i].length, 0)].tobytes()) for i in range(B)]


def _check_batch(ctx, name, rank_strings, stride=None):
    xs = [_inverse(name, r) for r in rank_strings]
    got = _decode_batch(ctx, name, xs, stride)
    bad = [i for i, (st, ln, by) in enumerate(got) if st != 0 or ln != len(xs[i]) or by != xs[i]]
    assert not bad, "%s: blocks %s of %d differ from the oracle's inverse (lengths %s)" % (name, bad[:8], len(xs), [len(xs[i]) for i in bad[:8]])


SEAM_LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, AHEAD * CHUNK - 1, AHEAD * CHUNK + 1, (AHEAD + 1) * CHUNK - 1,
                (AHEAD + 1) * CHUNK, (AHEAD + 1) * CHUNK + 1, 16383, 16384, 16385, 65536 + 37)


@pytest.mark.parametrize("name,mode", CHAINS)
def test_chunk_seams_and_tails(ctx, name, mode):
    """block lengths around one row, 1 KiB, 2 KiB, 3 KiB, 16 KiB and 64 KiB: one block at a time through
    kz_transform_inverse, then all of them as one batch (one wave per workgroup)"""
    strings = [_ranks(n, 100 + k, stretch=192) for k, n in enumerate(SEAM_LENGTHS)]
    for r in strings:
        assert _gpu_inverse_one(ctx, mode, r) == _inverse(name, r), "length %d" % len(r)
    _check_batch(ctx, name, strings)


@pytest.mark.parametrize("name,mode", CHAINS)
def test_forward_rank_outputs_of_the_generator_classes(ctx, name, mode):
    """rank strings as the encoder makes them: the forward of the generator's five classes, raw and behind a BWT"""
    n = 65536 + 37
    strings = []
    for cls in range(5):
        x = datagen.block(cls, n, cls).tobytes()
        ok, r = oracle.transform_forward(name, x)
        assert ok and len(r) == n
        strings.append(r)
        ok, y = oracle.transform_forward("BWT", x)
        ok2, r2 = oracle.transform_forward(name, y)
        assert ok and ok2
        strings.append(r2)
    for r in strings:
        assert _gpu_inverse_one(ctx, mode, r) == _inverse(name, r)
    _check_batch(ctx, name, strings)


@pytest.mark.parametrize("name,mode", CHAINS)
def test_every_row_form_on_each_side_of_a_seam(ctx, name, mode):
    """one form alone; the forms in alternating stretches of 1 KiB (a chunk) and of 192 bytes (three rows: a change of form within
    a few rows of every seam); and the alternating strings moved by 1..63 bytes, so that every row phase meets every seam"""
    n = 6 * CHUNK + 300
    strings = [_ranks(n, 7, forms=(f,)) for f in FORMS]
    strings += [_ranks(n, 11 + s, stretch=CHUNK, shift=s) for s in range(64)]
    strings += [_ranks(n, 211 + s, stretch=192, shift=s) for s in range(64)]
    for r in strings[:6] + strings[67:70]:
        assert _gpu_inverse_one(ctx, mode, r) == _inverse(name, r)
    _check_batch(ctx, name, strings)


def test_every_workgroup_shape(ctx):
    """batches of 3, C + 1, 2 C + 1 and 4 C + 1 blocks (C = compute units): one, two, four and eight waves per workgroup.  Blocks of
    2-3 KiB, lengths mixed, empty blocks among them."""
    import torch
    C = torch.cuda.get_device_properties(0).multi_processor_count
    lengths = (2048, 3072, 0, 2049, 3071, 2500, 2111, 3009, 2047 + 64)
    base = [_ranks(3072, 500 + k, stretch=192, shift=7 * k) for k in range(16)]
    for name, _ in CHAINS:
        for B in (3, C + 1, 2 * C + 1, 4 * C + 1):
            _check_batch(ctx, name, [base[(5 * i + B) % 16][:lengths[(i + B) % len(lengths)]] for i in range(B)])


@pytest.mark.parametrize("name,mode", CHAINS)
def test_blocks_that_fill_their_slot_exactly(ctx, name, mode):
    """every block is as long as the stride of the caller's buffers, and that length is no multiple of 16: a store of a whole chunk
    past a block's end would land in its neighbour's first bytes"""
    n = 4099
    strings = [_ranks(n, 900 + k, stretch=192, shift=k) for k in range(24)]
    _check_batch(ctx, name, strings, stride=n)


def test_both_decoder_schedules(ctx, monkeypatch):
    """the staged decoder and the overlapped ones (views of the batch with masked lengths, RANK inverses of the cost classes side by
    side) on one 40-block batch of 64 KiB blocks: every schedule returns the oracle's decoding of the same block streams"""
    bs, B = 65536, 40
    inp = np.stack([datagen.block(i, bs) for i in range(B)])
    lens = np.full(B, bs, dtype=np.int32)
    lens[3], lens[11], lens[17], lens[29] = 9, 0, 30000, bs - 1
    ostride = kz.max_block_stream_bytes(bs)
    for chain in ("BWT+RANK+ZRLT", "BWT+MTFT+ZRLT"):
        out = np.zeros((B, ostride), dtype=np.uint8)
        res = kz.encode_blocks(ctx, chain, "ANS0", inp, bs, lens, out, ostride)
        assert all(r.status == 0 for r in res)
        bits = np.array([r.bits for r in res], dtype=np.int64)
        want = []
        for i in range(B):
            if lens[i] == 0:                                              # (an empty block has no stream to hand to the oracle)
                want.append((0, 0, b""))
                continue
            r, by = oracle.decode_block(chain, "ANS0", bs, out[i, :(int(bits[i]) + 7) // 8].tobytes(), int(bits[i]), bs)
            assert r == lens[i] and by == inp[i, :lens[i]].tobytes()
            want.append((0, int(lens[i]), by))
        for mode, fuse, nosf, wide in (("staged", "1000000", None, None), ("overlapped", "8", "1", "1"), ("overlapped3", "8", "1", "0"),
                                       ("first", "8", None, "1"), ("first3", "8", None, "0")):
            monkeypatch.setenv("KZ_FUSE_MIN_BLOCKS", fuse)
            if nosf:
                monkeypatch.setenv("KZ_NO_SFIRST", nosf)
            else:
                monkeypatch.delenv("KZ_NO_SFIRST", raising=False)
            if wide:
                monkeypatch.setenv("KZ_WIDE_QUEUES", wide)
            else:
                monkeypatch.delenv("KZ_WIDE_QUEUES", raising=False)
            dec = np.zeros((B, bs), dtype=np.uint8)
            r2 = kz.decode_blocks(ctx, chain, "ANS0", bs, out, ostride, bits, dec, bs)
            got = [(r2[i].status, r2[i].length, dec[i, :max(r2[i].length, 0)].tobytes()) for i in range(B)]
            assert got == want, (chain, mode, [i for i in range(B) if got[i] != want[i]][:8])
