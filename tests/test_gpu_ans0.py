"""The device's ANS0 coder (kanzi_amd/csrc/kz_ans.hip) on the case set of tests/ans0cases.py, bit for bit against the CPU oracle:
the encoder cases through kz.ANSRangeEncoder and back through kz.ANSRangeDecoder (every branch of the data-parallel
normalizeFrequencies, every header form, every way the four-lane coding loop ends, the splices of k_ans_enc_concat), the block
of 65 chunks (the carry of k_ans_enc_scan), the model's streams at every logRange the decoder accepts, the crafted streams that
end in one known event at one known chunk, and batches through kz.encode_blocks / kz.decode_blocks (chain NONE) where raw,
header-only and ordinary blocks meet in one launch and where the index pass needs a second workgroup.  What each case makes the
kernels do is proven on the CPU in tests/test_ans0_cases.py, and so is every expected answer the oracle's encoder cannot give
(the model and the oracle's decoder agree on it there).

The payload window of k_ans_dec_chunk.  Host streams are copied into slots of align(longest stream + 64, 256) zeroed bytes
(kz_entropy_decode, kz_decode_blocks); device streams are read in place and carry KZ_STREAM_SLACK = 64 bytes behind the longest
stream (checked by kz_decode_blocks).  winOk asks for payByte + sz + 48 <= inStride.  The chunk kernel only decodes chunks the
index pass walked to the end (ck < nIdx, and not the header-only chunk of a SKIP): for those the index pass has seen the end of
the payload at or before the block's last bit, so payByte + sz <= stream bytes <= inStride - 64.  A size that reaches past the
bits fails in the index pass (fail_cut_payload, fail_size_above_buffer here) before the chunk kernel looks at it.  So no stream,
valid or not, makes winOk false under the layout contract, and there is no case for the byte-peek fallback.  The window itself:
window_uniform (all four lanes refill at most steps, the window slides every step or two), window_two_symbols (a few refills in
4096 steps, long stretches without a slide), and every other case in between."""
import numpy as np
import pytest

import ans0cases as C
import kanzi_amd as kz
import oracle

pytestmark = pytest.mark.gpu

POISON = 0xA5


def gpu_encode(ctx, data):
    e = kz.ANSRangeEncoder(ctx)
    assert e.encode(np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8), 0, len(data)) == len(data)
    return e.bits[0]


def gpu_decode(ctx, bits, nbits, count):
    """-> (verdict: decode() == count, bytes, bits consumed)"""
    d = kz.ANSRangeDecoder(ctx, bits, nbits)
    buf = np.full(count, POISON, dtype=np.uint8)
    ok = d.decode(buf, 0, count) == count
    return ok, (bytes(buf) if ok else None), (d.bits_consumed if ok else None)


def _round(ctx, data):
    """the device writes the oracle's bits and reads them as the oracle does (bytes, and every bit consumed)"""
    want = oracle.entropy_encode("ANS0", data)
    assert gpu_encode(ctx, data) == want
    if not data:
        return
    r, out, pos = oracle.entropy_decode("ANS0", want[0], want[1], len(data))
    assert r == len(data) and pos == want[1]
    assert gpu_decode(ctx, want[0], want[1], len(data)) == (True, out, pos)
    return out


def test_encoder_cases(ctx):
    bad, back = [], 0
    for c in C.encoder_cases():
        try:
            back += _round(ctx, c.data) == c.data
        except AssertionError:
            bad.append(c.name)
    assert not bad, " ".join(bad)
    assert back == len(C.encoder_cases()) - 2                 # all but the empty block and slow-_limit, which the reference itself does not return


def test_block_of_65_chunks(ctx):
    """the exclusive scan of the chunk bit lengths carries past the 64 chunks of one wave iteration"""
    data = C.scan_case()
    assert _round(ctx, data) == data


@pytest.mark.parametrize("name", sorted(C.lr_inputs()))
def test_decoder_accepts_every_lr(ctx, name):
    """the model's streams at logRange 8 .. 15 (the encoders only write 12): ans_fill_f2s with idle lanes below 12, the binary
    search in the cumulative table above"""
    data = C.lr_inputs()[name]
    for lr in C.LR_RANGE:
        bits, nbits = C.lr_stream(name, lr)
        assert oracle.entropy_decode("ANS0", bits, nbits, len(data)) == (len(data), data, nbits), lr
        assert gpu_decode(ctx, bits, nbits, len(data)) == (True, data, nbits), lr


def test_crafted_events(ctx):
    """one event at a known chunk, or two in either order: the verdict, the bytes with the zero tail from where the reference stops
    writing, and after STOP / SKIP the bits consumed, all the oracle's"""
    bad = []
    for d in C.decoder_cases():
        r, out, pos = oracle.entropy_decode("ANS0", d.bits, d.nbits, d.count)
        assert (r == d.count) == (d.event[0] != "FAIL"), d.name
        want = (True, out, pos) if r == d.count else (False, None, None)
        if gpu_decode(ctx, d.bits, d.nbits, d.count) != want:
            bad.append(d.name)
    assert not bad, " ".join(bad)


def _batch(blocks):
    bs = max(len(b) for b in blocks)
    inp = np.zeros((len(blocks), bs), dtype=np.uint8)
    lens = np.zeros(len(blocks), dtype=np.int32)
    for i, b in enumerate(blocks):
        inp[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[i] = len(b)
    return inp, lens, bs


def test_mixed_batch(ctx):
    """raw (1, 16, 32 bytes), header-only (one symbol, three chunks) and ordinary blocks of 1 to 9 chunks in one launch: the chunk
    grid is 9 wide for all of them.  The uniform blocks (4096 bytes: the total == scale shortcut; 50000 bytes) are coded and then
    stored as copy blocks, being no shorter coded; their skewed twins at the end stay coded.  Each row is the oracle's block
    stream of that block alone, and decodes back."""
    blocks = [C.rnd(701, 1), C.rnd(702, 16), C.rnd(703, 32, 4), C.rnd(704, 33, 4), bytes([9]) * (2 * C.CHUNK + 5), C.geometric(705, C.CHUNK + 1),
              C.even(4096, range(256), 706), C.rnd(707, 50000), C.geometric(708, 8 * C.CHUNK + 77, 0.1, 150),
              C.from_counts([(s, 1) for s in range(255)] + [(255, 3841)], 709), C.rnd(710, 50000, 200)]      # (the two before stay coded)
    coded = [not (oracle.encode_block("NONE", "ANS0", b, block_size=9 * C.CHUNK)[0][0] & 0x80) for b in blocks]
    assert coded == [False, False, False, True, True, True, False, False, True, True, True]
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, "NONE", "ANS0", inp, bs, lens, out, ostride)
    for i, b in enumerate(blocks):
        s, w, sf, pl = oracle.encode_block("NONE", "ANS0", b, block_size=bs)
        assert (res[i].status, res[i].bits, res[i].skipFlags, res[i].length) == (0, w, sf, pl), i
        assert out[i, :(w + 7) // 8].tobytes() == s, i
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.full((len(blocks), bs), POISON, dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, "NONE", "ANS0", bs, out, ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert (res2[i].status, res2[i].length) == (0, len(b)) and dec[i, :len(b)].tobytes() == b, i
        assert bool((dec[i, len(b):] == POISON).all()), i


def test_batch_of_70_blocks_with_events(ctx):
    """70 blocks of 33 .. 300 bytes: k_ans_dec_index runs one lane per block, so rows 64 .. 69 are its second workgroup.  Five rows
    carry a crafted event (three of them in that workgroup); each row ends as the oracle ends that block alone, and the
    neighbours come back untouched."""
    n = 70
    lens = [33 + (i * 97) % 268 if i < 60 else 150 + 15 * (i - 60) for i in range(n)]
    blocks = [C.geometric(800 + i, lens[i], 0.6, 5) for i in range(n)]
    streams = [oracle.encode_block("NONE", "ANS0", b, block_size=512)[:2] for b in blocks]
    assert all(not (streams[i][0][0] & 0x80) for i in range(60, n))                # entropy coded, not copy blocks
    assert sum(1 for s, w in streams if not (s[0] & 0x80)) >= 50
    rows = (3, 40, 64, 66, 69)
    kinds = {}
    for row, (cnt, b, nb, kind) in zip(rows, C.small_event_blocks()):
        streams[row] = C.block_stream(cnt, b, nb)
        lens[row], blocks[row], kinds[row] = cnt, None, kind
    istride = (max(len(s) for s, w in streams) + 64) | 1
    inp = np.full((n, istride), POISON, dtype=np.uint8)
    for i, (s, w) in enumerate(streams):
        inp[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    bits = np.array([w for s, w in streams], dtype=np.int64)
    ostride = 513
    dec = np.full((n, ostride), POISON, dtype=np.uint8)
    res = kz.decode_blocks(ctx, "NONE", "ANS0", 512, inp, istride, bits, dec, ostride)
    bad = []
    for i in range(n):
        r, want = oracle.decode_block("NONE", "ANS0", 512, streams[i][0], streams[i][1], 512)
        if blocks[i] is not None:
            assert (r, want) == (lens[i], blocks[i]), i
        else:
            assert (r == lens[i]) == (kinds[i] != "FAIL"), i
        if r < 0:
            ok = res[i].status != 0
        else:
            ok = (res[i].status, res[i].length) == (0, r) and dec[i, :r].tobytes() == want and bool((dec[i, r:] == POISON).all())
        if not ok:
            bad.append((i, res[i].status, res[i].length))
    assert not bad, bad
