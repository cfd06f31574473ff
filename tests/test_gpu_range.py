"""RANGE (order-0 range coder, EntropyCodecFactory.RANGE_TYPE = 4) on the device against the CPU model tests/rangemodel.py, which is
written from the reference's Java: single blocks, streams the encoder never writes (other lr, the grow-only f2s), damaged input,
the batched calls, whole streams and the TEXT variant that RANGE selects (TextCodec2, TransformFactory.java:275-286)."""
import numpy as np
import pytest
import torch

import datagen
import katmodels
import kanzi_amd as kz
import rangecases
import rangemodel
import textgen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return kz.Context(0)


def gpu_encode(ctx, data):
    e = kz.RangeEncoder(ctx)
    assert e.encode(np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8), 0, len(data)) == len(data)
    return e.bits[0]


def gpu_decode(ctx, bits, nbits, count):
    """-> (ok, bytes, bits consumed)"""
    d = kz.RangeDecoder(ctx, bits, nbits)
    buf = np.zeros(count, dtype=np.uint8)
    ok = d.decode(buf, 0, count) == count
    return ok, bytes(buf), getattr(d, "bits_consumed", 0)


def test_single_block_parity(ctx):
    """the encoder's bits are the model's; the decoder restores the input and consumes what was written"""
    for label, d in rangecases.parity_inputs():
        bits, nbits = gpu_encode(ctx, d)
        want = rangemodel.encode(d)
        assert (nbits, bits) == (want[1], want[0]), label
        if label == "low range":
            assert all(h >= 1 for h in rangemodel.low_range_hits), label   # the branch ran in the model's encode of each chunk
        ok, out, used = gpu_decode(ctx, bits, nbits, len(d))
        assert ok and out == d, label
        if d:
            assert used == nbits, label


def test_streams_the_encoder_never_writes(ctx):
    """lr 8, 9 and 15 for a whole block, a chunk at lr 8 behind one at lr 15, and quotients that land in the entries the wider chunk
    left in f2s: verdict, bytes and bits consumed are the model's"""
    for label, bits, nbits, count, want in rangecases.unusual_streams():
        ok, out, used = gpu_decode(ctx, bits, nbits, count)
        assert ok == want[0], label
        if ok:
            assert out == want[1] and used == want[2], label


def test_damaged_input_follows_the_reference(ctx):
    compared = 0
    for cls, trial, bad, nb, count, want in rangecases.damaged_trials():
        ok, out, used = gpu_decode(ctx, bad, nb, count)
        assert ok == want[0], (cls, trial)
        if ok:
            assert out == want[1] and used == want[2], (cls, trial)
        compared += 1
    assert compared == 48


def _range_block_from_none(stream, nbits, n, nfun):
    """the block stream EncodingTask.encodeBlock writes under RANGE, from the one it writes under NONE for the same chain (the
    transforms do not depend on the coder unless the chain has TEXT): a NONE block is always a raw "transformed copy"
    (CompressedOutputStream.java:926-973), whose header gives the skip flags and the transformed bytes"""
    if n <= 15:                                                # SMALL_BLOCK_SIZE: stored whatever the coder
        return stream[:(nbits + 7) // 8], nbits
    assert nfun <= 4
    cmode = stream[0]
    ds = ((cmode >> 5) & 3) + 1
    post = int.from_bytes(stream[1:1 + ds], "big")
    payload = stream[2 + ds:2 + ds + post]
    skip = ((cmode & 0x0F) << 4) | 0x0F
    bits, eb = rangemodel.encode(payload)
    written = 8 * (2 + ds) + eb
    if post < (written + 7) >> 3:
        return stream[:(nbits + 7) // 8], nbits
    mode = (((ds - 1) & 3) << 5) | (skip >> 4)
    hsf = ((mode << 4) | 0x0F) & 0xFF
    HASH = 0x1E35A7BD
    ck = (HASH * 0x01030507) & 0xFFFFFFFF
    for v in (mode, hsf, post, (written >> 32) & 0xFFFFFFFF, written & 0xFFFFFFFF):
        ck = katmodels._mix32(ck, HASH, v)
    ck = (ck >> 23) ^ (ck >> 3)
    head = bytes([mode]) + post.to_bytes(ds, "big") + bytes([ck & 0xFF])
    return head + bits, written


def _batch(blocks):
    bs = max(len(b) for b in blocks)
    inp = np.zeros((len(blocks), bs), dtype=np.uint8)
    lens = np.zeros(len(blocks), dtype=np.int32)
    for i, b in enumerate(blocks):
        inp[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[i] = len(b)
    return inp, lens, bs


@pytest.mark.parametrize("chain", ["NONE", "BWT+RANK+ZRLT", "LZ"])
def test_batched_block_streams(ctx, chain):
    """blocks of unequal length, one of 15 bytes (a copy block) and one incompressible (the raw fallback), in host memory, in device
    memory and through the submit forms"""
    rng = np.random.default_rng(11)
    blocks = [datagen.block(c, 33000 + 999 * c).tobytes() for c in range(5)]
    blocks += [b"0123456789abcde", bytes(rng.integers(0, 256, 5000, dtype=np.uint8)), bytes(rng.integers(0, 4, 777, dtype=np.uint8)), b"xy" * 20]
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    ref = np.zeros((len(blocks), ostride), dtype=np.uint8)
    rn = kz.encode_blocks(ctx, chain, "NONE", inp, bs, lens, ref, ostride)
    nfun = len(chain.split("+"))
    want = [_range_block_from_none(ref[i].tobytes(), rn[i].bits, len(b), nfun) for i, b in enumerate(blocks)]
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, chain, "RANGE", inp, bs, lens, out, ostride)
    for i in range(len(blocks)):
        assert res[i].status == 0 and res[i].bits == want[i][1], (chain, i)
        assert out[i, :(res[i].bits + 7) // 8].tobytes() == want[i][0], (chain, i)
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(blocks), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, chain, "RANGE", bs, out, ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert res2[i].status == 0 and res2[i].length == len(b) and dec[i, :len(b)].tobytes() == b, (chain, i)
    # device memory, and the asynchronous calls
    d_in = torch.from_numpy(inp).cuda()
    d_out = torch.zeros((len(blocks), ostride), dtype=torch.uint8, device="cuda")
    res_d = kz.encode_blocks(ctx, chain, "RANGE", d_in.data_ptr(), bs, lens, d_out.data_ptr(), ostride, kz.MEM_DEVICE)
    host = d_out.cpu().numpy()
    for i in range(len(blocks)):
        assert res_d[i].bits == res[i].bits and host[i, :(res[i].bits + 7) // 8].tobytes() == want[i][0], (chain, i)
    d_dec = torch.zeros((len(blocks), bs), dtype=torch.uint8, device="cuda")
    kz.decode_blocks(ctx, chain, "RANGE", bs, d_out.data_ptr(), ostride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
    assert np.array_equal(d_dec.cpu().numpy(), dec)
    out2 = np.zeros_like(out)
    job = kz.submit_encode_blocks(ctx, chain, "RANGE", inp, bs, lens, out2, ostride)
    job.wait()
    assert np.array_equal(out2, out)
    dec2 = np.zeros_like(dec)
    kz.submit_decode_blocks(ctx, chain, "RANGE", bs, out, ostride, bits, dec2, bs).wait()
    assert np.array_equal(dec2, dec)


def test_batched_text_chain_round_trip(ctx):
    blocks = [textgen.bulk_text(40000, s).tobytes() for s in range(3)] + [datagen.block(c, 20000).tobytes() for c in range(3)] + [b"short text"]
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    ctx.set_block_size(bs)
    res = kz.encode_blocks(ctx, "TEXT+UTF+BWT+RANK+ZRLT", "RANGE", inp, bs, lens, out, ostride)
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(blocks), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, "TEXT+UTF+BWT+RANK+ZRLT", "RANGE", bs, out, ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert res[i].status == 0 and res2[i].status == 0 and dec[i, :len(b)].tobytes() == b, i


def test_whole_stream(ctx, monkeypatch):
    """kz_compress == the model's .knz (katmodels.knz_stream with the RANGE block streams), kz_decompress restores the input."""
    data = datagen.stream(3, 20000).tobytes() + b"tail"
    orig = katmodels._knz_block

    def block_range(block, names, entropy, block_size, static_words):
        s, w = orig(block, names, "NONE", block_size, static_words)
        return _range_block_from_none(s, w, len(block), len(names))
    monkeypatch.setattr(katmodels, "_knz_block", block_range)
    cos = kz.CompressedOutputStream(ctx, "BWT+RANK+ZRLT", "RANGE", 20000)
    cos.write(data)
    cos.close()
    want = katmodels.knz_stream(data, ["BWT", "RANK", "ZRLT"], "RANGE", 20000, [], kz.knz_index(cos.output)["inputSize"])
    assert cos.output == want
    assert kz.CompressedInputStream(ctx, cos.output).read() == data


def _text_stage_output(ctx, entropy, inp, lens, bs):
    """the TEXT stage's bytes of every block of a TEXT & entropy batch: the coder's payload, decoded"""
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(lens), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, "TEXT", entropy, inp, bs, lens, out, ostride)
    stages = []
    for i in range(len(lens)):
        assert res[i].status == 0, (entropy, i)
        s = out[i, :(res[i].bits + 7) // 8].tobytes()
        ds = ((s[0] >> 5) & 3) + 1
        post = int.from_bytes(s[1:1 + ds], "big")
        if s[0] & 0x80:                                        # stored raw ("transformed copy" or copy block)
            stages.append((s[0] & 0x0F, s[2 + ds:2 + ds + post]))
            continue
        dec = kz.RangeDecoder(ctx, s[2 + ds:], res[i].bits - 8 * (2 + ds)) if entropy == "RANGE" else kz.ANSRangeDecoder(ctx, s[2 + ds:], res[i].bits - 8 * (2 + ds))
        buf = np.zeros(post, dtype=np.uint8)
        assert dec.decode(buf, 0, post) == post, (entropy, i)
        stages.append((s[0] & 0x0F, bytes(buf)))
    return stages


def test_text_forward_under_range_is_textcodec2(ctx):
    """TEXT under RANGE is TextCodec2, as under ANS0 (TransformFactory.java:275-286): the stage's output is the same bytes"""
    blocks = [textgen.bulk_text(30000, s).tobytes() for s in range(3)] + [datagen.block(3, 20000).tobytes()]
    inp, lens, bs = _batch(blocks)
    ctx.set_block_size(bs)
    a = _text_stage_output(ctx, "RANGE", inp, lens, bs)
    b = _text_stage_output(ctx, "ANS0", inp, lens, bs)
    assert a == b
    assert any(len(t) < len(blk) for (_, t), blk in zip(a, blocks))          # TEXT was applied somewhere
