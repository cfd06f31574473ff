"""CM (the context-model binary coder, EntropyCodecFactory.CM_TYPE = 6) on the device against the CPU model tests/cmmodel.py, which is
written from the reference's Java: single blocks, streams the encoder never writes, damaged input, the batched calls with the
output bound, whole streams with the TEXT variant that CM selects (TextCodec1, TransformFactory.java:275-286), and the refusals."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import cmcases
import cmmodel
import datagen
import katmodels
import kanzi_amd as kz
import textgen

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    return kz.Context(0)


def gpu_encode(ctx, data):
    e = kz.CMEncoder(ctx)
    assert e.encode(np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8), 0, len(data)) == len(data)
    return e.bits[0]


def gpu_decode(ctx, bits, nbits, count):
    """-> (ok, bytes, bits consumed)"""
    d = kz.CMDecoder(ctx, bits, nbits)
    buf = np.zeros(count, dtype=np.uint8)
    ok = d.decode(buf, 0, count) == count
    return ok, bytes(buf), getattr(d, "bits_consumed", 0)


def test_single_block_parity(ctx):
    """the encoder's bits are the model's, bit for bit and in length; the decoder restores the input and consumes what was written"""
    for label, (d, want, want_bits, _) in cmcases.encoded().items():
        bits, nbits = gpu_encode(ctx, d)
        assert nbits == want_bits and bits == want, label
        ok, out, used = gpu_decode(ctx, bits, nbits, len(d))
        assert ok and out == d, label
        if d:
            assert used == nbits, label


def test_streams_the_encoder_never_writes(ctx):
    """a varint longer than needed, payload behind what the decode reads, szBytes at count << 5 and one above: verdict, bytes and
    bits consumed are the model's"""
    seen = 0
    for label, bits, nbits, count, want in cmcases.unusual_streams():
        ok, out, used = gpu_decode(ctx, bits, nbits, count)
        assert ok == want[0], label
        if ok:
            assert out == want[1] and used == want[2], label
        seen += 1
    assert seen == 4


def test_damaged_input_follows_the_reference(ctx):
    compared = 0
    for cls, trial, bad, nb, count, want in cmcases.damaged_trials():
        ok, out, used = gpu_decode(ctx, bad, nb, count)
        assert ok == want[0], (cls, trial)
        if ok:
            assert out == want[1] and used == want[2], (cls, trial)
        compared += 1
    assert compared == 32


@functools.lru_cache(maxsize=None)
def _model_encode(payload):
    return cmmodel.encode(payload)


def _cm_block_from_none(stream, nbits, n, nfun):
    """the block stream EncodingTask.encodeBlock writes under CM, from the one it writes under NONE for the same chain (the
    transforms of these chains do not depend on the coder): a NONE block is always a raw "transformed copy"
    (CompressedOutputStream.java:926-973), whose header gives the skip flags and the transformed bytes.  -> (bytes, bits, coded)"""
    if n <= 15:                                                # SMALL_BLOCK_SIZE: stored whatever the coder
        return stream[:(nbits + 7) // 8], nbits, False
    assert nfun <= 4
    cmode = stream[0]
    ds = ((cmode >> 5) & 3) + 1
    post = int.from_bytes(stream[1:1 + ds], "big")
    payload = stream[2 + ds:2 + ds + post]
    skip = ((cmode & 0x0F) << 4) | 0x0F
    bits, eb = _model_encode(payload)
    written = 8 * (2 + ds) + eb
    if post < (written + 7) >> 3:
        return stream[:(nbits + 7) // 8], nbits, False
    mode = (((ds - 1) & 3) << 5) | (skip >> 4)
    hsf = ((mode << 4) | 0x0F) & 0xFF
    HASH = 0x1E35A7BD
    ck = (HASH * 0x01030507) & 0xFFFFFFFF
    for v in (mode, hsf, post, (written >> 32) & 0xFFFFFFFF, written & 0xFFFFFFFF):
        ck = katmodels._mix32(ck, HASH, v)
    ck = (ck >> 23) ^ (ck >> 3)
    head = bytes([mode]) + post.to_bytes(ds, "big") + bytes([ck & 0xFF])
    return head + bits, written, True


def _batch(blocks):
    bs = max(len(b) for b in blocks)
    inp = np.zeros((len(blocks), bs), dtype=np.uint8)
    lens = np.zeros(len(blocks), dtype=np.int32)
    for i, b in enumerate(blocks):
        inp[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[i] = len(b)
    return inp, lens, bs


@functools.lru_cache(maxsize=None)
def _pool():
    """the few distinct blocks the batches are made of (the model codes each once): about 2 KiB each, compressible ones, a random one
    (the raw fallback), and the short ones"""
    rng = np.random.default_rng(12)
    typical = [datagen.block(c, 2048 + 37 * c).tobytes() for c in range(5)] + [bytes(rng.integers(0, 256, 2000, dtype=np.uint8))]
    short = [b"", b"0123456789abcde", b"0123456789abcdef", b"xy" * 20]
    return typical, short, datagen.block(0, 1 << 16).tobytes()


def _blocks(nblocks):
    typical, short, big = _pool()
    if nblocks == 1:
        return [typical[0]]
    out = [big] + short[:max(0, min(len(short), nblocks - 2))]
    k = 0
    while len(out) < nblocks:
        out.append(typical[k % len(typical)])
        k += 1
    return out


def _tail_untouched(row, nbits):
    """the bytes of an output row behind the stream's last 32-bit word are as the call's own clearing of the rows left them"""
    return bool(np.all(row[(((nbits + 7) // 8) + 3) // 4 * 4:] == 0))


@pytest.mark.parametrize("nblocks", [1, 2, 65, 257])
@pytest.mark.parametrize("chain", ["NONE", "BWT+RANK+ZRLT", "LZ"])
def test_batched_block_streams(ctx, chain, nblocks):
    """batches of 1, 2, 65 and 257 blocks (more than a wave of blocks, more than the 256 CUs hold at once) of unequal length, with
    blocks of 0, 15 and 16 bytes, a random one (the raw fallback) and one of 64 KiB, in device memory: every block stream is the
    model's, nothing is written into a row behind its stream (the call clears the rows first) nor into the guards around the
    buffer; decode restores every block"""
    blocks = _blocks(nblocks)
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    ref = np.zeros((nblocks, ostride), dtype=np.uint8)
    rn = kz.encode_blocks(ctx, chain, "NONE", inp, bs, lens, ref, ostride)
    nfun = len(chain.split("+"))
    want = [_cm_block_from_none(ref[i].tobytes(), rn[i].bits, len(b), nfun) for i, b in enumerate(blocks)]
    guard = 4096
    d_in = torch.from_numpy(inp).cuda()
    d_out = torch.full((guard + nblocks * ostride + guard,), FILL, dtype=torch.uint8, device="cuda")
    res = kz.encode_blocks(ctx, chain, "CM", d_in.data_ptr(), bs, lens, d_out.data_ptr() + guard, ostride, kz.MEM_DEVICE)
    host = d_out.cpu().numpy()
    assert np.all(host[:guard] == FILL) and np.all(host[guard + nblocks * ostride:] == FILL), chain
    out = host[guard:guard + nblocks * ostride].reshape(nblocks, ostride)
    coded = 0
    for i in range(nblocks):
        assert res[i].status == 0 and res[i].bits == want[i][1], (chain, i)
        assert out[i, :(res[i].bits + 7) // 8].tobytes() == want[i][0], (chain, i)
        if want[i][2]:                                         # (a block stored raw instead may have had a longer CM stream under it)
            assert _tail_untouched(out[i], res[i].bits), (chain, i)
            coded += 1
    assert coded >= 1, chain
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((nblocks, bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, chain, "CM", bs, np.ascontiguousarray(out), ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert res2[i].status == 0 and res2[i].length == len(b) and dec[i, :len(b)].tobytes() == b, (chain, i)


def test_output_bound(monkeypatch):
    """A block whose stream does not fit its output row fails, alone, and writes nothing behind the row.  No input of test size
    outgrows the stride the batched calls ask for, so the rows are made shorter than the stride (KZ_CM_TEST_ROW_BYTES): first to
    the model's length of the longest stream rounded up to a word, which succeeds; then to 4 bytes less than its block header,
    varint and payload take, which fails that block only."""
    typical, _, _ = _pool()
    blocks = [typical[1], typical[4], typical[2], typical[0]]
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    ref = np.zeros((len(blocks), ostride), dtype=np.uint8)
    rn = kz.encode_blocks(kz.Context(0), "NONE", "NONE", inp, bs, lens, ref, ostride)
    want = [_cm_block_from_none(ref[i].tobytes(), rn[i].bits, len(b), 1) for i, b in enumerate(blocks)]
    assert all(w[2] for w in want)
    nbytes = [(w[1] + 7) // 8 for w in want]
    longest = int(np.argmax(nbytes))
    assert sorted(nbytes)[-2] + 16 < nbytes[longest]            # the others fit the shorter row too
    for row_bytes, fails in (((nbytes[longest] + 3) // 4 * 4, False), (nbytes[longest] - 7 - 4, True)):
        monkeypatch.setenv("KZ_CM_TEST_ROW_BYTES", str(row_bytes))
        c = kz.Context(0)                                      # the switches are read when a context is made
        d_in = torch.from_numpy(inp).cuda()
        guard = 4096
        d_out = torch.full((guard + len(blocks) * ostride + guard,), FILL, dtype=torch.uint8, device="cuda")
        res = kz.encode_blocks(c, "NONE", "CM", d_in.data_ptr(), bs, lens, d_out.data_ptr() + guard, ostride, kz.MEM_DEVICE)
        host = d_out.cpu().numpy()
        assert np.all(host[:guard] == FILL) and np.all(host[guard + len(blocks) * ostride:] == FILL), row_bytes
        out = host[guard:guard + len(blocks) * ostride].reshape(len(blocks), ostride)
        for i in range(len(blocks)):
            assert np.all(out[i, row_bytes:] == 0), (row_bytes, i)           # nothing behind the row (the call cleared it), whatever became of the block
            if fails and i == longest:
                assert res[i].status == -13 and res[i].bits == 0, (row_bytes, i)          # ERR_PROCESS_BLOCK, as RANGE fails a block
                continue
            assert res[i].status == 0 and res[i].bits == want[i][1], (row_bytes, i)
            assert out[i, :nbytes[i]].tobytes() == want[i][0], (row_bytes, i)
    monkeypatch.delenv("KZ_CM_TEST_ROW_BYTES")
    # the single-block call has the same bound: the stream must fit kz_max_block_stream_bytes(n)
    e = kz.CMEncoder(kz.Context(0))
    assert e.encode(np.frombuffer(blocks[0], dtype=np.uint8), 0, len(blocks[0])) == len(blocks[0])


def test_whole_stream(ctx, monkeypatch):
    """kz_compress == the model's .knz (katmodels.knz_stream with the CM block streams), kz_decompress restores the input; with
    32-bit block checksums the stream still round-trips (the reader verifies them)."""
    data = datagen.stream(3, 20000).tobytes() + b"tail"
    orig = katmodels._knz_block

    def block_cm(block, names, entropy, block_size, static_words):
        s, w = orig(block, names, "NONE", block_size, static_words)
        return _cm_block_from_none(s, w, len(block), len(names))[:2]
    monkeypatch.setattr(katmodels, "_knz_block", block_cm)
    cos = kz.CompressedOutputStream(ctx, "BWT+RANK+ZRLT", "CM", 20000)
    cos.write(data)
    cos.close()
    idx = kz.knz_index(cos.output)
    assert idx["entropy"] == 6
    want = katmodels.knz_stream(data, ["BWT", "RANK", "ZRLT"], "CM", 20000, [], idx["inputSize"])
    assert cos.output == want
    assert kz.CompressedInputStream(ctx, cos.output).read() == data
    cos = kz.CompressedOutputStream(ctx, "BWT+RANK+ZRLT", "CM", 20000, checksum=32)
    cos.write(data)
    cos.close()
    assert kz.knz_index(cos.output)["checksum"] == 32
    assert kz.CompressedInputStream(ctx, cos.output).read() == data
    bad = bytearray(cos.output)
    bad[len(bad) // 2] ^= 0x10                                 # a flipped payload bit: CM decodes other bytes, the checksum catches them
    with pytest.raises(kz.KanziError):
        kz.CompressedInputStream(ctx, bytes(bad)).read()


def test_whole_text_stream(ctx):
    """TEXT+UTF+BWT+RANK+ZRLT&CM on 200 KB of English in 64 KiB blocks, with and without checksums"""
    data = textgen.bulk_text(200000, 4).tobytes()
    for chk in (0, 32):
        cos = kz.CompressedOutputStream(ctx, "TEXT+UTF+BWT+RANK+ZRLT", "CM", 1 << 16, checksum=chk)
        cos.write(data)
        cos.close()
        assert len(cos.output) < len(data) // 2
        assert kz.CompressedInputStream(ctx, cos.output).read() == data, chk


def _text_static_words():
    """DICT_EN_1024 as the generated header holds it (the same reader as test_oracle.py's)"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "kzo_text_dict.h")).read()
    return b"".join(m.group(1).encode() for m in re.finditer(r'^\s*"([^"]*)"', src, re.M))


def test_text_forward_under_cm_is_textcodec1(ctx):
    """TEXT under CM is TextCodec1 (TransformFactory.java:275-286): each block's CM payload, decoded, equals
    katmodels.text_forward(variant 1) and differs from variant 2"""
    bs = 16000
    blocks = [textgen.bulk_text(bs, s).tobytes() for s in range(2)]
    ctx.set_block_size(bs)
    inp, lens, _ = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, "TEXT", "CM", inp, bs, lens, out, ostride)
    dic = katmodels.text_static_dictionary(_text_static_words())
    for i, b in enumerate(blocks):
        s = out[i].tobytes()
        mode = s[0]
        assert res[i].status == 0 and not (mode & 0x80) and not (mode & 0x08), i      # entropy coded, TEXT applied
        ds = ((mode >> 5) & 3) + 1
        post = int.from_bytes(s[1:1 + ds], "big")
        ok, got, _ = gpu_decode(ctx, s[2 + ds:], res[i].bits - 8 * (2 + ds), post)
        ok1, want1, _ = katmodels.text_forward(b, 1, bs, dic)
        ok2, want2, _ = katmodels.text_forward(b, 2, bs, dic)
        assert ok and ok1 and got == bytes(want1) and got != bytes(want2), i


def test_refusals(ctx):
    """blocks of 1 << 26 bytes and more are refused in both directions before anything is read (the reference codes them in 8 or
    16 chunks); ids that are not built stay refused"""
    small = np.zeros(64, dtype=np.uint8)
    rc = ctx.lib.kz_entropy_encode(ctx.h, 6, small.ctypes.data, 1 << 26, small.ctypes.data, 64)
    assert rc == -3 and "1 << 26" in ctx.error()                # ERR_INVALID_CODEC
    rc = ctx.lib.kz_entropy_decode(ctx.h, 6, small.ctypes.data, 64 * 8, small.ctypes.data, 1 << 26, None)
    assert rc == -3 and "1 << 26" in ctx.error()
    with pytest.raises(kz.KanziError) as e:
        ctx.set_entropy(9)                                      # TPAQX
    assert e.value.code == 3
    inp = np.zeros((1, 64), dtype=np.uint8)
    out = np.zeros((1, kz.max_block_stream_bytes(64)), dtype=np.uint8)
    for ent in (7, 9):                                          # TPAQ, TPAQX
        with pytest.raises(kz.KanziError) as e:
            kz.encode_blocks(ctx, "NONE", ent, inp, 64, [64], out, out.shape[1])
        assert e.value.code == 3
