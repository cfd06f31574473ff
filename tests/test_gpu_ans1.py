"""ANS1 (order-1 range ANS, EntropyCodecFactory.ANS1_TYPE = 8) on the device against the CPU model tests/ans1model.py, which is
written from the reference's Java: single blocks, the lr range the decoder accepts, damaged input, the batched calls, whole
streams and the TEXT variant that ANS1 selects (TextCodec1, TransformFactory.java:275-286)."""
import numpy as np
import pytest
import torch

import ans1model
import datagen
import katmodels
import kanzi_amd as kz
import refinputs
import textgen

pytestmark = pytest.mark.gpu

MIB4 = 1 << 22


@pytest.fixture(scope="module")
def ctx():
    return kz.Context(0)


def gpu_encode(ctx, data):
    e = kz.ANSRangeEncoder(ctx, order=1)
    assert e.encode(np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8), 0, len(data)) == len(data)
    return e.bits[0]


def gpu_decode(ctx, bits, nbits, count):
    """-> (ok, bytes, bits consumed)"""
    d = kz.ANSRangeDecoder(ctx, bits, nbits, order=1)
    buf = np.zeros(count, dtype=np.uint8)
    ok = d.decode(buf, 0, count) == count
    return ok, bytes(buf), getattr(d, "bits_consumed", 0)


def model_decode(bits, nbits, count):
    """-> (ok, bytes, bits consumed) of the reference's decoder"""
    try:
        r, out, used, _ = ans1model.decode(bits, nbits, count, 1)
    except katmodels.JavaException:
        return False, None, None
    return r == count, out, used


def check_block(ctx, data, model=None):
    bits, nbits = gpu_encode(ctx, data)
    want = ans1model.encode(data, 1) if model is None else model
    assert (nbits, bits) == (want[1], want[0]), len(data)
    ok, out, used = gpu_decode(ctx, bits, nbits, len(data))
    assert ok, len(data)
    if out != data:                                       # the reference's own round trip fails here (tests/test_ans1_model.py)
        assert out == model_decode(bits, nbits, len(data))[1], len(data)
    elif len(data):
        assert used == nbits, len(data)
    return bits, nbits, out


def test_single_block_parity(ctx):
    rng = np.random.default_rng(5)
    inputs = refinputs.entropy_inputs() + refinputs.edge_inputs()
    inputs += [bytes(rng.integers(0, 6, n, dtype=np.uint8)) for n in (0, 1, 32, 33)]
    inputs += [datagen.block(c, 65536).tobytes() for c in range(5)]
    for d in inputs:
        _, _, out = check_block(ctx, d)
        assert out == d, len(d)


def test_blocks_of_several_chunks(ctx):
    """4 MiB is one chunk; 4 MiB + {1, 2, 3} ends with a chunk of 1-3 bytes that codes the previous chunk's last byte in context 0;
    + 33 a short second chunk; 8 MiB + 5 three chunks.  0x00 never follows 0x00 in chunk 0 of `base`, so its last byte (set to
    0x00 or to a byte present in context 0) decides whether that Symbol was ever reset: both cases of the reference's tail-chunk
    quirk."""
    base = bytearray(datagen.block(2, MIB4 + 64).tobytes())
    for i in range(1, len(base)):
        if base[i] == 0 and base[i - 1] == 0:
            base[i] = 1
    first = base[0]
    d4 = bytes(base[:MIB4])
    b4, n4 = gpu_encode(ctx, d4)
    variants = {1: bytes(base[:MIB4 + 1]), 33: bytes(base[:MIB4 + 33])}
    t = bytearray(base[:MIB4 + 2]); t[MIB4 - 1] = 0; variants[2] = bytes(t)        # a Symbol never reset: the tail comes back wrong
    t = bytearray(base[:MIB4 + 3]); t[MIB4 - 1] = first; variants[3] = bytes(t)    # present in context 0: round trip
    wrong = 0
    for k, d in sorted(variants.items()):
        want = ans1model.encode(d, 1)
        if k == 1:                                            # the 4 MiB block is chunk 0 of this stream
            assert want[0][:n4 // 8] == b4[:n4 // 8]
        _, _, out = check_block(ctx, d, want)
        wrong += out != d
        if k == 3:
            assert out == d
    assert wrong >= 1
    ok, out, used = gpu_decode(ctx, b4, n4, MIB4)
    assert ok and out == d4 and used == n4
    d8 = datagen.block(4, 2 * MIB4 + 5).tobytes()
    _, _, out = check_block(ctx, d8)


def test_decoder_accepts_every_lr(ctx):
    """Streams the model writes at lr 8, 11, 14 and 15 (the encoder itself only writes 11; decodeHeader takes 8 .. 15).  The
    second input does not survive lr 8 in the reference itself: the device gives the model decoder's bytes."""
    for data, roundtrip in ((datagen.block(3, 30000).tobytes(), True), (datagen.block(3, 50000).tobytes(), False)):
        for lr in (8, 11, 14, 15):
            bits, nbits = ans1model.encode(data, 1, lr=lr)
            want = model_decode(bits, nbits, len(data))
            ok, out, used = gpu_decode(ctx, bits, nbits, len(data))
            assert ok == want[0] and out == want[1], lr
            if roundtrip or lr != 8:
                assert out == data and used == nbits, lr


def test_damaged_input_follows_the_reference(ctx):
    rng = np.random.default_rng(99)
    compared = 0
    for cls in (0, 3):
        data = datagen.block(cls, 40000).tobytes()
        good, nbits = ans1model.encode(data, 1)
        for trial in range(24):
            bad = refinputs.corrupt(rng, good, trial % 8)
            nb = min(nbits, len(bad) * 8)
            want = model_decode(bad, nb, len(data))
            ok, out, used = gpu_decode(ctx, bad, nb, len(data))
            assert ok == want[0], (cls, trial)
            if ok:
                assert out == want[1] and used == want[2], (cls, trial)
            compared += 1
    assert compared == 48


def _ctx_header_bits(chunk):
    """bit length of every context header of an order-1 chunk (the model's own writer)"""
    freqs = ans1model._histogram(chunk, 1)
    lens = []
    for k in range(256):
        bs = ans1model._Bits()
        alphabet = katmodels._normalize(freqs[k], sum(freqs[k]), 1 << 11)
        katmodels._encode_alphabet(bs, alphabet)
        ans1model._header_freqs(bs, alphabet, freqs[k], 11)
        lens.append(bs.n)
    return lens


def test_stale_context_of_the_previous_chunk(ctx):
    """Damage that sends a chunk into a context that is empty there but was filled in the previous chunk of the block: that
    context keeps its tables (decodeHeader `continue`, ANSRangeDecoder.java:467-468).  Context 255's header in chunk 1 is
    replaced by ALPHABET_0; chunk 1 then decodes through chunk 0's table for it."""
    rng = np.random.default_rng(3)
    tail = bytes(rng.integers(250, 256, 2000, dtype=np.uint8))
    data = datagen.block(3, MIB4).tobytes() + tail
    assert 0xFF in data[:MIB4 - 1]                             # context 255 is filled in chunk 0
    bits, nbits = gpu_encode(ctx, data)
    want = ans1model.encode(data, 1)
    assert (bits, nbits) == want
    n0 = ans1model.encode(data[:MIB4], 1)[1]
    lens = _ctx_header_bits(tail)
    at = n0 + 3 + sum(lens[:255])
    s = format(int.from_bytes(bits, "big"), "0%db" % (8 * len(bits)))[:nbits]
    assert s[at] == "1" and lens[255] > 2                      # context 255 is present in the tail chunk
    s2 = s[:at] + "01" + s[at + lens[255]:]
    nb2 = len(s2)
    bad = int(s2 + "0" * (-nb2 % 8), 2).to_bytes((nb2 + 7) // 8, "big")
    r, out, _, _ = ans1model.decode(bad, nb2, len(data), 1)
    assert out[:MIB4] == data[:MIB4]
    ok, got, _ = gpu_decode(ctx, bad, nb2, len(data))
    assert ok == (r == len(data)) and (not ok or got == out)
    # chunk 0's payload size off by one: chunk 0 stops early (n != sz), the reference reads no further than its payload, and the
    # bits consumed say so although chunk 1 follows
    p0 = 3 + sum(_ctx_header_bits(data[:MIB4]))
    s3 = s[:p0 + 7] + ("1" if s[p0 + 7] == "0" else "0") + s[p0 + 8:]
    bad3 = int(s3 + "0" * (-nbits % 8), 2).to_bytes((nbits + 7) // 8, "big")
    r3, out3, used3, clean3 = ans1model.decode(bad3, nbits, len(data), 1)
    assert r3 == len(data) and not clean3 and used3 <= n0 + 8 < nbits
    ok, got, used = gpu_decode(ctx, bad3, nbits, len(data))
    assert ok and got == out3 and used == used3


def _ans1_block_from_none(stream, nbits, n, nfun):
    """the block stream EncodingTask.encodeBlock writes under ANS1, from the one it writes under NONE for the same chain (the
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
    bits, eb = ans1model.encode(payload, 1)
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
    rng = np.random.default_rng(11)
    blocks = [datagen.block(c, 30000 + 999 * c).tobytes() for c in range(5)]
    blocks += [b"0123456789abcde", bytes(rng.integers(0, 256, 5000, dtype=np.uint8)), bytes(rng.integers(0, 4, 777, dtype=np.uint8)), b"xy" * 20]
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    ref = np.zeros((len(blocks), ostride), dtype=np.uint8)
    rn = kz.encode_blocks(ctx, chain, "NONE", inp, bs, lens, ref, ostride)
    nfun = len(chain.split("+"))
    want = [_ans1_block_from_none(ref[i].tobytes(), rn[i].bits, len(b), nfun) for i, b in enumerate(blocks)]
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    res = kz.encode_blocks(ctx, chain, "ANS1", inp, bs, lens, out, ostride)
    for i in range(len(blocks)):
        assert res[i].status == 0 and res[i].bits == want[i][1], (chain, i)
        assert out[i, :(res[i].bits + 7) // 8].tobytes() == want[i][0], (chain, i)
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(blocks), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, chain, "ANS1", bs, out, ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert res2[i].status == 0 and res2[i].length == len(b) and dec[i, :len(b)].tobytes() == b, (chain, i)
    # device memory, and the asynchronous calls
    d_in = torch.from_numpy(inp).cuda()
    d_out = torch.zeros((len(blocks), ostride), dtype=torch.uint8, device="cuda")
    res_d = kz.encode_blocks(ctx, chain, "ANS1", d_in.data_ptr(), bs, lens, d_out.data_ptr(), ostride, kz.MEM_DEVICE)
    host = d_out.cpu().numpy()
    for i in range(len(blocks)):
        assert res_d[i].bits == res[i].bits and host[i, :(res[i].bits + 7) // 8].tobytes() == want[i][0], (chain, i)
    d_dec = torch.zeros((len(blocks), bs), dtype=torch.uint8, device="cuda")
    kz.decode_blocks(ctx, chain, "ANS1", bs, d_out.data_ptr(), ostride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
    assert np.array_equal(d_dec.cpu().numpy(), dec)
    out2 = np.zeros_like(out)
    job = kz.submit_encode_blocks(ctx, chain, "ANS1", inp, bs, lens, out2, ostride)
    job.wait()
    assert np.array_equal(out2, out)
    dec2 = np.zeros_like(dec)
    kz.submit_decode_blocks(ctx, chain, "ANS1", bs, out, ostride, bits, dec2, bs).wait()
    assert np.array_equal(dec2, dec)


def test_batched_text_chain_round_trip(ctx):
    blocks = [textgen.bulk_text(40000, s).tobytes() for s in range(3)] + [datagen.block(c, 20000).tobytes() for c in range(3)] + [b"short text"]
    inp, lens, bs = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    ctx.set_block_size(bs)
    res = kz.encode_blocks(ctx, "TEXT+UTF+BWT+RANK+ZRLT", "ANS1", inp, bs, lens, out, ostride)
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(blocks), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, "TEXT+UTF+BWT+RANK+ZRLT", "ANS1", bs, out, ostride, bits, dec, bs)
    for i, b in enumerate(blocks):
        assert res[i].status == 0 and res2[i].status == 0 and dec[i, :len(b)].tobytes() == b, i


def test_whole_stream(ctx, monkeypatch):
    """kz_compress == the model's .knz (katmodels.knz_stream with the ANS1 block streams), kz_decompress restores the input."""
    data = datagen.stream(3, 20000).tobytes() + b"tail"
    orig = katmodels._knz_block

    def block_ans1(block, names, entropy, block_size, static_words):
        s, w = orig(block, names, "NONE", block_size, static_words)
        return _ans1_block_from_none(s, w, len(block), len(names))
    monkeypatch.setattr(katmodels, "_knz_block", block_ans1)
    cos = kz.CompressedOutputStream(ctx, "BWT+RANK+ZRLT", "ANS1", 20000)
    cos.write(data)
    cos.close()
    want = katmodels.knz_stream(data, ["BWT", "RANK", "ZRLT"], "ANS1", 20000, [], kz.knz_index(cos.output)["inputSize"])
    assert cos.output == want
    assert kz.CompressedInputStream(ctx, cos.output).read() == data


@pytest.mark.parametrize("form", ["2", "1", ""])
def test_text_inverse_under_ans1(form, monkeypatch, capfd):
    """TEXT under ANS1 is TextCodec1: the serial device form must decode it as such and finish every block it takes (KZ_TEXT_GPU=2:
    told TextCodec2, it would size its output for the other codec and hand every block back), the row form hands its blocks to the
    host (KZ_TEXT_GPU=1), and by default a batch of 512 blocks or more stays on the host stage (no device launch)."""
    data = b"".join(textgen.bulk_text(8192, s % 7).tobytes() for s in range(520))
    bs = 8192
    monkeypatch.setenv("KZ_TEXT_GPU", "0")
    host = kz.Context(0)
    cos = kz.CompressedOutputStream(host, "TEXT", "ANS1", bs)
    cos.write(data)
    cos.close()
    knz = cos.output
    assert kz.CompressedInputStream(host, knz).read() == data
    if form:
        monkeypatch.setenv("KZ_TEXT_GPU", form)
    else:
        monkeypatch.delenv("KZ_TEXT_GPU", raising=False)
    monkeypatch.setenv("KZ_TEXT_GPU_TRACE", "1")
    dev = kz.Context(0)
    capfd.readouterr()
    assert kz.CompressedInputStream(dev, knz).read() == data
    err = capfd.readouterr().err
    trace = [l.split() for l in err.splitlines() if l.startswith("[textgpu] took")]
    took, fin = sum(int(t[2]) for t in trace), sum(int(t[5]) for t in trace)
    if form == "2":
        assert took > 0 and fin == took, err[-400:]
    if form == "1":
        assert took > 0 and fin == 0, err[-400:]
    if form == "":
        assert not trace, err[-400:]


def _text_static_words():
    """DICT_EN_1024 as the generated header holds it (the same reader as test_oracle.py's)"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "kzo_text_dict.h")).read()
    return b"".join(m.group(1).encode() for m in re.finditer(r'^\s*"([^"]*)"', src, re.M))


@pytest.mark.parametrize("fwd", ["0", "1"])
def test_text_forward_under_ans1_is_textcodec1(fwd, monkeypatch):
    """The TEXT forward of an ANS1 stream is TextCodec1 (TransformFactory.java:275-286), on the host stage and with the device
    forward switched on (that form only writes TextCodec2 and must stay out): each block's ANS1 payload, decoded by the model,
    equals katmodels.text_forward(variant 1) and differs from variant 2."""
    monkeypatch.setenv("KZ_TEXT_FWD_GPU", fwd)
    c = kz.Context(0)
    bs = 24000
    blocks = [textgen.bulk_text(bs, s).tobytes() for s in range(3)]
    c.set_block_size(bs)
    inp, lens, _ = _batch(blocks)
    ostride = kz.max_block_stream_bytes(bs)
    out = np.zeros((len(blocks), ostride), dtype=np.uint8)
    res = kz.encode_blocks(c, "TEXT", "ANS1", inp, bs, lens, out, ostride)
    dic = katmodels.text_static_dictionary(_text_static_words())
    differs = 0
    for i, b in enumerate(blocks):
        s = out[i].tobytes()
        mode = s[0]
        assert res[i].status == 0 and not (mode & 0x80) and not (mode & 0x08), i      # entropy coded, TEXT applied
        ds = ((mode >> 5) & 3) + 1
        post = int.from_bytes(s[1:1 + ds], "big")
        nb = res[i].bits - 8 * (2 + ds)
        r, got, _, _ = ans1model.decode(s[2 + ds:], nb, post, 1)
        ok1, want1, _ = katmodels.text_forward(b, 1, bs, dic)
        ok2, want2, _ = katmodels.text_forward(b, 2, bs, dic)
        assert r == post and ok1 and got == bytes(want1), i
        differs += bytes(want2) != got
    assert differs == len(blocks)
