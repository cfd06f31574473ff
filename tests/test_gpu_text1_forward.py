"""The device TEXT forward of TextCodec1 streams (FPAQ / CM / ANS1: kanzi_amd/csrc/kz_text_fwd_gpu.hip, k_tf_* at TextCodec1's seams)
against the oracle on the case set of tests/text1cases.py (checked on the CPU by tests/test_text1_cases.py).  KZ_TEXT1_FWD_GPU=1
puts the stage on the device; its trace lines begin with "[textfwd1]" ("[textfwd] " stays TextCodec2's alone), and the counts in
them show that the device finished what the case set marks for it, so a path that did not run fails the test."""
import numpy as np
import pytest
import torch

import kanzi_amd as kz
import oracle
import text1cases
import textgen

pytestmark = pytest.mark.gpu

LEVEL6 = "TEXT+UTF+BWT+SRT+ZRLT"
_CASES = {}


def _cases(bs):
    if bs not in _CASES:
        _CASES[bs] = text1cases.cases(bs)
    return _CASES[bs]


def _trace(err):
    """(took, finished, kept) of every "[textfwd1] took" line, and the lines that are TextCodec2's"""
    t1 = [(int(x[2]), int(x[5]), int(x[7])) for x in (l.split() for l in err.splitlines() if l.startswith("[textfwd1] took"))]
    return t1, [l for l in err.splitlines() if l.startswith("[textfwd] ")]


def _batch(blocks, bs):
    """the blocks and one empty slot in the middle -> (rows, lengths)"""
    blocks = list(blocks)
    blocks.insert(len(blocks) // 2, b"")
    inp = np.zeros((len(blocks), bs), dtype=np.uint8)
    for i, d in enumerate(blocks):
        inp[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    return blocks, inp, np.array([len(d) for d in blocks], dtype=np.int32)


def _encode(ctx, chain, ent, inp, lens, bs, device=False):
    ostride = kz.max_block_stream_bytes(bs)
    if device:
        d_in = torch.from_numpy(inp).cuda()
        d_out = torch.zeros((len(lens), ostride), dtype=torch.uint8, device="cuda")
        res = kz.encode_blocks(ctx, chain, ent, d_in.data_ptr(), bs, lens, d_out.data_ptr(), ostride, kz.MEM_DEVICE)
        return res, d_out.cpu().numpy(), ostride
    out = np.zeros((len(lens), ostride), dtype=np.uint8)
    return kz.encode_blocks(ctx, chain, ent, inp, bs, lens, out, ostride), out, ostride


def _check_against_oracle(ctx, capfd, monkeypatch, chain, ent, bs, device):
    monkeypatch.setenv("KZ_TEXT1_FWD_GPU", "1")
    monkeypatch.setenv("KZ_TEXT_GPU_TRACE", "1")
    cases = _cases(bs)
    blocks, inp, lens = _batch([c.block for c in cases], bs)
    ctx.set_block_size(bs)
    capfd.readouterr()
    res, out, ostride = _encode(ctx, chain, ent, inp, lens, bs, device)
    t1, t2 = _trace(capfd.readouterr().err)
    for i, d in enumerate(blocks):
        so, w, sf, pl = oracle.encode_block(chain, ent, d, block_size=bs)
        if not d:                                   # the empty slot: no bits and no bytes, as in the oracle, which codes no block for it and
            sf = res[i].skipFlags                   # so has no skip flags to compare (the host stage's are compared in the CM / ANS1 test)
        assert res[i].status == 0 and (res[i].bits, res[i].skipFlags, res[i].length) == (w, sf, pl), (chain, bs, i, len(d))
        assert out[i, :(w + 7) // 8].tobytes() == so, (chain, bs, i)
    assert t1 and sum(t[1] for t in t1) >= sum(c.device for c in cases), (t1, sum(c.device for c in cases))
    assert not t2, t2
    bits = np.array([r.bits for r in res], dtype=np.int64)
    dec = np.zeros((len(blocks), bs), dtype=np.uint8)
    res2 = kz.decode_blocks(ctx, chain, ent, bs, out, ostride, bits, dec, bs)
    for i, d in enumerate(blocks):
        assert res2[i].status == 0 and res2[i].length == len(d) and dec[i, :len(d)].tobytes() == d, (chain, bs, i)


@pytest.mark.parametrize("bs", [32768, 1 << 20])
@pytest.mark.parametrize("chain", ["TEXT", "TEXT+UTF", LEVEL6])
def test_chains_against_the_oracle(chain, bs, monkeypatch, capfd):
    """Every case and one empty slot through kz_encode_blocks under FPAQ: status, bits, skip flags, length and stream bytes are the
    oracle's per block, the device finished at least the cases marked for it, and kz_decode_blocks returns the blocks."""
    ctx = kz.Context(0)
    try:
        _check_against_oracle(ctx, capfd, monkeypatch, chain, "FPAQ", bs, False)
    finally:
        ctx.close()


def test_device_input(monkeypatch, capfd):
    """The same with the batch and the streams in device memory (torch tensors, KZ_MEM_DEVICE)."""
    ctx = kz.Context(0)
    try:
        _check_against_oracle(ctx, capfd, monkeypatch, "TEXT", "FPAQ", 32768, True)
    finally:
        ctx.close()


@pytest.mark.parametrize("chain,ent", [("TEXT+UTF", "CM"), ("TEXT", "ANS1")])
def test_cm_and_ans1_streams_equal_the_host_stage(chain, ent, monkeypatch, capfd):
    """CM and ANS1 select TextCodec1 too: the streams with the stage on the device equal, byte for byte, those of the host stage
    (KZ_TEXT1_FWD_GPU=0: the code path pinned against the models by the existing suites); only the first run shows finished blocks."""
    bs = 32768
    cases = _cases(bs)
    blocks, inp, lens = _batch([c.block for c in cases], bs)
    monkeypatch.setenv("KZ_TEXT_GPU_TRACE", "1")
    runs = []
    for sw in ("1", "0"):
        monkeypatch.setenv("KZ_TEXT1_FWD_GPU", sw)
        ctx = kz.Context(0)
        try:
            ctx.set_block_size(bs)
            capfd.readouterr()
            res, out, _ = _encode(ctx, chain, ent, inp, lens, bs)
            t1, t2 = _trace(capfd.readouterr().err)
        finally:
            ctx.close()
        assert all(r.status == 0 for r in res) and not t2
        runs.append(([(r.bits, r.skipFlags, r.length) for r in res], [out[i, :(res[i].bits + 7) // 8].tobytes() for i in range(len(blocks))], t1))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert sum(t[1] for t in runs[0][2]) >= sum(c.device for c in cases) and not runs[1][2], (runs[0][2], runs[1][2])


def test_streams(monkeypatch, capfd):
    """kz_compress on 600 blocks of 8 192 bytes of mixed text at level 6 (chunks of 256 blocks: their TEXT stage runs on the device,
    they are not pre-staged on the host): the .knz is the oracle's, and so is kz_compress_device's from device memory."""
    monkeypatch.setenv("KZ_STREAM_CHUNK", "256")
    monkeypatch.setenv("KZ_TEXT1_FWD_GPU", "1")
    monkeypatch.setenv("KZ_TEXT_GPU_TRACE", "1")
    bs = 8192
    c = textgen.cases()
    base = (c["english"][:900000] + c["utf8"][:120000] + c["xml"][:300000] + c["random"][:70000] + c["english_crlf"][:400000] + c["many_words"][:500000]
            + c["english_escapes"])
    data = (base * 4)[:600 * bs - 777]
    want = oracle.compress(LEVEL6, "FPAQ", bs, data, jobs=8)
    ctx = kz.Context(0)
    try:
        capfd.readouterr()
        out = kz.CompressedOutputStream(ctx, LEVEL6, "FPAQ", bs)
        out.write(data)
        out.close()
        got = bytes(out.output)
        t1, t2 = _trace(capfd.readouterr().err)
        assert got == want
        assert sum(t[1] for t in t1) > 200 and not t2, t1
        src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        cap = kz.compress_bound(len(data), bs)
        dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        n = kz.compress_device(ctx, LEVEL6, "FPAQ", bs, src.data_ptr(), len(data), dst.data_ptr(), cap)
        t1, t2 = _trace(capfd.readouterr().err)
        assert dst[:n].cpu().numpy().tobytes() == want
        assert sum(t[1] for t in t1) > 200 and not t2, t1
    finally:
        ctx.close()


def test_4mib_blocks(monkeypatch, capfd):
    """The 4 MiB group (map of 2^19 slots) under TEXT+UTF & FPAQ equals the oracle.  No block of textgen.big_blocks wraps the word list
    under TextCodec1 (text1cases, case 11); the one the device keeps and gives back to the host stage is the block of invented words, in
    which two words share hash and length: kept - finished >= 1, and so took - finished >= 1."""
    monkeypatch.setenv("KZ_TEXT1_FWD_GPU", "1")
    monkeypatch.setenv("KZ_TEXT_GPU_TRACE", "1")
    bs = 4 << 20
    cases = _cases(bs)
    blocks = [c.block for c in cases]
    inp = np.zeros((len(blocks), bs), dtype=np.uint8)
    for i, d in enumerate(blocks):
        inp[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    lens = np.array([len(d) for d in blocks], dtype=np.int32)
    ctx = kz.Context(0)
    try:
        ctx.set_block_size(bs)
        capfd.readouterr()
        res, out, _ = _encode(ctx, "TEXT+UTF", "FPAQ", inp, lens, bs)
    finally:
        ctx.close()
    t1, t2 = _trace(capfd.readouterr().err)
    for i, d in enumerate(blocks):
        so, w, sf, pl = oracle.encode_block("TEXT+UTF", "FPAQ", d, block_size=bs)
        assert res[i].status == 0 and (res[i].bits, res[i].skipFlags, res[i].length) == (w, sf, pl), (cases[i], len(d))
        assert out[i, :(w + 7) // 8].tobytes() == so, cases[i]
    took, fin, kept = sum(t[0] for t in t1), sum(t[1] for t in t1), sum(t[2] for t in t1)
    assert fin >= sum(c.device for c in cases) and took - fin >= 1 and kept - fin >= 1 and not t2, t1


def test_switches(monkeypatch, capfd):
    """KZ_TEXT1_FWD_GPU=0: host stage; unset: by batch size -- a batch of 8 blocks is under the default of 64 and under
    KZ_TEXT1_FWD_GPU_MIN=9, and at KZ_TEXT1_FWD_GPU_MIN=8 --; TextCodec2's switch does not reach FPAQ streams.  Same streams every time."""
    bs = 32768
    blocks = [c.block for c in _cases(bs) if c.device][:8]
    inp = np.zeros((8, bs), dtype=np.uint8)
    for i, d in enumerate(blocks):
        inp[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    lens = np.array([len(d) for d in blocks], dtype=np.int32)
    monkeypatch.setenv("KZ_TEXT_GPU_TRACE", "1")
    monkeypatch.delenv("KZ_TEXT_FWD_GPU", raising=False)

    def run(env):
        for k in ("KZ_TEXT1_FWD_GPU", "KZ_TEXT1_FWD_GPU_MIN", "KZ_TEXT_FWD_GPU"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = kz.Context(0)
        try:
            ctx.set_block_size(bs)
            capfd.readouterr()
            res, out, _ = _encode(ctx, "TEXT", "FPAQ", inp, lens, bs)
        finally:
            ctx.close()
        err = capfd.readouterr().err
        return [out[i, :(res[i].bits + 7) // 8].tobytes() for i in range(8)], [l for l in err.splitlines() if l.startswith("[textfwd1]")], _trace(err)[1]

    host, l1, l2 = run({"KZ_TEXT1_FWD_GPU": "0"})
    assert not l1 and not l2
    s, l1, l2 = run({})
    assert s == host and not l1 and not l2
    s, l1, l2 = run({"KZ_TEXT1_FWD_GPU_MIN": "9"})
    assert s == host and not l1 and not l2
    s, l1, l2 = run({"KZ_TEXT1_FWD_GPU_MIN": "8"})
    assert s == host and l1 and not l2
    s, l1, l2 = run({"KZ_TEXT_FWD_GPU": "1"})
    assert s == host and not l1 and not l2
