"""The batched encode and decode drivers (kanzi_amd/csrc/kz_encode.hip, kz_decode.hip) under each of their modes: one pass, the host
chunk pipelines, the device TEXT / UTF forward, and block checksums (which keep the decoder on its one-pass path).  One batch of 20
blocks of 16 KiB whose blocks TEXT takes, UTF takes or neither takes, with lengths 0, 9, 15, 16 and a ragged last block, in host and in
device memory: every mode's streams, bits, skip flags and lengths are the oracle's per block, and every decode restores the input."""
import numpy as np
import pytest

import kanzi_amd as kz
import oracle
import textgen

pytestmark = pytest.mark.gpu

BS, NB = 16384, 20
CHAINS = {"ans0": ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0"), "level6": kz.level_chain(6)}
MODES = ["default", "host_chunks", "device_forward", "checksum32"]


def switches(mode, name):
    if mode == "host_chunks":
        return {"KZ_HOST_CHUNK": "8", "KZ_HOST_CHUNK_DEC": "8"}
    if mode == "device_forward":                    # TextCodec2 streams (ANS0) and TextCodec1 streams (level 6: FPAQ) have switches of their own
        return {"KZ_TEXT_FWD_GPU": "1", "KZ_TEXT_FWD_GPU_MIN": "1"} if name == "ans0" else {"KZ_TEXT1_FWD_GPU": "1", "KZ_TEXT1_FWD_GPU_MIN": "1"}
    return {}


_BATCH, _REF = [], {}


def batch():
    """(rows, lengths): english / utf8 / xml / random in turn, short blocks in the middle of the chunks, a ragged last block"""
    if not _BATCH:
        c = textgen.cases()
        kinds = [c["english"], c["utf8"], c["xml"], c["random"]]
        rows = np.zeros((NB, BS), dtype=np.uint8)
        for i in range(NB):
            src = kinds[i % 4]
            off = (i // 4) * BS % (len(src) - BS)
            rows[i] = np.frombuffer(src[off:off + BS], dtype=np.uint8)
        lens = np.full(NB, BS, dtype=np.int32)
        lens[2], lens[5], lens[9], lens[12], lens[-1] = 0, 9, 15, 16, 12345
        _BATCH.extend([rows, lens])
    return _BATCH


def reference(name, checksum):
    """the oracle's (stream, bits, skip flags, length) per block, computed once per chain and checksum kind"""
    if (name, checksum) not in _REF:
        rows, lens = batch()
        chain, ent = CHAINS[name]
        _REF[name, checksum] = [oracle.encode_block(chain, ent, rows[i, :lens[i]], checksum=checksum, block_size=BS) if lens[i] else None for i in range(NB)]
    return _REF[name, checksum]


def check_streams(res, out, ref):
    for i, want in enumerate(ref):
        assert res[i].status == 0, i
        if want is None:                            # the empty block: no bits, no bytes (the oracle codes no block for it)
            assert (res[i].bits, res[i].length) == (0, 0), i
            continue
        s, w, sf, pl = want
        assert (res[i].bits, res[i].skipFlags, res[i].length) == (w, sf, pl), i
        assert out[i, :(w + 7) // 8].tobytes() == s, i


def check_blocks(res, dec, rows, lens):
    for i in range(NB):
        assert res[i].status == 0 and res[i].length == lens[i], i
        assert np.array_equal(dec[i, :lens[i]], rows[i, :lens[i]]), i


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CHAINS))
def test_every_driver_mode_codes_the_same_blocks(ctx, monkeypatch, name, mode):
    torch = pytest.importorskip("torch")
    chain, ent = CHAINS[name]
    checksum = 32 if mode == "checksum32" else 0
    rows, lens = batch()
    ref = reference(name, checksum)
    assert len({r[2] for r in ref if r is not None}) >= 3      # TEXT taken / UTF taken / neither: the case list is not one-sided
    for k, v in switches(mode, name).items():
        monkeypatch.setenv(k, v)
    ostride = kz.max_block_stream_bytes(BS)
    ctx.set_block_size(BS)
    ctx.set_checksum(checksum)
    try:
        out_h = np.zeros((NB, ostride), dtype=np.uint8)
        res_h = kz.encode_blocks(ctx, chain, ent, rows, BS, lens, out_h, ostride)
        check_streams(res_h, out_h, ref)
        d_in = torch.from_numpy(rows).cuda()
        d_out = torch.zeros((NB, ostride), dtype=torch.uint8, device="cuda")
        res_d = kz.encode_blocks(ctx, chain, ent, d_in.data_ptr(), BS, lens, d_out.data_ptr(), ostride, kz.MEM_DEVICE)
        check_streams(res_d, d_out.cpu().numpy(), ref)
        bits = np.array([r.bits for r in res_h], dtype=np.int64)
        dec_h = np.zeros((NB, BS), dtype=np.uint8)
        check_blocks(kz.decode_blocks(ctx, chain, ent, BS, out_h, ostride, bits, dec_h, BS), dec_h, rows, lens)
        d_dec = torch.zeros((NB, BS), dtype=torch.uint8, device="cuda")
        res2 = kz.decode_blocks(ctx, chain, ent, BS, d_out.data_ptr(), ostride, bits, d_dec.data_ptr(), BS, kz.MEM_DEVICE)
        check_blocks(res2, d_dec.cpu().numpy(), rows, lens)
    finally:
        ctx.set_checksum(0)
