"""CM (the context-model binary coder) timings: one 4 MiB block alone (English, random, sensor-like) through NONE&CM -- the k_cm_enc /
k_cm_dec kernel times and ns per coded bit -- and then B x 4 MiB blocks of the bench's mix held in HBM, next to FPAQ (the other
one-chain-per-block coder) and ANS0 on the same input in the same run (the stage timers: encode = the entropy stage inside
kz_encode_blocks, decode = the one inside kz_decode_blocks).  A CM block occupies a whole CU (its predictor fills the LDS), so a batch
takes ceil(B / CUs) times a lone block: if that estimate passes MAX_S seconds per direction, B is cut to fit and the line says so.
Diagnostic.
   B=2048 MAX_S=150 python tools/cm_probe.py          (CODERS=CM,FPAQ,ANS0 by default)"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen, textgen

B = int(os.environ.get("B", "2048")); D = 64; bs = 4 << 20
MAX_S = float(os.environ.get("MAX_S", "150"))
coders = os.environ.get("CODERS", "CM,FPAQ,ANS0").split(",")
dev = torch.device("cuda", 0)
ctx = kz.Context(0)
ctx.set_timing(True)
o_stride = kz.max_block_stream_bytes(bs)
print(json.dumps({"blocks": B, "block_bytes": bs}), flush=True)


def run(chain, coder, d_in, n_blocks):
    """-> (encode stage ms, decode stage ms, kernel ms of both directions, results) of the measured pass"""
    d_enc = torch.zeros((n_blocks, o_stride), dtype=torch.uint8, device=dev)
    d_dec = torch.zeros((n_blocks, bs), dtype=torch.uint8, device=dev)
    lengths = np.full(n_blocks, bs, dtype=np.int32)
    ctx.set_kernel_timing(True); ctx.reset_kernel_timing(); ctx.reset_timing()
    res = kz.encode_blocks(ctx, chain, coder, d_in.data_ptr(), bs, lengths, d_enc.data_ptr(), o_stride, kz.MEM_DEVICE)
    torch.cuda.synchronize()
    st_enc, kt_enc = ctx.stage_times(), ctx.kernel_times()
    bits = np.array([r.bits for r in res], dtype=np.int64)
    ctx.reset_kernel_timing(); ctx.reset_timing()
    res2 = kz.decode_blocks(ctx, chain, coder, bs, d_enc.data_ptr(), o_stride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
    torch.cuda.synchronize()
    st_dec, kt_dec = ctx.stage_times(), ctx.kernel_times()
    assert all(r.status == 0 for r in res) and all(r.status == 0 and r.length == bs for r in res2) and torch.equal(d_in, d_dec), (chain, coder)
    return st_enc.get("entropy_enc", {}).get("ms", 0.0), st_dec.get("entropy_dec", {}).get("ms", 0.0), kt_enc, kt_dec, res, bits


lone_s = 0.0
rng = np.random.default_rng(1)
for label, data in (("english", textgen.bulk_text(bs, 1)), ("random", rng.integers(0, 256, bs, dtype=np.uint8)), ("sensor", datagen.sensor_like(bs, 1))):
    d_in = torch.from_numpy(np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8)[:bs]).reshape(1, bs)).to(dev)
    row = {}
    for coder in ("CM", "FPAQ"):
        if label == "english":
            run("NONE", coder, d_in, 1)                                       # warm-up
        enc_ms, dec_ms, kt_enc, kt_dec, res, bits = run("NONE", coder, d_in, 1)
        raw = bool(res[0].mode & 0x80)                                        # stored raw: the coder still ran over the whole block
        row[coder] = {"enc_ms": round(enc_ms, 2), "dec_ms": round(dec_ms, 2), "raw_block": raw, "ratio": round(float(bits[0]) / 8 / bs, 4),
                      "enc_ns_per_bit": round(enc_ms * 1e6 / (8 * bs), 2), "dec_ns_per_bit": None if raw else round(dec_ms * 1e6 / (8 * bs), 2),
                      "kernels_enc_ms": {k: round(v["ms"], 2) for k, v in kt_enc.items() if coder.lower() in k},
                      "kernels_dec_ms": {k: round(v["ms"], 2) for k, v in kt_dec.items() if coder.lower() in k}}
        if coder == "CM":
            lone_s = max(lone_s, enc_ms / 1e3, dec_ms / 1e3)
    print(json.dumps({"lone 4 MiB block, " + label: row}), flush=True)

cus = torch.cuda.get_device_properties(0).multi_processor_count
rounds = max(1, int(MAX_S / max(lone_s, 1e-3)))
Bcm = min(B, rounds * cus)
host = np.stack([datagen.block(k, bs) for k in range(D)])                     # the bench's mix (SURVEY 8d generator), tiled
d_all = torch.from_numpy(host).to(dev).repeat((B + D - 1) // D, 1)[:B].contiguous()
for coder in coders:
    nb = Bcm if coder == "CM" else B
    d_in = d_all[:nb]
    run("NONE", coder, d_in[:min(nb, cus)], min(nb, cus))                     # warm-up (one round of CUs)
    t0 = time.perf_counter()
    enc_ms, dec_ms, kt_enc, kt_dec, res, bits = run("NONE", coder, d_in, nb)
    print(json.dumps({"NONE&" + coder: {
        "blocks": nb, "cut_to_fit_MAX_S": nb != B, "wall_s": round(time.perf_counter() - t0, 2),
        "entropy_enc_ms": round(enc_ms, 2), "entropy_dec_ms": round(dec_ms, 2),
        "enc_ms_per_2048_blocks": round(enc_ms * 2048 / nb, 1), "dec_ms_per_2048_blocks": round(dec_ms * 2048 / nb, 1),
        "ratio": round(float(bits.sum()) / 8 / (nb * bs), 4), "raw_blocks": sum(1 for r in res if r.mode & 0x80)}}), flush=True)
