"""ANS1 (order-1 range ANS) on the bench's block mix: the entropy stages of NONE&ANS1 and BWT+RANK+ZRLT&ANS1 on B x 4 MiB blocks held
in HBM (the stage timers: encode = the ANS1 stage inside kz_encode_blocks, decode = the ANS1 stage inside kz_decode_blocks), the
per-kernel times, and the decode latency of a single 4 MiB block.  Diagnostic.
   B=2048 python tools/ans1_probe.py"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

B = int(os.environ.get("B", "2048")); D = 64; bs = 4 << 20
dev = torch.device("cuda", 0)
host = np.stack([datagen.block(k, bs) for k in range(D)])                 # the bench's mix (SURVEY 8d generator), tiled
d_in = torch.from_numpy(host).to(dev).repeat((B + D - 1) // D, 1)[:B].contiguous()
o_stride = kz.max_block_stream_bytes(bs)
d_enc = torch.zeros((B, o_stride), dtype=torch.uint8, device=dev)
d_dec = torch.zeros((B, bs), dtype=torch.uint8, device=dev)
lengths = np.full(B, bs, dtype=np.int32)
ctx = kz.Context(0)
ctx.set_timing(True)
out = {"blocks": B, "block_bytes": bs}
for chain in ("NONE", "BWT+RANK+ZRLT"):
    for it in range(2):                                                    # warm-up, then the measured pass
        ctx.set_kernel_timing(it == 1); ctx.reset_kernel_timing(); ctx.reset_timing()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = kz.encode_blocks(ctx, chain, "ANS1", d_in.data_ptr(), bs, lengths, d_enc.data_ptr(), o_stride, kz.MEM_DEVICE)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        st_enc = ctx.stage_times()
        kt_enc = ctx.kernel_times()
        bits = np.array([r.bits for r in res], dtype=np.int64)
        ctx.reset_kernel_timing(); ctx.reset_timing()
        res2 = kz.decode_blocks(ctx, chain, "ANS1", bs, d_enc.data_ptr(), o_stride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        st_dec = ctx.stage_times()
        kt_dec = ctx.kernel_times()
    assert all(r.status == 0 and r.length == bs for r in res2) and torch.equal(d_in, d_dec), chain
    raw = sum(1 for r in res if r.mode & 0x80)
    out[chain + "&ANS1"] = {
        "encode_s": round(t1 - t0, 4), "decode_s": round(t2 - t1, 4),
        "entropy_enc_ms": round(st_enc.get("entropy_enc", {}).get("ms", 0.0), 2),
        "entropy_dec_ms": round(st_dec.get("entropy_dec", {}).get("ms", 0.0), 2),
        "ratio": round(float(bits.sum()) / 8 / (B * bs), 4), "raw_blocks": raw,
        "kernels_enc_ms": {k: round(v["ms"], 2) for k, v in kt_enc.items() if "ans" in k},
        "kernels_dec_ms": {k: round(v["ms"], 2) for k, v in kt_dec.items() if "ans" in k}}
    print(json.dumps({chain + "&ANS1": out[chain + "&ANS1"]}), flush=True)
# one 4 MiB block: decode latency (best of 5)
one = host[:1].copy()
enc1 = np.zeros((1, o_stride), dtype=np.uint8)
r1 = kz.encode_blocks(ctx, "NONE", "ANS1", one, bs, lengths[:1], enc1, o_stride)
b1 = np.array([r1[0].bits], dtype=np.int64)
d_one = torch.from_numpy(enc1).to(dev)
d_back = torch.zeros((1, bs), dtype=torch.uint8, device=dev)
lat = []
for _ in range(5):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    kz.decode_blocks(ctx, "NONE", "ANS1", bs, d_one.data_ptr(), o_stride, b1, d_back.data_ptr(), bs, kz.MEM_DEVICE)
    torch.cuda.synchronize(); lat.append(time.perf_counter() - t0)
assert torch.equal(d_back.cpu(), torch.from_numpy(one))
out["single_block_decode_ms"] = round(min(lat) * 1e3, 2)
print(json.dumps({"single_block_decode_ms": out["single_block_decode_ms"]}), flush=True)
