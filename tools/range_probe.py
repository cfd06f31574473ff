"""RANGE (order-0 range coder) on the bench's block mix: the entropy stages of NONE&RANGE and BWT+RANK+ZRLT&RANGE on B x 4 MiB blocks
held in HBM (the stage timers: encode = the entropy stage inside kz_encode_blocks, decode = the one inside kz_decode_blocks), the
RANGE kernels' times and the coded size, next to ANS0 (the same chunked order-0 model) and FPAQ (the other one-chain-per-block
decoder) on the same input in the same run.  Diagnostic.
   B=2048 python tools/range_probe.py          (CODERS=RANGE,ANS0,FPAQ by default)"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

B = int(os.environ.get("B", "2048")); D = 64; bs = 4 << 20
coders = os.environ.get("CODERS", "RANGE,ANS0,FPAQ").split(",")
dev = torch.device("cuda", 0)
host = np.stack([datagen.block(k, bs) for k in range(D)])                 # the bench's mix (SURVEY 8d generator), tiled
d_in = torch.from_numpy(host).to(dev).repeat((B + D - 1) // D, 1)[:B].contiguous()
o_stride = kz.max_block_stream_bytes(bs)
d_enc = torch.zeros((B, o_stride), dtype=torch.uint8, device=dev)
d_dec = torch.zeros((B, bs), dtype=torch.uint8, device=dev)
lengths = np.full(B, bs, dtype=np.int32)
ctx = kz.Context(0)
ctx.set_timing(True)
print(json.dumps({"blocks": B, "block_bytes": bs}), flush=True)
for chain in ("NONE", "BWT+RANK+ZRLT"):
    for coder in coders:
        for it in range(2):                                                # warm-up, then the measured pass
            ctx.set_kernel_timing(it == 1); ctx.reset_kernel_timing(); ctx.reset_timing()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = kz.encode_blocks(ctx, chain, coder, d_in.data_ptr(), bs, lengths, d_enc.data_ptr(), o_stride, kz.MEM_DEVICE)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            st_enc = ctx.stage_times()
            kt_enc = ctx.kernel_times()
            bits = np.array([r.bits for r in res], dtype=np.int64)
            ctx.reset_kernel_timing(); ctx.reset_timing()
            res2 = kz.decode_blocks(ctx, chain, coder, bs, d_enc.data_ptr(), o_stride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
            torch.cuda.synchronize(); t2 = time.perf_counter()
            st_dec = ctx.stage_times()
            kt_dec = ctx.kernel_times()
        assert all(r.status == 0 for r in res) and all(r.status == 0 and r.length == bs for r in res2) and torch.equal(d_in, d_dec), (chain, coder)
        mine = ("range", "ans_enc_scan", "ans_enc_concat") if coder == "RANGE" else ("ans",) if coder == "ANS0" else ("fpaq",)
        print(json.dumps({chain + "&" + coder: {
            "encode_s": round(t1 - t0, 4), "decode_s": round(t2 - t1, 4),
            "entropy_enc_ms": round(st_enc.get("entropy_enc", {}).get("ms", 0.0), 2),
            "entropy_dec_ms": round(st_dec.get("entropy_dec", {}).get("ms", 0.0), 2),
            "coded_bytes": int((bits.sum() + 7) // 8), "ratio": round(float(bits.sum()) / 8 / (B * bs), 4),
            "raw_blocks": sum(1 for r in res if r.mode & 0x80),
            "kernels_enc_ms": {k: round(v["ms"], 2) for k, v in kt_enc.items() if any(m in k for m in mine)},
            "kernels_dec_ms": {k: round(v["ms"], 2) for k, v in kt_dec.items() if any(m in k for m in mine)}}}), flush=True)
