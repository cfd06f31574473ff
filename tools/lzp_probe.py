"""LZP next to LZ on the same batch, B x 4 MiB blocks held in HBM, kernel timers on.  Diagnostic.
  Inputs: (a) the bench's block mix, (b) exe_like blocks only (the one synthetic class LZP applies to at this size).
  Per input and transform (entropy NONE): the forward and inverse kernel times (k_lzp_fwd / k_lzp_inv next to the untouched
  k_lz_fwd / k_lz_inv), per GiB of input too, the share of blocks the transform applied to, the coded bytes, and the round trip.
   B=2048 python tools/lzp_probe.py"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

B = int(os.environ.get("B", "2048")); D = 64; bs = 4 << 20
dev = torch.device("cuda", 0)
host = np.stack([datagen.block(k, bs) for k in range(D)])                 # the bench's mix (SURVEY 8d generator), tiled
d_mix = torch.from_numpy(host).to(dev).repeat((B + D - 1) // D, 1)[:B].contiguous()
hexe = np.stack([np.frombuffer(bytes(datagen.exe_like(bs, k + 1)), dtype=np.uint8) for k in range(16)])
d_exe = torch.from_numpy(hexe).to(dev).repeat((B + 15) // 16, 1)[:B].contiguous()
o_stride = kz.max_block_stream_bytes(bs)
d_enc = torch.zeros((B, o_stride), dtype=torch.uint8, device=dev)
d_dec = torch.zeros((B, bs), dtype=torch.uint8, device=dev)
ctx = kz.Context(0)
ctx.set_timing(True)


def run(d_in, chain, pick):
    lengths = np.full(B, bs, dtype=np.int32)
    for it in range(2):                                                    # warm-up, then the measured pass
        ctx.set_kernel_timing(it == 1); ctx.reset_kernel_timing(); ctx.reset_timing()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = kz.encode_blocks(ctx, chain, "NONE", d_in.data_ptr(), bs, lengths, d_enc.data_ptr(), o_stride, kz.MEM_DEVICE)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        kt_enc = ctx.kernel_times()
        bits = np.array([r.bits for r in res], dtype=np.int64)
        ctx.reset_kernel_timing(); ctx.reset_timing()
        res2 = kz.decode_blocks(ctx, chain, "NONE", bs, d_enc.data_ptr(), o_stride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        kt_dec = ctx.kernel_times()
    assert all(r.status == 0 and r.length == bs for r in res2) and torch.equal(d_in, d_dec), chain
    ctx.set_kernel_timing(False)
    gib = B * bs / float(1 << 30)
    ke = {k: round(v["ms"], 2) for k, v in kt_enc.items() if pick in k}
    kd = {k: round(v["ms"], 2) for k, v in kt_dec.items() if pick in k}
    applied = sum(1 for r in res if not (r.skipFlags & 0x80))
    row = {"blocks": B, "applied": applied, "applied_share": round(applied / B, 3), "coded_bytes": int((bits.sum() + 7) // 8),
           "encode_MBps": round(B * bs / 1e6 / (t1 - t0), 1), "decode_MBps": round(B * bs / 1e6 / (t2 - t1), 1),
           "kernels_fwd_ms": ke, "kernels_inv_ms": kd, "fwd_ms": round(sum(ke.values()), 2), "inv_ms": round(sum(kd.values()), 2),
           "fwd_ms_per_GiB": round(sum(ke.values()) / gib, 3), "inv_ms_per_GiB": round(sum(kd.values()) / gib, 3)}
    print(json.dumps({chain: row}), flush=True)
    return row


for name, d_in in (("mix", d_mix), ("exe_like", d_exe)):
    print(json.dumps({"input": name, "blocks": B}), flush=True)
    lz = run(d_in, "LZ", "k_lz_")
    lzp = run(d_in, "LZP", "k_lzp_")
    print(json.dumps({"lzp_over_lz": {"input": name, "forward": round(lzp["fwd_ms"] / lz["fwd_ms"], 3),
                                      "inverse": round(lzp["inv_ms"] / max(lz["inv_ms"], 1e-9), 3) if lz["inv_ms"] else None}}), flush=True)
