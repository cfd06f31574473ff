"""RLT on the bench's block mix, B x 4 MiB blocks held in HBM, kernel timers on.  Diagnostic.
  1. the RLT kernels (forward and inverse, entropy NONE and FPAQ) next to the ZRLT kernels of a ZRLT run over the same batch, in this
     process.  (The FPAQ run takes min(B, FPAQ_B) blocks: its coder is the slow part and tells nothing about RLT; times are also
     given per GiB of input.)
  2. RLT+BWT+RANK+ZRLT & ANS0 against BWT+RANK+ZRLT & ANS0 on (a) the mix and (b) B blocks of class 4 (long runs): encode and decode
     MB/s, the forward BWT stage, total coded bytes.
   B=2048 python tools/rlt_probe.py"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

B = int(os.environ.get("B", "2048")); FB = min(B, int(os.environ.get("FPAQ_B", "256"))); D = 64; bs = 4 << 20
dev = torch.device("cuda", 0)
host = np.stack([datagen.block(k, bs) for k in range(D)])                 # the bench's mix (SURVEY 8d generator), tiled
d_mix = torch.from_numpy(host).to(dev).repeat((B + D - 1) // D, 1)[:B].contiguous()
host4 = np.stack([datagen.block(5 * k + 4, bs, 4) for k in range(16)])    # class 4 only
d_c4 = torch.from_numpy(host4).to(dev).repeat((B + 15) // 16, 1)[:B].contiguous()
o_stride = kz.max_block_stream_bytes(bs)
d_enc = torch.zeros((B, o_stride), dtype=torch.uint8, device=dev)
d_dec = torch.zeros((B, bs), dtype=torch.uint8, device=dev)
ctx = kz.Context(0)
ctx.set_timing(True)


def run(d_in, chain, entropy, nblk, pick):
    lengths = np.full(nblk, bs, dtype=np.int32)
    for it in range(2):                                                    # warm-up, then the measured pass
        ctx.set_kernel_timing(it == 1); ctx.reset_kernel_timing(); ctx.reset_timing()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = kz.encode_blocks(ctx, chain, entropy, d_in.data_ptr(), bs, lengths, d_enc.data_ptr(), o_stride, kz.MEM_DEVICE)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        st_enc, kt_enc = ctx.stage_times(), ctx.kernel_times()
        bits = np.array([r.bits for r in res], dtype=np.int64)
        ctx.reset_kernel_timing(); ctx.reset_timing()
        res2 = kz.decode_blocks(ctx, chain, entropy, bs, d_enc.data_ptr(), o_stride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        st_dec, kt_dec = ctx.stage_times(), ctx.kernel_times()
    assert all(r.status == 0 and r.length == bs for r in res2) and torch.equal(d_in[:nblk], d_dec[:nblk]), chain
    ctx.set_kernel_timing(False)
    gib = nblk * bs / float(1 << 30)
    ke = {k: round(v["ms"], 2) for k, v in kt_enc.items() if pick in k}
    kd = {k: round(v["ms"], 2) for k, v in kt_dec.items() if pick in k}
    first = 0x80 >> 0
    row = {"blocks": nblk, "encode_MBps": round(nblk * bs / 1e6 / (t1 - t0), 1), "decode_MBps": round(nblk * bs / 1e6 / (t2 - t1), 1),
           "coded_bytes": int((bits.sum() + 7) // 8), "first_stage_applied": sum(1 for r in res if not (r.skipFlags & first) and not (r.mode & 0x80 and r.length == bs)),
           "bwt_fwd_ms": round(st_enc.get("bwt_fwd", {}).get("ms", 0.0), 2),
           "kernels_fwd_ms": ke, "kernels_inv_ms": kd,
           "fwd_ms": round(sum(ke.values()), 2), "inv_ms": round(sum(kd.values()), 2),
           "fwd_ms_per_GiB": round(sum(ke.values()) / gib, 3), "inv_ms_per_GiB": round(sum(kd.values()) / gib, 3)}
    print(json.dumps({"%s&%s" % (chain, entropy): row}), flush=True)
    return row


z = run(d_mix, "ZRLT", "NONE", B, "k_zrlt")
r = run(d_mix, "RLT", "NONE", B, "k_rlt")
f = run(d_mix, "RLT", "FPAQ", FB, "k_rlt")
print(json.dumps({"rlt_over_zrlt": {"forward_NONE": round(r["fwd_ms_per_GiB"] / z["fwd_ms_per_GiB"], 2), "inverse_NONE": round(r["inv_ms_per_GiB"] / z["inv_ms_per_GiB"], 2),
                                    "forward_FPAQ": round(f["fwd_ms_per_GiB"] / z["fwd_ms_per_GiB"], 2), "inverse_FPAQ": round(f["inv_ms_per_GiB"] / z["inv_ms_per_GiB"], 2),
                                    "allowed": 3.0}}), flush=True)
for name, d_in in (("mix", d_mix), ("class4", d_c4)):
    print(json.dumps({"input": name}), flush=True)
    run(d_in, "BWT+RANK+ZRLT", "ANS0", B, "k_rlt")
    run(d_in, "RLT+BWT+RANK+ZRLT", "ANS0", B, "k_rlt")
