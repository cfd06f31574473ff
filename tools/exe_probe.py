"""EXE on executable-like blocks, B x 4 MiB blocks held in HBM, kernel timers on.  Diagnostic.
  1. per input (tests/execases.py x86_like and arm64_like, the bench's datagen.exe_like): the EXE kernels forward and inverse next to
     the RLT kernels of an RLT run over the same batch (RLT makes the same kind of passes: maps, scan, sizes, sum-scan, emit), the
     share of blocks taken and the coded bytes, entropy NONE.
  2. EXE+LZX & HUFFMAN against LZX & HUFFMAN, and EXE+BWT+RANK+ZRLT & ANS0 against BWT+RANK+ZRLT & ANS0: coded bytes (CHAIN_B blocks).
  3. a batch of one block: the wall time of the ten launches of the forward and the six of the inverse.
   B=2048 python tools/exe_probe.py        (B=64 CHAIN_B=16 for a short run)"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen, execases

B = int(os.environ.get("B", "2048")); CB = min(B, int(os.environ.get("CHAIN_B", "128"))); D = 8; bs = 4 << 20
dev = torch.device("cuda", 0)
o_stride = kz.max_block_stream_bytes(bs)
d_enc = torch.zeros((B, o_stride), dtype=torch.uint8, device=dev)
d_dec = torch.zeros((B, bs), dtype=torch.uint8, device=dev)
ctx = kz.Context(0)
ctx.set_timing(True)


def batch(gen):
    host = np.stack([np.frombuffer(bytes(gen(bs, k)), dtype=np.uint8) for k in range(D)])
    return torch.from_numpy(host).to(dev).repeat((B + D - 1) // D, 1)[:B].contiguous()


def run(d_in, chain, entropy, nblk, pick, passes=2):
    lengths = np.full(nblk, bs, dtype=np.int32)
    for it in range(passes):                                               # warm-up, then the measured pass
        ctx.set_kernel_timing(it == passes - 1); ctx.reset_kernel_timing(); ctx.reset_timing()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = kz.encode_blocks(ctx, chain, entropy, d_in.data_ptr(), bs, lengths, d_enc.data_ptr(), o_stride, kz.MEM_DEVICE)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        kt_enc = ctx.kernel_times()
        bits = np.array([r.bits for r in res], dtype=np.int64)
        ctx.reset_kernel_timing(); ctx.reset_timing()
        res2 = kz.decode_blocks(ctx, chain, entropy, bs, d_enc.data_ptr(), o_stride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        kt_dec = ctx.kernel_times()
    assert all(r.status == 0 and r.length == bs for r in res2) and torch.equal(d_in[:nblk], d_dec[:nblk]), chain
    ctx.set_kernel_timing(False)
    gib = nblk * bs / float(1 << 30)
    ke = {k: round(v["ms"], 2) for k, v in kt_enc.items() if pick in k}
    kd = {k: round(v["ms"], 2) for k, v in kt_dec.items() if pick in k}
    row = {"blocks": nblk, "encode_ms": round((t1 - t0) * 1e3, 2), "decode_ms": round((t2 - t1) * 1e3, 2),
           "coded_bytes": int((bits.sum() + 7) // 8), "first_stage_applied": sum(1 for r in res if not (r.skipFlags & 0x80)),
           "kernels_fwd_ms": ke, "kernels_inv_ms": kd, "fwd_ms_per_GiB": round(sum(ke.values()) / gib, 3), "inv_ms_per_GiB": round(sum(kd.values()) / gib, 3)}
    print(json.dumps({"%s&%s" % (chain, entropy): row}), flush=True)
    return row


for name, gen in (("x86_like", execases.x86_like), ("arm64_like", execases.arm64_like), ("exe_like", datagen.exe_like)):
    d_in = batch(gen)
    print(json.dumps({"input": name, "B": B}), flush=True)
    e = run(d_in, "EXE", "NONE", B, "k_exe")
    r = run(d_in, "RLT", "NONE", B, "k_rlt")
    print(json.dumps({"exe_over_rlt": {"input": name, "forward": round(e["fwd_ms_per_GiB"] / max(r["fwd_ms_per_GiB"], 1e-9), 2),
                                       "inverse": round(e["inv_ms_per_GiB"] / max(r["inv_ms_per_GiB"], 1e-9), 2),
                                       "taken": e["first_stage_applied"] / float(B)}}), flush=True)
    for chain, ent in (("LZX", "HUFFMAN"), ("EXE+LZX", "HUFFMAN"), ("BWT+RANK+ZRLT", "ANS0"), ("EXE+BWT+RANK+ZRLT", "ANS0")):
        run(d_in, chain, ent, CB, "k_exe")
    print(json.dumps({"one_block": name}), flush=True)
    run(d_in, "EXE", "NONE", 1, "k_exe", passes=3)
