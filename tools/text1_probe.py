"""The TEXT forward of TextCodec1 streams on the host (KZ_TEXT1_FWD_GPU=0) and on the device (=1), same batches.  Diagnostic (needs a GPU).
  Input: the text-heavy mix (bench.text_mix: of 8 blocks 5 English, 1 XML, 1 UTF-8, 1 binary) at 4 MiB blocks, 64 / 128 / 256 / 512
  blocks held in HBM.  Chains: the level-6 encode TEXT+UTF+BWT+SRT+ZRLT & FPAQ, and TEXT+UTF & FPAQ.
  Per switch value, chain and batch size: one warm-up pass, then REPS timed kz_encode_blocks calls -> median, min, max (ms), and one
  more pass with KZ_TEXT_GPU_TRACE=1 whose "[textfwd1]" lines (blocks taken / finished / kept, the host passes) go to stderr, and with
  the kernel timers on: the eight largest kernel times of that pass.
  Each switch value runs in a child process of its own with a time limit.
   python tools/text1_probe.py [both|0|1] [share]      share: kz_host_share(share) first (8 on a 16-CPU box = one rank's two CPUs)
   REPS=5 SIZES=64,128,256,512 python tools/text1_probe.py"""
import json, os, subprocess, sys, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1] if len(sys.argv) > 1 else "both"
share = int(sys.argv[2]) if len(sys.argv) > 2 else 1
if mode == "both":
    for m in ("0", "1"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), m, str(share)], timeout=int(os.environ.get("LIMIT", "420")))
        if r.returncode:
            sys.exit(r.returncode)                                         # nothing more on the GPU behind a step that failed
    sys.exit(0)

sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["KZ_TEXT1_FWD_GPU"] = mode
os.environ.pop("KZ_TEXT_GPU_TRACE", None)
import numpy as np, torch
import kanzi_amd as kz
import bench

REPS = int(os.environ.get("REPS", "5"))
SIZES = [int(x) for x in os.environ.get("SIZES", "64,128,256,512").split(",")]
bs = 4 << 20
cpus = kz.load_library().kz_host_share(share)
d16 = torch.from_numpy(bench.text_mix(16, bs)).cuda()
ostride = kz.max_block_stream_bytes(bs)
ctx = kz.Context(0); ctx.set_block_size(bs)
print(json.dumps({"KZ_TEXT1_FWD_GPU": mode, "host_cpus": cpus, "reps": REPS}), flush=True)
for chain in ("TEXT+UTF+BWT+SRT+ZRLT", "TEXT+UTF"):
    for B in SIZES:
        d_in = d16.repeat((B + 15) // 16, 1)[:B].contiguous()
        d_enc = torch.zeros((B, ostride), dtype=torch.uint8, device="cuda")
        lens = np.full(B, bs, dtype=np.int32)
        ms = []
        for rep in range(REPS + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = kz.encode_blocks(ctx, chain, "FPAQ", d_in.data_ptr(), bs, lens, d_enc.data_ptr(), ostride, kz.MEM_DEVICE)
            torch.cuda.synchronize()
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3)
        assert all(r.status == 0 for r in res)
        ms.sort()
        print(json.dumps({"switch": mode, "chain": chain, "blocks": B, "median_ms": round(ms[len(ms) // 2], 1), "min_ms": round(ms[0], 1), "max_ms": round(ms[-1], 1),
                          "text_applied": sum(1 for r in res if not (r.skipFlags & 0x80)), "coded_bytes": int(sum(r.bits for r in res) // 8)}), flush=True)
        os.environ["KZ_TEXT_GPU_TRACE"] = "1"; ctx.reload_switches()
        sys.stderr.write("[probe] switch %s, %s, %d blocks:\n" % (mode, chain, B)); sys.stderr.flush()
        ctx.set_kernel_timing(True); ctx.reset_kernel_timing()
        kz.encode_blocks(ctx, chain, "FPAQ", d_in.data_ptr(), bs, lens, d_enc.data_ptr(), ostride, kz.MEM_DEVICE)
        kt = sorted(((round(v["ms"], 1), k) for k, v in ctx.kernel_times().items()), reverse=True)
        ctx.set_kernel_timing(False)
        os.environ.pop("KZ_TEXT_GPU_TRACE"); ctx.reload_switches()
        print(json.dumps({"switch": mode, "chain": chain, "blocks": B, "kernels_ms": {k: v for v, k in kt[:8]}}), flush=True)
        del d_in, d_enc
ctx.close()
