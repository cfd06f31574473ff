"""Many .knz streams in one call next to a loop of single-stream calls over the same buffers: N streams of one block each
(BWT+RANK+ZRLT&ANS0, block size 4 MiB, so a 64 KiB stream is one 64 KiB block), timed two ways in one process:
   many   compress_many_device + decompress_many_device
   loop   compress_device + decompress_device, stream after stream (what there was before the many-stream calls)
Both are timed with events on the context's stream, after a warm-up pass, REPS times; the table gives the median and the spread
(max - min) / median of the many-stream call.  A loop pass that would run longer than LOOP_S seconds is stopped after the streams
it got through and scaled to N (marked "~": every stream costs the same chain).
Diagnostic.   NS=1,8,64,512,2048 SIZES=65536,1048576,4194304 REPS=3 LOOP_S=5 python tools/knz_many_probe.py"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

NS = [int(v) for v in os.environ.get("NS", "1,8,64,512,2048").split(",")]
SIZES = [int(v) for v in os.environ.get("SIZES", "65536,1048576,4194304").split(",")]
REPS = int(os.environ.get("REPS", "3"))
LOOP_S = float(os.environ.get("LOOP_S", "5"))
bs = 4 << 20
chain, coder = "BWT+RANK+ZRLT", "ANS0"
dev = torch.device("cuda", 0)
ctx = kz.Context(0)
st = torch.cuda.ExternalStream(ctx.stream, device=dev)                     # the events go on the context's own stream
D = 64
mix = torch.from_numpy(np.stack([datagen.block(k, bs) for k in range(D)])).to(dev)   # the bench's mix


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    r = fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3, r


rows = []
for size in SIZES:
    for N in NS:
        free, _ = torch.cuda.mem_get_info(dev)
        if N * size * 8 > free:
            print(json.dumps({"skipped": {"streams": N, "bytes": size, "why": "memory"}}), flush=True)
            continue
        src = torch.empty(N * size, dtype=torch.uint8, device=dev)
        for s in range(N):                                                 # stream s: the head of block s of the mix
            src[s * size:(s + 1) * size] = mix[s % D, :size]
        cap1 = kz.compress_bound(size, bs)
        lens, soff, doff, caps = [size] * N, [s * size for s in range(N)], [s * cap1 for s in range(N)], [cap1] * N
        dst = torch.empty(N * cap1, dtype=torch.uint8, device=dev)
        back = torch.empty(N * size, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        many_e, many_d, loop_e, loop_d = [], [], [], []
        for it in range(REPS + 1):                                         # pass 0 warms up
            te, sizes = timed(lambda: kz.compress_many_device(ctx, chain, coder, bs, src.data_ptr(), soff, lens, dst.data_ptr(), doff, caps))
            back.zero_(); torch.cuda.synchronize()
            td, got = timed(lambda: kz.decompress_many_device(ctx, dst.data_ptr(), doff, sizes, back.data_ptr(), soff, lens))
            assert got == lens and torch.equal(back, src)
            if it:
                many_e.append(te); many_d.append(td)
        keep = dst.clone()
        scaled = False
        for it in range(min(REPS, 2) + 1):
            t_e = t_d = 0.0
            done = 0
            w0 = time.perf_counter()
            for s in range(N):
                t, sz = timed(lambda: kz.compress_device(ctx, chain, coder, bs, src.data_ptr() + soff[s], size, dst.data_ptr() + doff[s], cap1))
                t_e += t
                t, n = timed(lambda: kz.decompress_device(ctx, dst.data_ptr() + doff[s], sz, back.data_ptr() + soff[s], size))
                t_d += t
                assert sz == sizes[s] and n == size
                done += 1
                if time.perf_counter() - w0 > LOOP_S:
                    break
            if done < N:
                scaled = True
                t_e, t_d = t_e * N / done, t_d * N / done
            else:
                assert torch.equal(dst, keep) and torch.equal(back, src)   # the same streams, byte for byte
            if it:
                loop_e.append(t_e); loop_d.append(t_d)
        med = lambda v: float(np.median(v))
        tot = [a + b for a, b in zip(many_e, many_d)]
        r = {"streams": N, "bytes": size, "many_enc_s": med(many_e), "many_dec_s": med(many_d), "loop_enc_s": med(loop_e), "loop_dec_s": med(loop_d),
             "many_spread": (max(tot) - min(tot)) / med(tot), "loop_scaled": scaled,
             "ratio": (med(loop_e) + med(loop_d)) / (med(many_e) + med(many_d)), "stream_bytes": int(sum(sizes))}
        rows.append(r)
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
        del src, dst, back, keep
        torch.cuda.empty_cache()

print("\n| stream | N | many enc + dec (ms) | spread | loop enc + dec (ms) | loop / many |\n|---|---|---|---|---|---|")
for r in rows:
    print("| %d KiB | %d | %.2f + %.2f | %.0f %% | %s%.2f + %.2f | %.2f |" % (r["bytes"] >> 10, r["streams"], r["many_enc_s"] * 1e3, r["many_dec_s"] * 1e3,
          r["many_spread"] * 100, "~" if r["loop_scaled"] else "", r["loop_enc_s"] * 1e3, r["loop_dec_s"] * 1e3, r["ratio"]))
