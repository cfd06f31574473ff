"""A store of N .knz streams in HBM (what kz_compress_many_device leaves behind): what it costs to overwrite 10^5 records of 128
bytes spread over all of them
   many     one kz_write_bytes_many_device call
   loop     N kz_write_bytes_device calls on the same ranges, stream by stream
   recode   kz_decompress_many_device of everything, the records scattered into the plain bytes, kz_compress_many_device of everything
on the read probe's shapes (tools/knz_store_probe.py): 64 streams of 16 blocks of 64 KiB; 8 streams of 32 blocks of 4 MiB with the
records confined to the first 1, 8 and all 32 blocks of every stream; and a single stream of each kind, where there is nothing to
merge.  The loop and the recode route use calls that were there before the many-stream write.  Wall time of the synchronous calls on
the host clock with a device sync around each, the routes alternating inside every repetition: median of REPS after WARM warm-up
rounds, min .. max behind it.  The new streams of `many` and `loop` are compared byte for byte once.  Behind every shape the kernel
times of one more `many` call and one more `loop` (the context's kernel timers), and the emit's traffic rate: bytes read plus bytes
written over the summed launch time of k_knz_splice_many resp. k_knz_splice.  Diagnostic; bench.py does not measure this.
   python tools/knz_store_write_probe.py [--out FILE]          REPS=5 WARM=1 RECORDS=100000 CHAIN=BWT+RANK+ZRLT CODER=ANS0 in the environment"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

chain, coder = os.environ.get("CHAIN", "BWT+RANK+ZRLT"), os.environ.get("CODER", "ANS0")
REPS, WARM, RECORDS = int(os.environ.get("REPS", "5")), int(os.environ.get("WARM", "1")), int(os.environ.get("RECORDS", "100000"))
REC = 128
# (block size, streams, blocks per stream, blocks of every stream that records may touch)
SHAPES = [(64 << 10, 64, 16, 16), (64 << 10, 1, 16, 16), (4 << 20, 8, 32, 1), (4 << 20, 8, 32, 8), (4 << 20, 8, 32, 32), (4 << 20, 1, 32, 32)]
if os.environ.get("SHAPES"):
    SHAPES = [tuple(int(x) for x in s.split(":")) for s in os.environ["SHAPES"].split(",")]
dev = torch.device("cuda", 0)
ctx = kz.Context(0)
lines, result = [], {"probe": "knz_store_write", "chain": chain + "&" + coder, "records": RECORDS, "record_bytes": REC, "reps": REPS, "warm": WARM, "cases": []}
i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def ms(t):
    return "%9.3f ms (%8.3f .. %8.3f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernels(fn):
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        fn()
        return ctx.kernel_times()
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()


def top(times, n=6):
    return "  ".join("%s %.2f ms x%d" % (k, v["ms"], v["launches"]) for k, v in sorted(times.items(), key=lambda kv: -kv[1]["ms"])[:n])


say("overwriting %d records of %d bytes in a store of N streams in HBM, %s&%s" % (RECORDS, REC, chain, coder))
say("wall time of the synchronous calls, the routes alternating; median of %d after %d warm-up rounds (min .. max)" % (REPS, WARM))
for BS, N, NB, TOUCH in SHAPES:
    host = np.stack([datagen.block(k, BS) for k in range(8)])
    n1 = NB * BS
    d_in = torch.from_numpy(host).to(dev)[[(s + k) % 8 for s in range(N) for k in range(NB)]].contiguous().view(-1)
    caps = [kz.compress_bound(n1, BS)] * N
    slot = [s * caps[0] + 1 for s in range(N)]                               # odd addresses
    d_knz = torch.empty(N * caps[0] + 16, dtype=torch.uint8, device=dev)
    sizes = kz.compress_many_device(ctx, chain, coder, BS, d_in.data_ptr(), [s * n1 for s in range(N)], [n1] * N, d_knz.data_ptr(), slot, caps)
    assert all(z > 0 for z in sizes), sizes
    index = kz.knz_index_many_device(ctx, d_knz.data_ptr(), slot, sizes)
    so, sl = i64(slot), i64(sizes)
    first = i64([s * NB for s in range(N + 1)])
    e_off, e_w = i64([b[0] for ix in index for b in ix["blocks"]]), i64([b[1] for ix in index for b in ix["blocks"]])
    rng = np.random.default_rng(2026)
    rs = rng.integers(0, N, RECORDS).astype(np.int32)
    ro = i64(rng.integers(0, TOUCH * BS - REC, RECORDS))
    rl = np.full(RECORDS, REC, dtype=np.int64)
    total = RECORDS * REC
    d_new = torch.randint(0, 256, (total + 16,), dtype=torch.uint8, device=dev)
    _, wcaps = kz.write_bytes_many_bound(index, [BS] * N)
    wcaps = [c + (c & 1) for c in wcaps]
    wslot = i64([s * wcaps[0] + 1 for s in range(N)])
    wcap = i64(wcaps)
    d_out = torch.empty(N * wcaps[0] + 16, dtype=torch.uint8, device=dev)
    dl = np.zeros(N, dtype=np.int64)

    def many():
        rc = ctx.lib.kz_write_bytes_many_device(ctx.h, d_knz.data_ptr(), so.ctypes.data, sl.ctypes.data, N, first.ctypes.data, e_off.ctypes.data, e_w.ctypes.data, None, None,
                                                rs.ctypes.data, ro.ctypes.data, rl.ctypes.data, RECORDS, d_new.data_ptr() + 1, total, d_out.data_ptr(), wslot.ctypes.data,
                                                wcap.ctypes.data, dl.ctypes.data, None, None)
        assert rc == 0 and all(x > 0 for x in dl), (rc, dl.tolist(), ctx.error())

    # ---- loop: per stream its records in call order, their new bytes packed for that stream alone (made once) ----
    order = np.argsort(rs, kind="stable")
    bounds = np.searchsorted(rs[order], np.arange(N + 1))
    d_loop_new = d_new[1:1 + total].view(RECORDS, REC)[torch.from_numpy(order).to(dev)].contiguous().view(-1)
    d_loop = torch.empty(N * wcaps[0] + 16, dtype=torch.uint8, device=dev)
    per = [(i64(ro[order[bounds[s]:bounds[s + 1]]]), i64(rl[order[bounds[s]:bounds[s + 1]]]), int(bounds[s]) * REC, int(bounds[s + 1] - bounds[s])) for s in range(N)]
    ll = np.zeros(N, dtype=np.int64)

    def loop():
        for s in range(N):
            o, l, at, cnt = per[s]
            ll[s] = ctx.lib.kz_write_bytes_device(ctx.h, d_knz.data_ptr() + slot[s], sizes[s], e_off[s * NB:].ctypes.data, e_w[s * NB:].ctypes.data, None, NB, o.ctypes.data,
                                                  l.ctypes.data, cnt, d_loop_new.data_ptr() + at, cnt * REC, d_loop.data_ptr() + int(wslot[s]), wcaps[s], None, None)
            assert ll[s] > 0, (s, ll[s], ctx.error())

    # ---- recode: everything decoded, the records scattered into the plain bytes, everything encoded ----
    d_plain = torch.empty(N * n1 + 16, dtype=torch.uint8, device=dev)
    d_re = torch.empty(N * caps[0] + 16, dtype=torch.uint8, device=dev)
    where = (torch.from_numpy(rs.astype(np.int64) * n1 + ro).to(dev)[:, None] + torch.arange(REC, device=dev)[None, :]).view(-1)

    def recode():
        got = kz.decompress_many_device(ctx, d_knz.data_ptr(), slot, sizes, d_plain.data_ptr(), [s * n1 for s in range(N)], [n1] * N)
        assert all(g == n1 for g in got)
        d_plain[where] = d_new[1:1 + total]                                   # (records that overlap: any order; the time is what counts here)
        torch.cuda.synchronize()
        out = kz.compress_many_device(ctx, chain, coder, BS, d_plain.data_ptr(), [s * n1 for s in range(N)], [n1] * N, d_re.data_ptr(), slot, caps)
        assert all(z > 0 for z in out)

    # ---- once for the bytes ----
    many(); loop()
    assert dl.tolist() == ll.tolist(), "the loop writes streams of other sizes"
    for s in range(N):
        a, b = int(wslot[s]), int(wslot[s]) + int(dl[s])
        assert torch.equal(d_out[a:b], d_loop[a:b]), ("the loop writes other bytes", s)
    fns = {"many": many, "loop": loop, "recode": recode}
    t = {k: [] for k in fns}
    for r in range(WARM + REPS):
        for k in t:
            x = timed(fns[k])
            if r >= WARM:
                t[k].append(x)
    mm = {k: med(v) for k, v in t.items()}
    km, kl = kernels(many), kernels(loop)
    moved = 2 * int(dl.sum())                                                 # the emit reads every bit of the new streams once and writes it once
    sm, sp = km.get("k_knz_splice_many", {"ms": 0, "launches": 0}), kl.get("k_knz_splice", {"ms": 0, "launches": 0})
    say("block size %8d  N = %3d x %2d blocks, records in the first %2d of each  (%d -> %d bytes)" % (BS, N, NB, TOUCH, N * n1, sum(sizes)))
    say("  many   %s" % ms(mm["many"]))
    say("  loop   %s   loop / many = %.2f" % (ms(mm["loop"]), mm["loop"][0] / mm["many"][0]))
    say("  recode %s   recode / many = %.2f" % (ms(mm["recode"]), mm["recode"][0] / mm["many"][0]))
    say("  many's kernels: %s" % top(km))
    say("  loop's kernels: %s" % top(kl))
    say("  emit: k_knz_splice_many %.3f ms in %d launches = %.2f TB/s;  k_knz_splice %.3f ms in %d launches = %.2f TB/s  (%d bytes read plus written)"
        % (sm["ms"], sm["launches"], moved / max(sm["ms"], 1e-9) / 1e9, sp["ms"], sp["launches"], moved / max(sp["ms"], 1e-9) / 1e9, moved))
    result["cases"].append(dict({"block_size": BS, "streams": N, "blocks": NB, "touch": TOUCH, "emit_bytes": moved, "splice_many_ms": round(sm["ms"], 4), "splice_ms": round(sp["ms"], 4)},
                                **{k + "_ms": [round(x * 1e3, 3) for x in v] for k, v in mm.items()}))
    del d_in, d_knz, d_out, d_loop, d_plain, d_re, d_new, d_loop_new, where
    torch.cuda.empty_cache()
say()
say(json.dumps(result))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
