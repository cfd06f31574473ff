"""kz_knz_scan_device (every bit position tested, no walk) next to kz_knz_index_device (the serial walk of the length prefixes) on
two streams in HBM, in one process:
   big      1 GiB in 4 MiB blocks: 256 prefixes to walk
   small    256 MiB in 1 KiB blocks: 262 144 prefixes to walk
NONE&NONE blocks of random bytes: the stream is as long as the data, and incompressible payload is what gives the scan the most
chance hits to link.  Both calls are synchronous (they end in a wait for the context's stream) and are timed with the host clock
around the raw library call, into arrays allocated beforehand; after a warm-up call REPS times, the median and the spread
(max - min) / median are printed, the kernels' own times of one scan call besides, and what the scan found.
Diagnostic.   REPS=7 python tools/knz_scan_probe.py [big|small ...]"""
import ctypes, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz

REPS = max(5, int(os.environ.get("REPS", "7")))
SHAPES = {"big": (1 << 30, 4 << 20), "small": (256 << 20, 1024)}
dev = torch.device("cuda", 0)
ctx = kz.Context(0)


def stats(v):
    m = float(np.median(v))
    return {"ms": round(m, 4), "spread": round((max(v) - min(v)) / m, 3)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def probe(name):
    n, bs = SHAPES[name]
    data = torch.randint(0, 256, (n + 1,), dtype=torch.uint8, device=dev)[1:]   # an odd address
    cap = kz.compress_bound(n, bs)
    knz = torch.empty(cap + 3, dtype=torch.uint8, device=dev)[3:]
    torch.cuda.synchronize()
    size = kz.compress_device(ctx, "NONE", "NONE", bs, data.data_ptr(), n, knz.data_ptr(), cap)
    del data
    nb = n // bs
    hdr = [ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)]
    hp = [ctypes.addressof(h) for h in hdr]
    off, bits = np.zeros(nb + 16, dtype=np.int64), np.zeros(nb + 16, dtype=np.int64)
    walk = lambda: ctx.lib.kz_knz_index_device(ctx.h, knz.data_ptr(), size, *hp, off.ctypes.data, bits.ctypes.data, len(off))
    cols = np.zeros((4, nb + 4096), dtype=np.int64)
    head = ctypes.c_int64(0)
    scan = lambda: ctx.lib.kz_knz_scan_device(ctx.h, knz.data_ptr(), size, 4, *hp, cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data,
                                              cols[3].ctypes.data, cols.shape[1], ctypes.addressof(head))
    t_walk, t_scan = [], []
    for it in range(REPS + 1):                                     # alternating, the first pair is the warm-up
        tw, rw = timed(walk)
        ts, rs = timed(scan)
        assert rw == nb, rw
        assert nb <= rs <= cols.shape[1], rs
        if it:
            t_walk.append(tw); t_scan.append(ts)
    # the scan's chain from head is the walk's list
    k, i, same = int(rs), int(head.value), 0
    while i >= 0:
        assert cols[1][i] == off[same] and cols[2][i] == bits[same], (name, same)
        same, i = same + 1, int(cols[3][i])
    assert same == nb and i == kz.SCAN_END, (same, i)
    ctx.set_kernel_timing(True); ctx.reset_kernel_timing()
    scan()
    kern = {k_: round(v["ms"], 4) for k_, v in ctx.kernel_times().items()}
    ctx.set_kernel_timing(False); ctx.reset_kernel_timing()
    r = {"stream_bytes": int(size), "blocks": nb, "walk": stats(t_walk), "scan": stats(t_scan), "scan_kernels_ms": kern,
         "kept_entries": k, "kept_off_the_chain": k - nb}
    r["scan_over_walk"] = round(r["scan"]["ms"] / r["walk"]["ms"], 4)
    r["scan_GBps"] = round(size / r["scan"]["ms"] / 1e6, 1)
    return r


out = {"reps": REPS}
for name in (sys.argv[1:] or ["big", "small"]):
    out[name] = probe(name)
    torch.cuda.empty_cache()
print(json.dumps(out))
