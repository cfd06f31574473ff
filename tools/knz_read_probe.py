"""Byte-addressed reads of a device-resident .knz stream (kz_read_bytes_device): what three shapes of request cost on a stream of
4 MiB blocks in HBM, and where the time goes.
   records-128   10^5 random records of 128 bytes
   records-64k   10^3 random records of 64 KiB
   whole         the whole stream as one range
For each: the call's wall time (host clock around the synchronous call: median of REPS after WARM warm-up calls, min .. max behind
it); from the kernel timers of REPS further calls (mean per call), the copy kernel k_knz_read and everything else (check, unpack, decode); the same
call with the segments copied by k_knz_scatter (KZ_READ_SCATTER=1: the ragged copy, one workgroup column per segment), the two
alternating; and a plain device-to-device copy of as many bytes as the request delivers.  Every read is compared with the source
bytes once.  A record costs the decode of its whole block, whatever its length: with 4 MiB blocks the decode is nearly all of the
call, which is why the copy kernels are compared by their own timers.  Diagnostic; bench.py does not measure this.
   python tools/knz_read_probe.py [--out FILE]          BLOCKS=32 REPS=7 WARM=2 CHAIN=BWT+RANK+ZRLT CODER=ANS0 in the environment"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

chain, coder = os.environ.get("CHAIN", "BWT+RANK+ZRLT"), os.environ.get("CODER", "ANS0")
REPS, WARM, NB = int(os.environ.get("REPS", "7")), int(os.environ.get("WARM", "2")), int(os.environ.get("BLOCKS", "32"))
BS = 4 << 20
dev = torch.device("cuda", 0)
ctx = kz.Context(0)
lines, result = [], {"probe": "knz_read", "chain": chain + "&" + coder, "blocks": NB, "block_size": BS, "reps": REPS, "warm": WARM, "cases": {}}


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def ms(t):
    return "%9.3f ms (%.3f .. %.3f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def scatter(on):
    if on:
        os.environ["KZ_READ_SCATTER"] = "1"
    else:
        os.environ.pop("KZ_READ_SCATTER", None)
    ctx.reload_switches()


def kernels(fn):
    """the kernel timers over REPS calls -> {name: ms per call}"""
    ctx.set_kernel_timing(True)
    ctx.reset_kernel_timing()
    try:
        for _ in range(REPS):
            fn()
        return {k: v["ms"] / REPS for k, v in ctx.kernel_times().items()}
    finally:
        ctx.set_kernel_timing(False)
        ctx.reset_kernel_timing()


host = np.stack([datagen.block(k, BS) for k in range(8)])
d_in = torch.from_numpy(host).to(dev).repeat((NB + 7) // 8, 1)[:NB].contiguous()
n = NB * BS
cap = kz.compress_bound(n, BS)
d_knz = torch.empty(cap, dtype=torch.uint8, device=dev)
size = kz.compress_device(ctx, chain, coder, BS, d_in.data_ptr(), n, d_knz.data_ptr(), cap)
index = kz.knz_index_device(ctx, d_knz.data_ptr(), size)["blocks"]
flat = d_in.view(-1)
say("byte-addressed reads on device memory: %d blocks of %d bytes, %s&%s, %d -> %d bytes; median of %d calls after %d warm-up calls (min .. max)"
    % (NB, BS, chain, coder, n, size, REPS, WARM))
rng = np.random.default_rng(2025)
cases = [("records-128", rng.integers(0, n - 128, 100000), 128), ("records-64k", rng.integers(0, n - 65536, 1000), 65536), ("whole", np.zeros(1, dtype=np.int64), n)]
for name, offs, length in cases:
    offs = [int(o) for o in offs]
    sizes = [length] * len(offs)
    total = length * len(offs)
    d_out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    d_copy = torch.empty(total, dtype=torch.uint8, device=dev)
    d_from = torch.full((total,), 7, dtype=torch.uint8, device=dev)
    a_off, a_w = np.ascontiguousarray([b[0] for b in index], dtype=np.int64), np.ascontiguousarray([b[1] for b in index], dtype=np.int64)
    a_ro, a_rl, a_got = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(sizes, dtype=np.int64), np.zeros(len(offs), dtype=np.int64)

    def call():                                                          # the C call alone, its arrays made once; dst at an odd address
        rc = ctx.lib.kz_read_bytes_device(ctx.h, d_knz.data_ptr(), size, a_off.ctypes.data, a_w.ctypes.data, None, len(index), a_ro.ctypes.data, a_rl.ctypes.data, len(offs),
                                          d_out.data_ptr() + 1, total, a_got.ctypes.data)
        assert rc == total, (rc, ctx.error())
        return a_got.tolist()

    # once for the bytes, with either copy kernel
    for on in (False, True):
        scatter(on)
        d_out.zero_()
        assert call() == sizes
        got = d_out[1:1 + total].view(len(offs), length)
        for i in range(0, len(offs), max(1, len(offs) // 512)):
            assert torch.equal(got[i], flat[offs[i]:offs[i] + length]), (name, on, i)
    scatter(False)
    for _ in range(WARM):
        call()
        d_copy.copy_(d_from)
    wall = {False: [], True: []}
    copy = []
    for _ in range(REPS):                                                # the two kernels alternate; the plain copy runs between them
        for on in (False, True):
            scatter(on)
            wall[on].append(timed(call))
        copy.append(timed(lambda: d_copy.copy_(d_from)))
    scatter(False)
    k_read = kernels(call)
    scatter(True)
    k_scat = kernels(call)
    scatter(False)
    t_read, t_scat = k_read.get("k_knz_read", 0.0), k_scat.get("k_knz_scatter", 0.0)
    assert "k_knz_scatter" not in k_read and "k_knz_read" not in k_scat
    rest = sum(v for k, v in k_read.items() if k != "k_knz_read")
    w, ws, c = med(wall[False]), med(wall[True]), med(copy)
    say("%-12s %6d ranges of %8d bytes = %10d bytes" % (name, len(offs), length, total))
    say("  call                          %s" % ms(w))
    say("  its kernels: k_knz_read %.3f ms (%.1f GB/s read + written) + all others (check, unpack, decode) %.3f ms" % (t_read, 2 * total / max(t_read, 1e-9) / 1e6, rest))
    say("  call with k_knz_scatter       %s   k_knz_scatter %.3f ms = %.2f x k_knz_read" % (ms(ws), t_scat, t_scat / max(t_read, 1e-9)))
    say("  plain device copy, same bytes %s   k_knz_read / copy = %.2f" % (ms(c), t_read / 1e3 / max(c[0], 1e-12)))
    result["cases"][name] = {"ranges": len(offs), "bytes": total, "call_ms": w[0] * 1e3, "call_scatter_ms": ws[0] * 1e3, "k_knz_read_ms": t_read,
                             "k_knz_scatter_ms": t_scat, "other_kernels_ms": rest, "device_copy_ms": c[0] * 1e3}
    del d_out, d_copy, d_from
say()
say(json.dumps(result))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
