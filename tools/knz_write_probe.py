"""Byte-addressed writes of a device-resident .knz stream (kz_write_bytes_device): what five shapes of update cost on a stream of
4 MiB blocks in HBM, and where the time goes.
   records-128/1    10^5 random records of 128 bytes, all inside one block
   records-128/8    the same inside 8 neighbouring blocks
   records-128/all  the same over all blocks
   records-64k      10^3 random records of 64 KiB over all blocks
   whole-blocks     every block as one range of its own
For each: the call's wall time (host clock around the synchronous call: median of REPS after WARM warm-up calls, min .. max behind
it); from the kernel timers of REPS further calls (mean per call), the patch kernel k_knz_write, the bit copy k_knz_splice and
everything else (check, unpack, decode, encode); the same call with the segments patched by k_knz_gather (KZ_WRITE_GATHER=1: the
ragged copy, one workgroup column per segment), the two alternating.  Beside them what a caller did before this call existed, in the
same process: kz_decompress_device of the whole stream, a patch of the decoded data, kz_compress_device of all of it.  Every result
is decoded once and compared with the ranges applied in order on the host.  Diagnostic; bench.py does not measure this.
   python tools/knz_write_probe.py [--out FILE]         BLOCKS=32 REPS=7 WARM=2 CHAIN=BWT+RANK+ZRLT CODER=ANS0 in the environment"""
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
lines, result = [], {"probe": "knz_write", "chain": chain + "&" + coder, "blocks": NB, "block_size": BS, "reps": REPS, "warm": WARM, "cases": {}}


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


def gather(on):
    if on:
        os.environ["KZ_WRITE_GATHER"] = "1"
    else:
        os.environ.pop("KZ_WRITE_GATHER", None)
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
a_off, a_w = np.ascontiguousarray([b[0] for b in index], dtype=np.int64), np.ascontiguousarray([b[1] for b in index], dtype=np.int64)
wcap = kz.write_bytes_bound(a_w, BS)
d_new = torch.empty(wcap + 16, dtype=torch.uint8, device=dev)
d_back = torch.empty(n, dtype=torch.uint8, device=dev)
orig = d_in.view(-1).cpu().numpy()
say("byte-addressed writes on device memory: %d blocks of %d bytes, %s&%s, %d -> %d bytes; median of %d calls after %d warm-up calls (min .. max)"
    % (NB, BS, chain, coder, n, size, REPS, WARM))
rng = np.random.default_rng(2026)
few = min(8, NB)
cases = [("records-128/1", rng.integers(0, BS - 128, 100000) + (NB // 2) * BS, 128),
         ("records-128/%d" % few, rng.integers(0, few * BS - 128, 100000) + ((NB - few) // 2) * BS, 128),
         ("records-128/all", rng.integers(0, n - 128, 100000), 128),
         ("records-64k", rng.integers(0, n - 65536, 1000), 65536),
         ("whole-blocks", np.arange(NB, dtype=np.int64) * BS, BS)]
for name, offs, length in cases:
    offs = [int(o) for o in offs]
    total = length * len(offs)
    payload = np.random.default_rng(len(offs) + length).integers(0, 256, total, dtype=np.uint8)
    d_data = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    d_data[3:3 + total] = torch.from_numpy(payload).to(dev)               # the new bytes at an odd address
    a_ro, a_rl = np.ascontiguousarray(offs, dtype=np.int64), np.full(len(offs), length, dtype=np.int64)
    a_no, a_nw = np.zeros(NB, dtype=np.int64), np.zeros(NB, dtype=np.int64)
    touched = len({o // BS for o in offs} | {(o + length - 1) // BS for o in offs})

    def call():                                                          # the C call alone, its arrays made once; dst at an odd address
        rc = ctx.lib.kz_write_bytes_device(ctx.h, d_knz.data_ptr(), size, a_off.ctypes.data, a_w.ctypes.data, None, NB, a_ro.ctypes.data, a_rl.ctypes.data, len(offs),
                                           d_data.data_ptr() + 3, total, d_new.data_ptr() + 1, wcap, a_no.ctypes.data, a_nw.ctypes.data)
        assert rc > 0, (rc, ctx.error())
        return rc

    want = orig.copy()                                                   # the ranges applied in order: the later one wins
    for i, o in enumerate(offs):
        want[o:o + length] = payload[i * length:(i + 1) * length]
    for on in (False, True):                                             # once for the bytes, with either patch kernel
        gather(on)
        d_new.zero_()
        rc = call()
        assert kz.decompress_device(ctx, d_new.data_ptr() + 1, rc, d_back.data_ptr(), n) == n
        assert np.array_equal(d_back.cpu().numpy(), want), (name, on)
    gather(False)
    for _ in range(WARM):
        call()
    wall = {False: [], True: []}
    for _ in range(REPS):                                                # the two kernels alternate
        for on in (False, True):
            gather(on)
            wall[on].append(timed(call))
    gather(False)
    k_write = kernels(call)
    gather(True)
    k_gath = kernels(call)
    gather(False)
    t_write, t_gath, t_splice = k_write.get("k_knz_write", 0.0), k_gath.get("k_knz_gather", 0.0), k_write.get("k_knz_splice", 0.0)
    assert "k_knz_gather" not in k_write and "k_knz_write" not in k_gath
    rest = sum(v for k, v in k_write.items() if k not in ("k_knz_write", "k_knz_splice"))
    w, wg = med(wall[False]), med(wall[True])
    say("%-16s %6d ranges of %8d bytes = %10d bytes, %d blocks touched" % (name, len(offs), length, total, touched))
    say("  call                          %s" % ms(w))
    say("  its kernels: k_knz_write %.3f ms (%.1f GB/s read + written) + k_knz_splice %.3f ms + all others (check, unpack, decode, encode) %.3f ms"
        % (t_write, 2 * total / max(t_write, 1e-9) / 1e6, t_splice, rest))
    say("  call with k_knz_gather        %s   k_knz_gather %.3f ms = %.2f x k_knz_write" % (ms(wg), t_gath, t_gath / max(t_write, 1e-9)))
    result["cases"][name] = {"ranges": len(offs), "bytes": total, "touched_blocks": touched, "call_ms": w[0] * 1e3, "call_gather_ms": wg[0] * 1e3, "k_knz_write_ms": t_write,
                             "k_knz_gather_ms": t_gath, "k_knz_splice_ms": t_splice, "other_kernels_ms": rest}
    if name == "records-128/all":                                        # what a caller did before: decode all, patch, encode all
        d_idx = (torch.from_numpy(a_ro).to(dev)[:, None] + torch.arange(length, device=dev)[None, :]).reshape(-1)
        d_val = d_data[3:3 + total]

        def before():
            assert kz.decompress_device(ctx, d_knz.data_ptr(), size, d_back.data_ptr(), n) == n
            d_back[d_idx] = d_val                                        # (which of two overlapping records wins is left open here: only the time counts)
            torch.cuda.synchronize()
            assert kz.compress_device(ctx, chain, coder, BS, d_back.data_ptr(), n, d_new.data_ptr(), wcap) > 0

        for _ in range(WARM):
            before()
        b = med([timed(before) for _ in range(REPS)])
        say("  before this call: kz_decompress_device, a patch, kz_compress_device of the whole stream")
        say("                                %s" % ms(b))
        result["decode_patch_encode_all_ms"] = b[0] * 1e3
        del d_idx
    del d_data
say()
say(json.dumps(result))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
