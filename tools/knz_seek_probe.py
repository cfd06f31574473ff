"""Reading part of a device-resident .knz stream: what the three ways to get `count` blocks cost, and whether the cost depends on
where the blocks lie.  Two streams of the headline chain (BWT+RANK+ZRLT&ANS0) on the bench's mix: SMALL x 1 KiB blocks and BIG x
4 MiB blocks.  For count = 1, 16, 256, at the start of the stream and near its end (at blocks that hold the same bytes as those at
the start: the input is a tiling, and a block's decode time depends on what is in it):
   indexed   decode_indexed_device over the kept index (k_knz_check, no walk)
   range     decompress_range_device (walks the prefixes in front of the range)
and once per stream   whole = decompress_device, index = knz_index_device (the walk the indexed form pays once).
Each figure is the median of REPS calls after WARM warm-up calls (host clock around a synchronous call; min .. max behind it); every
read is compared with the source bytes once.  Diagnostic.
   python tools/knz_seek_probe.py [--out FILE]          SMALL=131072 BIG=512 REPS=7 WARM=2 in the environment"""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

chain, coder = "BWT+RANK+ZRLT", "ANS0"
REPS, WARM = int(os.environ.get("REPS", "7")), int(os.environ.get("WARM", "2"))
dev = torch.device("cuda", 0)
ctx = kz.Context(0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=REPS, warm=WARM):
    """-> (median, min, max) seconds of fn(), which ends synchronised"""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def ms(t):
    return "%9.3f ms (%.3f .. %.3f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)


def probe(nb, bs, distinct):
    host = np.stack([datagen.block(k, bs) for k in range(distinct)])
    d_in = torch.from_numpy(host).to(dev).repeat((nb + distinct - 1) // distinct, 1)[:nb].contiguous()
    n = nb * bs
    cap = kz.compress_bound(n, bs)
    d_knz = torch.empty(cap, dtype=torch.uint8, device=dev)
    size = kz.compress_device(ctx, chain, coder, bs, d_in.data_ptr(), n, d_knz.data_ptr(), cap)
    src = d_knz.data_ptr()
    say("stream: %d blocks of %d bytes, %s&%s, %d -> %d bytes" % (nb, bs, chain, coder, n, size))
    idx = kz.knz_index_device(ctx, src, size)["blocks"]
    assert len(idx) == nb
    t = timed(lambda: kz.knz_index_device(ctx, src, size), reps=3, warm=1)
    say("  index   knz_index_device, all %d blocks          %s   %.2f us per block" % (nb, ms(t), t[0] * 1e6 / nb))
    d_out = torch.empty(n, dtype=torch.uint8, device=dev)
    t = timed(lambda: kz.decompress_device(ctx, src, size, d_out.data_ptr(), n), reps=3, warm=1)
    assert torch.equal(d_out.view(nb, bs), d_in)
    say("  whole   decompress_device, all %d blocks         %s   %.2f GB/s" % (nb, ms(t), n / t[0] / 1e9))
    flat = d_in.view(-1)
    for count in (1, 16, 256):
        if count >= nb:
            continue
        res = {}
        last = (nb - count - 1) // distinct * distinct                     # the same blocks' bytes as at block 0 (the input is tiled)
        for where, first in (("start", 0), ("end", last)):
            offs, ws = [o for o, _ in idx[first:first + count]], [w for _, w in idx[first:first + count]]
            want = flat[first * bs:(first + count) * bs]
            d_out[:count * bs].zero_()
            r = kz.decode_indexed_device(ctx, src, size, offs, ws, d_out.data_ptr(), bs)
            assert all(x.status == 0 and x.length == bs for x in r[:count]) and torch.equal(d_out[:count * bs], want)
            res["indexed", where] = timed(lambda: kz.decode_indexed_device(ctx, src, size, offs, ws, d_out.data_ptr(), bs))
            d_out[:count * bs].zero_()
            assert kz.decompress_range_device(ctx, src, size, first, count, d_out.data_ptr(), count * bs) == count * bs and torch.equal(d_out[:count * bs], want)
            res["range", where] = timed(lambda: kz.decompress_range_device(ctx, src, size, first, count, d_out.data_ptr(), count * bs))
        for form in ("indexed", "range"):
            a, b = res[form, "start"], res[form, "end"]
            say("  %-7s %3d blocks   at block 0 %s   at block %d %s   difference %.3f us per block in front"
                % (form, count, ms(a), last, ms(b), (b[0] - a[0]) * 1e6 / last))
    say()


say("seekable .knz reads on device memory: median of %d calls after %d warm-up calls (min .. max)" % (REPS, WARM))
probe(int(os.environ.get("SMALL", "131072")), 1024, 256)
probe(int(os.environ.get("BIG", "512")), 4 << 20, 8)
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
