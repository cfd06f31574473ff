"""A store of N .knz streams in HBM (what kz_compress_many_device leaves behind), 16 blocks a stream: what the index of all of them
and 10^5 records of 128 bytes spread over all of them cost
   many     one kz_knz_index_many_device call, one kz_read_bytes_many_device call
   loop     N kz_knz_index_device calls, N kz_read_bytes_device calls on the same ranges, stream by stream
   splice   kz_knz_splice_device of the N streams into one and ONE kz_read_bytes_device call on it with the table of block starts
            (the splice is paid once per store, the read per request: both are shown)
for N in 1, 8, 64, 512 at 64 KiB and at 4 MiB blocks.  A shape whose decoded rows (N x 16 x block size) do not fit one chunk's
staging rows is skipped: there the many-stream call decodes in several chunks and the comparison is another one.  The loop and the
splice route use single-stream calls only, so they cost what they cost without the many-stream calls.  Wall time of the
synchronous calls on the host clock, the three routes alternating inside every repetition: median of REPS after WARM warm-up
rounds, min .. max behind it.  Every route's bytes are compared with the source once.  Diagnostic; bench.py does not measure this.
   python tools/knz_store_probe.py [--out FILE]          REPS=7 WARM=2 RECORDS=100000 CHAIN=BWT+RANK+ZRLT CODER=ANS0 in the environment"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

chain, coder = os.environ.get("CHAIN", "BWT+RANK+ZRLT"), os.environ.get("CODER", "ANS0")
REPS, WARM, RECORDS = int(os.environ.get("REPS", "7")), int(os.environ.get("WARM", "2")), int(os.environ.get("RECORDS", "100000"))
STREAMS = [int(x) for x in os.environ.get("STREAMS", "1,8,64,512").split(",")]
SIZES = [int(x) for x in os.environ.get("BLOCK_SIZES", "%d,%d" % (64 << 10, 4 << 20)).split(",")]
NB, REC = 16, 128
dev = torch.device("cuda", 0)
ctx = kz.Context(0)
lines, result = [], {"probe": "knz_store", "chain": chain + "&" + coder, "blocks_per_stream": NB, "records": RECORDS, "record_bytes": REC, "reps": REPS, "warm": WARM, "cases": []}
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


def chunk_blocks(bs):
    """the blocks of one chunk of the indexed reads (kz_knz_stream.h: knz_chunk_blocks, without KZ_STREAM_CHUNK)"""
    return max(8, min(2048, (1 << 30) // bs))


say("a store of N streams of %d blocks in HBM, %s&%s; index of all streams, and %d records of %d bytes spread over all of them" % (NB, chain, coder, RECORDS, REC))
say("wall time of the synchronous calls, the routes alternating; median of %d after %d warm-up rounds (min .. max)" % (REPS, WARM))
for BS in SIZES:
    host = np.stack([datagen.block(k, BS) for k in range(8)])
    for N in STREAMS:
        if N * NB > chunk_blocks(BS):
            say("block size %8d  N = %3d: skipped, %d blocks of decoded rows do not fit one chunk's staging (%d blocks)" % (BS, N, N * NB, chunk_blocks(BS)))
            result["cases"].append({"block_size": BS, "streams": N, "skipped": True})
            continue
        n1 = NB * BS                                                         # bytes of a stream's data: whole blocks
        d_in = torch.from_numpy(host).to(dev)[[(s + k) % 8 for s in range(N) for k in range(NB)]].contiguous().view(-1)
        caps = [kz.compress_bound(n1, BS)] * N
        slot = [s * caps[0] + 1 for s in range(N)]                           # odd addresses
        d_knz = torch.empty(N * caps[0] + 16, dtype=torch.uint8, device=dev)
        sizes = kz.compress_many_device(ctx, chain, coder, BS, d_in.data_ptr(), [s * n1 for s in range(N)], [n1] * N, d_knz.data_ptr(), slot, caps)
        assert all(z > 0 for z in sizes), sizes
        so, sl = i64(slot), i64(sizes)
        rng = np.random.default_rng(2026)
        rs = rng.integers(0, N, RECORDS).astype(np.int32)
        ro = i64(rng.integers(0, n1 - REC, RECORDS))
        rl = np.full(RECORDS, REC, dtype=np.int64)
        total = RECORDS * REC
        d_out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        # ---- many ----
        status, first, got, sstat = np.zeros(N, dtype=np.int32), np.zeros(N + 1, dtype=np.int64), np.zeros(RECORDS, dtype=np.int64), np.zeros(N, dtype=np.int32)
        e_off, e_w = np.zeros(N * NB, dtype=np.int64), np.zeros(N * NB, dtype=np.int64)

        def index_many():
            rc = ctx.lib.kz_knz_index_many_device(ctx.h, d_knz.data_ptr(), so.ctypes.data, sl.ctypes.data, N, None, None, None, None, None, status.ctypes.data, first.ctypes.data,
                                                  e_off.ctypes.data, e_w.ctypes.data, N * NB)
            assert rc == N * NB, (rc, ctx.error())

        def read_many():
            rc = ctx.lib.kz_read_bytes_many_device(ctx.h, d_knz.data_ptr(), so.ctypes.data, sl.ctypes.data, N, first.ctypes.data, e_off.ctypes.data, e_w.ctypes.data, None, None,
                                                   rs.ctypes.data, ro.ctypes.data, rl.ctypes.data, RECORDS, d_out.data_ptr() + 1, total, got.ctypes.data, sstat.ctypes.data)
            assert rc == total, (rc, ctx.error())

        # ---- loop: per stream its own arrays, made once; the stream's records in call order, its slots back to back in a buffer of its own ----
        per = []
        order = np.argsort(rs, kind="stable")
        bounds = np.searchsorted(rs[order], np.arange(N + 1))
        d_loop = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        l_off, l_w = [np.zeros(NB, dtype=np.int64) for _ in range(N)], [np.zeros(NB, dtype=np.int64) for _ in range(N)]
        for s in range(N):
            mine = order[bounds[s]:bounds[s + 1]]
            per.append((i64(ro[mine]), i64(rl[mine]), np.zeros(max(len(mine), 1), dtype=np.int64), int(bounds[s]) * REC, len(mine)))

        def index_loop():
            for s in range(N):
                rc = ctx.lib.kz_knz_index_device(ctx.h, d_knz.data_ptr() + slot[s], sizes[s], None, None, None, None, None, l_off[s].ctypes.data, l_w[s].ctypes.data, NB)
                assert rc == NB, (rc, ctx.error())

        def read_loop():
            for s in range(N):
                o, l, g, at, cnt = per[s]
                rc = ctx.lib.kz_read_bytes_device(ctx.h, d_knz.data_ptr() + slot[s], sizes[s], l_off[s].ctypes.data, l_w[s].ctypes.data, None, NB, o.ctypes.data, l.ctypes.data, cnt,
                                                  d_loop.data_ptr() + 1 + at, cnt * REC, g.ctypes.data)
                assert rc == cnt * REC, (rc, ctx.error())

        # ---- splice: one joined stream and its table; record (s, o) lies at s * n1 + o of the joined data ----
        index_many()
        index_loop()
        assert [l_off[s].tolist() for s in range(N)] == [e_off[s * NB:(s + 1) * NB].tolist() for s in range(N)]
        pieces = [(s, int(e_off[s * NB + k]), int(e_w[s * NB + k])) for s in range(N) for k in range(NB)]
        jcap = kz.knz_splice_bound([p[2] for p in pieces])
        d_join = torch.empty(jcap + 16, dtype=torch.uint8, device=dev)
        ps, po, pw = np.ascontiguousarray([p[0] for p in pieces], dtype=np.int32), i64([p[1] for p in pieces]), i64([p[2] for p in pieces])
        jsize = [0]

        def splice():
            jsize[0] = ctx.lib.kz_knz_splice_device(ctx.h, d_knz.data_ptr(), so.ctypes.data, sl.ctypes.data, N, ps.ctypes.data, po.ctypes.data, pw.ctypes.data, len(pieces), N * n1,
                                                    d_join.data_ptr() + 1, jcap)
            assert jsize[0] > 0, (jsize[0], ctx.error())

        splice()
        j_index = kz.knz_index_device(ctx, d_join.data_ptr() + 1, jsize[0])["blocks"]
        j_off, j_w, j_tab = i64([b[0] for b in j_index]), i64([b[1] for b in j_index]), i64(kz.block_byte_offsets([n1] * N, BS))
        j_ro, j_got = i64(rs.astype(np.int64) * n1 + ro), np.zeros(RECORDS, dtype=np.int64)
        d_sp = torch.empty(total + 16, dtype=torch.uint8, device=dev)

        def read_spliced():
            rc = ctx.lib.kz_read_bytes_device(ctx.h, d_join.data_ptr() + 1, jsize[0], j_off.ctypes.data, j_w.ctypes.data, j_tab.ctypes.data, len(j_index), j_ro.ctypes.data, rl.ctypes.data,
                                              RECORDS, d_sp.data_ptr() + 1, total, j_got.ctypes.data)
            assert rc == total, (rc, ctx.error())

        # ---- once for the bytes ----
        read_many(); read_loop(); read_spliced()
        assert got.tolist() == [REC] * RECORDS and j_got.tolist() == [REC] * RECORDS
        m = d_out[1:1 + total].view(RECORDS, REC)
        assert torch.equal(m, d_sp[1:1 + total].view(RECORDS, REC)), "the spliced route reads other bytes"
        assert torch.equal(m[torch.from_numpy(order).to(dev)], d_loop[1:1 + total].view(RECORDS, REC)), "the loop reads other bytes"
        for i in range(0, RECORDS, max(1, RECORDS // 512)):
            a = int(rs[i]) * n1 + int(ro[i])
            assert torch.equal(m[i], d_in[a:a + REC]), (BS, N, i)
        # ---- the timed rounds: the routes alternate ----
        t = {k: [] for k in ("index_many", "index_loop", "read_many", "read_loop", "splice", "read_spliced")}
        fns = {"index_many": index_many, "index_loop": index_loop, "read_many": read_many, "read_loop": read_loop, "splice": splice, "read_spliced": read_spliced}
        for r in range(WARM + REPS):
            for k in t:
                x = timed(fns[k])
                if r >= WARM:
                    t[k].append(x)
        mm = {k: med(v) for k, v in t.items()}
        say("block size %8d  N = %3d  (%d blocks, %d -> %d bytes)" % (BS, N, N * NB, N * n1, sum(sizes)))
        say("  index   many %s   loop %s   loop / many = %.2f" % (ms(mm["index_many"]), ms(mm["index_loop"]), mm["index_loop"][0] / mm["index_many"][0]))
        say("  read    many %s   loop %s   loop / many = %.2f" % (ms(mm["read_many"]), ms(mm["read_loop"]), mm["read_loop"][0] / mm["read_many"][0]))
        say("  splice once  %s   then one read %s   read / many = %.2f" % (ms(mm["splice"]), ms(mm["read_spliced"]), mm["read_spliced"][0] / mm["read_many"][0]))
        result["cases"].append(dict({"block_size": BS, "streams": N, "skipped": False}, **{k + "_ms": [round(x * 1e3, 3) for x in v] for k, v in mm.items()}))
        del d_in, d_knz, d_out, d_loop, d_join, d_sp
        torch.cuda.empty_cache()
say()
say(json.dumps(result))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        f.write("\n".join(lines) + "\n")
