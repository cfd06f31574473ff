"""kz_knz_splice_device on a stream of 4 MiB blocks in HBM next to the two things it can be measured against, in one process:
   splice    all blocks of the stream, in order, into a new stream (the result is the stream itself), one call
   (a)       the only device route there was for the same bytes: k_knz_unpack into byte-aligned rows (the kernel's own time, taken
             from a kz_decompress_device call of the stream under kernel timing: the call that runs it), then
             kz_knz_assemble_device of those rows (timed as a call)
   (b)       a plain device copy of as many bytes as the stream has
The calls are timed with events on the context's stream, after a warm-up pass, REPS times; the median and the spread
(max - min) / median are printed, and the kernels' own time of the splice call besides.  NONE&NONE blocks of random bytes: the
stream is as long as the data, so the copy is all there is to time.
Diagnostic.   BLOCKS=64 REPS=9 python tools/knz_splice_probe.py"""
import json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz

BLOCKS = int(os.environ.get("BLOCKS", "64"))
REPS = int(os.environ.get("REPS", "9"))
bs = 4 << 20
chain, coder = "NONE", "NONE"
dev = torch.device("cuda", 0)
ctx = kz.Context(0)
st = torch.cuda.ExternalStream(ctx.stream, device=dev)                     # the events go on the context's own stream


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    r = fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def stats(v):
    m = float(np.median(v))
    return {"ms": round(m, 4), "spread": round((max(v) - min(v)) / m, 3)}


n = BLOCKS * bs
data = torch.randint(0, 256, (n + 1,), dtype=torch.uint8, device=dev)[1:]   # an odd address
cap = kz.compress_bound(n, bs)
knz = torch.empty(cap + 3, dtype=torch.uint8, device=dev)[3:]
torch.cuda.synchronize()
size = kz.compress_device(ctx, chain, coder, bs, data.data_ptr(), n, knz.data_ptr(), cap)
idx = kz.knz_index_device(ctx, knz.data_ptr(), size)
pieces, total = kz.splice_concat([idx])
assert len(pieces) == BLOCKS and total == n
out_cap = kz.knz_splice_bound([w for _, _, w in pieces])
out = torch.empty(out_cap + 5, dtype=torch.uint8, device=dev)[5:]

# ---- splice ----
t_splice = []
for it in range(REPS + 1):
    out.zero_(); torch.cuda.synchronize()
    t, got = timed(lambda: kz.knz_splice_device(ctx, knz.data_ptr(), [0], [size], pieces, total, out.data_ptr(), out_cap))
    assert got == size and torch.equal(out[:size], knz[:size])
    if it:
        t_splice.append(t)
ctx.set_kernel_timing(True); ctx.reset_kernel_timing()
kz.knz_splice_device(ctx, knz.data_ptr(), [0], [size], pieces, total, out.data_ptr(), out_cap)
k_splice = ctx.kernel_times()
ctx.reset_kernel_timing()

# ---- (a): the unpack kernel's time inside the call that runs it, then the assemble of rows ----
back = torch.empty(n, dtype=torch.uint8, device=dev)
t_unpack = []
for it in range(REPS + 1):
    ctx.reset_kernel_timing()
    assert kz.decompress_device(ctx, knz.data_ptr(), size, back.data_ptr(), n) == n
    if it:
        t_unpack.append(ctx.kernel_times()["k_knz_unpack"]["ms"])
ctx.set_kernel_timing(False); ctx.reset_kernel_timing()
assert torch.equal(back, data)
oS = kz.max_block_stream_bytes(bs)
rows = torch.empty(BLOCKS * oS, dtype=torch.uint8, device=dev)
res = kz.encode_blocks(ctx, chain, coder, data.data_ptr(), bs, [bs] * BLOCKS, rows.data_ptr(), oS, mem=kz.MEM_DEVICE)
bits = [int(r.bits) for r in res]
assert all(r.status == 0 for r in res) and bits == [w for _, _, w in pieces]
t_asm = []
for it in range(REPS + 1):
    out.zero_(); torch.cuda.synchronize()
    t, got = timed(lambda: kz.knz_assemble_device(ctx, chain, coder, bs, n, rows.data_ptr(), oS, bits, out.data_ptr(), out_cap))
    assert got == size and torch.equal(out[:size], knz[:size])
    if it:
        t_asm.append(t)

# ---- (b): a plain device copy of the stream's bytes ----
t_copy = []
with torch.cuda.stream(st):
    for it in range(REPS + 1):
        t, _ = timed(lambda: out[:size].copy_(knz[:size]))
        if it:
            t_copy.append(t)

r = {"blocks": BLOCKS, "stream_bytes": int(size), "splice": stats(t_splice),
     "splice_kernels_ms": {k: round(v["ms"], 4) for k, v in k_splice.items()},
     "a_unpack_kernel": stats(t_unpack), "a_assemble_call": stats(t_asm), "b_copy": stats(t_copy)}
r["a_total_ms"] = round(r["a_unpack_kernel"]["ms"] + r["a_assemble_call"]["ms"], 4)
gbs = lambda ms: round(2 * size / ms / 1e6, 1)                             # bytes read + bytes written
r["GBps"] = {"splice": gbs(r["splice"]["ms"]), "a": gbs(r["a_total_ms"]) , "b_copy": gbs(r["b_copy"]["ms"])}
print(json.dumps(r))
