"""The device-resident .knz stream next to what it is built from: the headline chain (BWT+RANK+ZRLT&ANS0) on B x 4 MiB blocks of the
bench's mix, as many as the card holds up to 2048, timed four ways in one run:
   1  encode_blocks + decode_blocks with MEM_DEVICE (block rows in HBM, no container)
   2  compress_device + decompress_device          (the .knz stream, HBM to HBM)
   3  kz_compress + kz_decompress                   (the .knz stream on host buffers)
   4  the k_knz_* kernels of a pass of (2), summed from the kernel timers
Diagnostic.   B=2048 python tools/knz_device_probe.py          (HOST=0 leaves row 3 out)"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import kanzi_amd as kz, datagen

D = 64; bs = 4 << 20
chain, coder = "BWT+RANK+ZRLT", "ANS0"
dev = torch.device("cuda", 0)
free, _ = torch.cuda.mem_get_info(dev)
B = max(8, min(int(os.environ.get("B", "2048")), int(free // (16 * bs))))      # in, rows, out, stream, staging and the coders' scratch
host = np.stack([datagen.block(k, bs) for k in range(D)])                 # the bench's mix (SURVEY 8d generator), tiled
d_in = torch.from_numpy(host).to(dev).repeat((B + D - 1) // D, 1)[:B].contiguous()
n = B * bs
o_stride = kz.max_block_stream_bytes(bs)
lengths = np.full(B, bs, dtype=np.int32)
ctx = kz.Context(0)
ctx.set_block_size(bs)
print(json.dumps({"blocks": B, "block_bytes": bs, "chain": chain + "&" + coder}), flush=True)


def row(name, enc_s, dec_s, extra=None):
    d = {"encode_s": round(enc_s, 4), "decode_s": round(dec_s, 4), "enc_GBps": round(n / enc_s / 1e9, 2), "dec_GBps": round(n / dec_s / 1e9, 2),
         "enc_dec_GBps": round(n / (enc_s + dec_s) / 1e9, 2)}
    d.update(extra or {})
    print(json.dumps({name: d}), flush=True)


# ---- 1: block rows ----
d_enc = torch.zeros((B, o_stride), dtype=torch.uint8, device=dev)
d_dec = torch.zeros((B, bs), dtype=torch.uint8, device=dev)
for it in range(2):                                                        # warm-up, then the measured pass
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = kz.encode_blocks(ctx, chain, coder, d_in.data_ptr(), bs, lengths, d_enc.data_ptr(), o_stride, kz.MEM_DEVICE)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    bits = np.array([r.bits for r in res], dtype=np.int64)
    res2 = kz.decode_blocks(ctx, chain, coder, bs, d_enc.data_ptr(), o_stride, bits, d_dec.data_ptr(), bs, kz.MEM_DEVICE)
    torch.cuda.synchronize(); t2 = time.perf_counter()
assert all(r.status == 0 for r in res) and all(r.status == 0 and r.length == bs for r in res2) and torch.equal(d_in, d_dec)
row("1 encode_blocks + decode_blocks (MEM_DEVICE)", t1 - t0, t2 - t1, {"coded_bytes": int((bits.sum() + 7) // 8)})
del d_enc
d_dec.zero_()

# ---- 2: the stream, HBM to HBM; the third pass with the kernel timers on (row 4) ----
cap = kz.compress_bound(n, bs)
d_knz = torch.empty(cap, dtype=torch.uint8, device=dev)
for it in range(5):
    # passes 0, 1: the default chunks (about 1 GiB: 256 blocks); 2: the kernel timers on (row 4); 3, 4: the whole batch as one chunk
    ctx.set_kernel_timing(it == 2); ctx.reset_kernel_timing()
    if it == 3:
        os.environ["KZ_STREAM_CHUNK"] = str(B); ctx.reload_switches()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    size = kz.compress_device(ctx, chain, coder, bs, d_in.data_ptr(), n, d_knz.data_ptr(), cap)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    back = kz.decompress_device(ctx, d_knz.data_ptr(), size, d_dec.data_ptr(), n)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    if it == 1:
        row("2 compress_device + decompress_device", t1 - t0, t2 - t1, {"stream_bytes": size})
    if it == 2:
        kt, tk = ctx.kernel_times(), (t1 - t0, t2 - t1)
    if it == 4:
        row("2b the same, KZ_STREAM_CHUNK=%d (one chunk)" % B, t1 - t0, t2 - t1, {"stream_bytes": size})
del os.environ["KZ_STREAM_CHUNK"]; ctx.reload_switches()
ctx.set_kernel_timing(False)
assert back == n and torch.equal(d_in.reshape(-1), d_dec.reshape(-1))
knz_dev = d_knz[:size].cpu().numpy()
print(json.dumps({"4 k_knz_* kernels of one pass of (2)": {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in kt.items() if k.startswith("k_knz_")},
                  "with_timers": {"encode_s": round(tk[0], 4), "decode_s": round(tk[1], 4)}}), flush=True)
del d_knz

# ---- 3: the stream on host buffers ----
if os.environ.get("HOST", "1") != "0":
    h_in = d_in.cpu().numpy().reshape(-1)
    h_knz = np.empty(cap, dtype=np.uint8)
    h_out = np.empty(n, dtype=np.uint8)
    for it in range(2):
        t0 = time.perf_counter()
        hsize = ctx.check(ctx.lib.kz_compress(ctx.h, kz.transform_type(chain), kz.ENTROPY_IDS[coder], bs, h_in.ctypes.data, n, h_knz.ctypes.data, cap))
        t1 = time.perf_counter()
        hback = ctx.check(ctx.lib.kz_decompress(ctx.h, h_knz.ctypes.data, hsize, h_out.ctypes.data, n))
        t2 = time.perf_counter()
    assert hsize == size and np.array_equal(h_knz[:hsize], knz_dev) and hback == n and np.array_equal(h_out, h_in)
    row("3 kz_compress + kz_decompress (host buffers)", t1 - t0, t2 - t1, {"stream_bytes": hsize, "equal_to_device_stream": True})
