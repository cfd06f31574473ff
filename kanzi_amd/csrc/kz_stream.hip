// kz_stream.hip -- host side of the .knz container around the HIP block pipeline: the part of
// K/io/CompressedOutputStream.java (writeHeader :236-313, ordered block emission :1024-1035, end
// marker :483-493) and K/io/CompressedInputStream.java (readHeader :359-515, block length prefix
// :1127-1129) that stays on the CPU.  Blocks go to the GPU in batches (kz_encode_blocks /
// kz_decode_blocks); only the bit-granular concatenation happens here.
#include "kz_internal.h"
#include <stdlib.h>
#include <algorithm>
#include <memory>
#include <thread>
#include <atomic>
#include <mutex>
#include <condition_variable>

namespace {
struct HostBits {            // MSB-first writer (DefaultOutputBitStream.java:103-205)
  uint8_t* p; int64_t cap; uint64_t pos; bool overflow;
  void put(uint64_t v, int count) {
    if (count <= 0) return;
    if ((int64_t)((pos + count + 7) >> 3) > cap) { overflow = true; return; }
    if (count < 64) v &= ((1ULL << count) - 1);
    while (count > 0) {
      const int bitoff = (int)(pos & 7), room = 8 - bitoff;
      const int take = count < room ? count : room;
      const uint8_t bits = (uint8_t)((v >> (count - take)) & ((1u << take) - 1));
      if (bitoff == 0) p[pos >> 3] = 0;
      p[pos >> 3] |= (uint8_t)(bits << (room - take));
      pos += take; count -= take;
    }
  }
  void putBytes(const uint8_t* s, uint64_t nbits) {
    if (!nbits) return;
    if ((int64_t)((pos + nbits + 7) >> 3) > cap) { overflow = true; return; }
    const int sh = (int)(pos & 7);
    const uint64_t full = nbits >> 3;
    if (sh == 0) { memcpy(p + (pos >> 3), s, (size_t)full); pos += full << 3; }
    else {
      uint8_t* d = p + (pos >> 3);
      const int up = 8 - sh;
      if (full) {
        d[0] = (uint8_t)((d[0] & (0xFF << up)) | (s[0] >> sh));         // keep the bits already in the partial byte
        for (uint64_t i = 1; i < full; i++) d[i] = (uint8_t)((s[i - 1] << up) | (s[i] >> sh));   // no carried dependency: vectorises
        d[full] = (uint8_t)(s[full - 1] << up);
      }
      pos += full << 3;
    }
    const int r = (int)(nbits & 7);
    if (r) put((uint64_t)(s[full] >> (8 - r)), r);
  }
};
struct HostBitsIn {
  const uint8_t* p; uint64_t nbits; uint64_t pos; bool error;
  uint64_t get(int count) {
    if (count <= 0) return 0;
    if (pos + (uint64_t)count > nbits) { error = true; pos = nbits; return 0; }
    uint64_t v = 0;
    while (count > 0) {
      const int bitoff = (int)(pos & 7), room = 8 - bitoff;
      const int take = count < room ? count : room;
      v = (v << take) | (uint64_t)((p[pos >> 3] >> (room - take)) & ((1u << take) - 1));
      pos += take; count -= take;
    }
    return v;
  }
  void getBytes(uint8_t* d, uint64_t nb) {
    if (pos + nb > nbits) { error = true; pos = nbits; return; }
    const int sh = (int)(pos & 7);
    const uint64_t full = nb >> 3;
    const uint8_t* s = p + (pos >> 3);
    if (sh == 0) memcpy(d, s, (size_t)full);
    else for (uint64_t i = 0; i < full; i++) d[i] = (uint8_t)((s[i] << sh) | (s[i + 1] >> (8 - sh)));
    pos += full << 3;
    const int r = (int)(nb & 7);
    if (r) d[full] = (uint8_t)(get(r) << (8 - r));
  }
};
inline uint32_t mix32(uint32_t c, uint32_t h, uint32_t v) { c ^= h * ~v; c = (c << 13) | (c >> 19); return c * 5u + 0x52DCE729u; }
inline int ilog2(uint32_t x) { return 31 - __builtin_clz(x); }

uint32_t header_cksum(int chkKind, int entropyType, uint64_t tt, int blockSize, int szMask, int64_t inputSize) {
  const uint32_t HASH = 0x1E35A7BDu;                          // CompressedOutputStream.java:293-309
  uint32_t c = HASH * (0x01030507u * 7u);
  c = mix32(c, HASH, (uint32_t)chkKind);
  c = mix32(c, HASH, (uint32_t)entropyType);
  c = mix32(c, HASH, (uint32_t)(tt >> 32));
  c = mix32(c, HASH, (uint32_t)tt);
  c = mix32(c, HASH, (uint32_t)blockSize);
  if (szMask > 0) { c = mix32(c, HASH, (uint32_t)((uint64_t)inputSize >> 32)); c = mix32(c, HASH, (uint32_t)inputSize); }
  return ((c >> 23) ^ (c >> 3)) & 0xFFFFFF;
}
int batch_blocks(int blockSize) {
  // blocks per kz_encode_blocks / kz_decode_blocks call of the host-buffer entry points: 8 GiB of input per call
  // (device scratch is bounded separately by the arena budget, which splits a call into sub-batches); the
  // serial kernels want a thousand blocks or more in flight.  The strided host staging buffers are allocated
  // uninitialised, so only the bytes actually produced/consumed are ever touched.
  return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (8LL << 30) / blockSize));
}
}  // namespace

// ---- host-only container helpers (no GPU needed): used by kz_compress and by multi-GPU gathers ----
static int write_stream_header(HostBits& bs, uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t n, int chkKind = 0) {
  bs.put(0x4B414E5A, 32); bs.put(7, 4); bs.put((uint64_t)chkKind, 2);
  bs.put(entropyType, 5); bs.put(transformType, 48); bs.put((uint32_t)blockSize >> 4, 28);
  int szMask = 0;
  if (n != 0 && n < (1LL << 48)) {
    if (n >= (1LL << 32)) szMask = 3;
    else { int64_t isz = n; if (isz > (1LL << 30)) { isz >>= 4; szMask++; } szMask += (ilog2((uint32_t)isz) >> 4) + 1; }
  }
  bs.put((uint64_t)szMask, 2);
  if (szMask > 0) bs.put((uint64_t)n, 16 * szMask);
  bs.put(0, 15);
  bs.put(header_cksum(chkKind, (int)entropyType, transformType, blockSize, szMask, n), 24);
  return szMask;
}
static void write_block(HostBits& bs, const uint8_t* stream, uint64_t written) {   // :1024-1035
  const int lw = (written < 8) ? 3 : ilog2((uint32_t)(written >> 3)) + 4;
  bs.put((uint64_t)(lw - 3), 5);
  bs.put(written, lw);
  bs.putBytes(stream, written);
}

// Assemble a complete .knz stream from per-block private streams (e.g. gathered from several GPUs
// in block-id order).  Pure host code.
extern "C" int64_t kz_knz_assemble(uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                                   int32_t checksumBits, const uint8_t* streams, int64_t stride, const int64_t* bits, int32_t nBlocks,
                                   uint8_t* dst, int64_t dstCap) {
  if (!dst || nBlocks < 0 || (nBlocks > 0 && (!streams || !bits))) return -KZ_ERR_INVALID_PARAM;
  if (checksumBits != 0 && checksumBits != 32 && checksumBits != 64) return -KZ_ERR_INVALID_PARAM;
  HostBits bs{dst, dstCap, 0, false};
  // the block streams carry 4 / 8 hash bytes in their headers when they were coded with kz_ctx_set_checksum(32 / 64): the
  // stream header must say so (CompressedOutputStream.java:244-250) or no reader can parse them
  write_stream_header(bs, transformType, entropyType, blockSize, inputSize, checksumBits == 32 ? 1 : (checksumBits == 64 ? 2 : 0));
  for (int i = 0; i < nBlocks; i++) if (bits[i] > 0) write_block(bs, streams + (int64_t)i * stride, (uint64_t)bits[i]);
  bs.put(0, 5); bs.put(0, 3);
  if (bs.overflow) return -KZ_ERR_WRITE_FILE;
  return (int64_t)((bs.pos + 7) >> 3);
}

// The same, block by block: a gatherer (rank 0 of a multi-GPU job) appends block streams in block-id order as they arrive instead
// of holding all of them first; memory is one block plus the destination.
struct kz_knz_writer { HostBits bs; };
extern "C" kz_knz_writer* kz_knz_writer_open(uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                                             int32_t checksumBits, uint8_t* dst, int64_t dstCap) {
  if (!dst || dstCap < 32 || (checksumBits != 0 && checksumBits != 32 && checksumBits != 64)) return nullptr;
  kz_knz_writer* w = new kz_knz_writer{HostBits{dst, dstCap, 0, false}};
  write_stream_header(w->bs, transformType, entropyType, blockSize, inputSize, checksumBits == 32 ? 1 : (checksumBits == 64 ? 2 : 0));
  return w;
}
extern "C" int32_t kz_knz_writer_add(kz_knz_writer* w, const uint8_t* stream, int64_t bits) {
  if (!w || bits < 0 || (bits > 0 && !stream)) return -KZ_ERR_INVALID_PARAM;
  if (bits > 0) write_block(w->bs, stream, (uint64_t)bits);
  return w->bs.overflow ? -KZ_ERR_WRITE_FILE : 0;
}
extern "C" int64_t kz_knz_writer_close(kz_knz_writer* w) {          // end marker (:491-492); returns the stream's size in bytes
  if (!w) return -KZ_ERR_INVALID_PARAM;
  w->bs.put(0, 5); w->bs.put(0, 3);
  const int64_t r = w->bs.overflow ? -KZ_ERR_WRITE_FILE : (int64_t)((w->bs.pos + 7) >> 3);
  delete w;
  return r;
}

// Parse the stream header and walk the block length prefixes: blockBitOff[i] = bit offset of block
// i's private stream inside src, blockBits[i] = its length W.  Returns the number of blocks or <0.
// Stream header, checked in the reference's order and with its codes (CompressedInputStream.java:359-478).
struct KnzHeader { int chkKind, entropyType, blockSize, szMask; uint64_t transformType; int64_t inputSize; };
static int read_stream_header(HostBitsIn& bs, KnzHeader& h, char* err, size_t errCap) {
  if (bs.get(32) != 0x4B414E5A) return -KZ_ERR_INVALID_FILE;                                    // :367-368
  const int bsVersion = (int)bs.get(4);
  if (bsVersion != 7) {                                                                            // :374-377; older layouts are not built here
    if (err) snprintf(err, errCap, "cannot read this version of the stream: %d (only 7 is built)", bsVersion);
    return -KZ_ERR_STREAM_VERSION;
  }
  h.chkKind = (int)bs.get(2);
  if (h.chkKind > 2) return -KZ_ERR_INVALID_FILE;                                               // :390-392
  h.entropyType = (int)bs.get(5);
  if (h.entropyType == 3 || h.entropyType > 9) return -KZ_ERR_INVALID_CODEC;                     // EntropyCodecFactory.getName :212-243
  h.transformType = bs.get(48);
  for (int i = 0; i < 8; i++) {                                                                  // TransformFactory.getName :368-449
    const int t = (int)((h.transformType >> (42 - 6 * i)) & 0x3F);
    if (t == 4 || t > 19) return -KZ_ERR_INVALID_CODEC;
  }
  h.blockSize = (int)(bs.get(28) << 4);
  if (h.blockSize < 1024 || h.blockSize > (1 << 30)) return -KZ_ERR_BLOCK_SIZE;                  // :419-422
  h.szMask = (int)bs.get(2);
  h.inputSize = h.szMask ? (int64_t)bs.get(16 * h.szMask) : 0;
  bs.get(15);
  const uint32_t ck = (uint32_t)bs.get(24);
  if (bs.error || ck != header_cksum(h.chkKind, h.entropyType, h.transformType, h.blockSize, h.szMask, h.inputSize))
    return -KZ_ERR_CRC_CHECK;                                                                    // :477-478
  return 0;
}

extern "C" int32_t kz_knz_index(const uint8_t* src, int64_t n, uint64_t* transformType, uint32_t* entropyType,
                                int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits, int64_t* blockBitOff, int64_t* blockBits, int32_t cap) {
  if (!src || n < 20) return -KZ_ERR_INVALID_FILE;
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, nullptr, 0); if (hrc) return hrc; }
  const uint64_t tt = h.transformType; const int et = h.entropyType, bsz = h.blockSize; const int64_t isz = h.inputSize;
  if (transformType) *transformType = tt;
  if (entropyType) *entropyType = (uint32_t)et;
  if (blockSize) *blockSize = bsz;
  if (inputSize) *inputSize = isz;
  if (checksumBits) *checksumBits = h.chkKind == 1 ? 32 : (h.chkKind == 2 ? 64 : 0);
  int nb = 0;
  for (;;) {
    const int lr = (int)bs.get(5) + 3;
    const uint64_t rd = bs.get(lr);
    if (bs.error) return -KZ_ERR_READ_FILE;
    if (rd == 0) break;
    if (nb < cap) { if (blockBitOff) blockBitOff[nb] = (int64_t)bs.pos; if (blockBits) blockBits[nb] = (int64_t)rd; }
    nb++;
    if (bs.pos + rd > bs.nbits) return -KZ_ERR_READ_FILE;
    bs.pos += rd;
  }
  return nb;
}


// run fn(i) for i in [0, n) on the host pool (blocks are independent)
template <typename F>
static void parallel_blocks(int n, F fn, int maxThreads = 32) {
  struct Thunk { static void run(int i, void* a) { (*(F*)a)(i); } };
  kz_parallel_for(n, maxThreads, &Thunk::run, (void*)&fn);
}

// Ordered emission of a batch (CompressedOutputStream.java:1024-1035) at bit granularity.  The serial pass writes,
// per block, the 5-bit / lw-bit length prefix and the (at most 7 + 7) payload bits that share a byte with a
// neighbour, skipping the bytes that belong to one payload only; those interiors are then copied (shifted) by a
// few threads.
static void emit_blocks(HostBits& bs, const uint8_t* streams, int64_t stride, const kz_block_result* res, int cnt) {
  struct Job { const uint8_t* s; uint8_t* d; uint64_t nbytes; int e; };
  std::vector<Job> jobs;
  jobs.reserve(cnt);
  for (int i = 0; i < cnt; i++) {
    const uint64_t W = (uint64_t)res[i].bits;
    if (W == 0) continue;
    const uint8_t* s = streams + (size_t)i * stride;
    const int lw = (W < 8) ? 3 : ilog2((uint32_t)(W >> 3)) + 4;
    bs.put((uint64_t)(lw - 3), 5);
    bs.put(W, lw);
    if (bs.overflow || (int64_t)((bs.pos + W + 7) >> 3) > bs.cap) { bs.overflow = true; return; }
    const int e = (int)((8 - (bs.pos & 7)) & 7);                  // payload bits that complete the current byte
    if (W < (uint64_t)e + 16) { bs.putBytes(s, W); continue; }    // tiny block: all serial
    if (e) bs.put((uint64_t)(s[0] >> (8 - e)), e);
    const uint64_t nbytes = (W - (uint64_t)e) >> 3;               // whole bytes owned by this payload alone
    jobs.push_back({s, bs.p + (bs.pos >> 3), nbytes, e});
    bs.pos += nbytes << 3;
    const int r = (int)((W - (uint64_t)e) & 7);                   // trailing bits
    if (r) {
      const uint64_t bitoff = (uint64_t)e + (nbytes << 3);
      const uint32_t two = ((uint32_t)s[bitoff >> 3] << 8) | (uint32_t)s[(bitoff >> 3) + 1];
      bs.put((uint64_t)((two >> (16 - (int)(bitoff & 7) - r)) & ((1u << r) - 1)), r);
    }
  }
  parallel_blocks((int)jobs.size(), [&](int k) {
    const Job& j = jobs[k];
    if (j.e == 0) { memcpy(j.d, j.s, (size_t)j.nbytes); return; }
    const int e = j.e, up = 8 - e;
    for (uint64_t i = 0; i < j.nbytes; i++) j.d[i] = (uint8_t)((j.s[i] << e) | (j.s[i + 1] >> up));
  });
}

extern "C" int64_t kz_compress_bound(int64_t n, int32_t blockSize) {
  if (n < 0 || blockSize <= 0) return -KZ_ERR_INVALID_PARAM;
  const int64_t nBlocks = (n + blockSize - 1) / blockSize;
  // per block: its stream (kz_max_block_stream_bytes) + length prefix and checksum; stream header, end marker, padding
  return 64 + nBlocks * (kz_max_block_stream_bytes((int32_t)std::min<int64_t>(n, blockSize)) + 24);
}

// ---- staging for the host-buffer stream calls: pinned host memory and HBM outside the arena, grow-only, kept by the context ----
static int stage_reserve(kz_ctx* ctx, kz_ctx::Stage& s, size_t need, bool pinned) { return kz_stage_reserve(ctx, s, need, pinned); }
static int stage_streams(kz_ctx* ctx) {
  if (!ctx->copyUp) KZ_HIP(hipStreamCreateWithFlags(&ctx->copyUp, hipStreamNonBlocking));
  if (!ctx->copyDown) KZ_HIP(hipStreamCreateWithFlags(&ctx->copyDown, hipStreamNonBlocking));
  return 0;
}
static int stream_chunk_blocks(const kz_ctx* ctx, int blockSize) {   // blocks per pipeline step of kz_compress: about 1 GiB of input
  if (ctx->sw.streamChunk > 0) return ctx->sw.streamChunk;
  return (int)std::max<int64_t>(8, std::min<int64_t>(2048, (1LL << 30) / blockSize));
}
struct BlockSizeScope {                                            // the context's "blockSize" entry = this stream's (TEXT reads it)
  kz_ctx* c; int saved; bool savedSet;
  BlockSizeScope(kz_ctx* c_, int v) : c(c_), saved(c_->blockSize), savedSet(c_->blockSizeSet) { c->blockSize = v; c->blockSizeSet = true; }
  ~BlockSizeScope() { c->blockSize = saved; c->blockSizeSet = savedSet; }
};

// Inputs of several chunks: a three-stage pipeline like the reference's task pool (K/io/CompressedOutputStream.java:541-566 fills
// `jobs` buffers, codes them side by side and emits in order).  Thread U stages chunk k+1 (host TEXT / UTF stages, copy into pinned
// memory, H2D on its own stream), the calling thread codes chunk k on the GPU (HBM in, HBM out), thread D brings chunk k-1 back
// (D2H of the bytes produced, ordered bit-granular emission into dst).  Blocks are independent: the stream is the same as the
// one-batch-at-a-time form's.
static int64_t compress_pipelined(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                                  const uint8_t* src, int64_t n, HostBits& bs, int64_t nblocks, int CH) {
  const int nch = (int)((nblocks + CH - 1) / CH);
  const int64_t oS = kz_max_block_stream_bytes(blockSize);
  { int rc = stage_streams(ctx); if (rc) return rc; }
  for (int i = 0; i < 2; i++) {
    int rc = stage_reserve(ctx, ctx->pinIn[i], (size_t)CH * blockSize, true);
    if (!rc) rc = stage_reserve(ctx, ctx->devIn[i], (size_t)CH * blockSize, false);
    if (!rc) rc = stage_reserve(ctx, ctx->devOut[i], (size_t)CH * oS, false);
    if (!rc) rc = stage_reserve(ctx, ctx->pinOut[i], (size_t)CH * oS, true);
    if (rc) return rc;
  }
  struct Chunk { std::vector<int32_t> lens; std::vector<kz_block_result> res; HostPre* pre = nullptr; };
  std::vector<Chunk> ck(nch);
  std::mutex mu;
  std::condition_variable cv;
  int uploaded = 0, encoded = 0, emitted = 0, failed = 0;          // chunks through each stage (under mu)
  auto fail = [&](int code) { std::lock_guard<std::mutex> g(mu); if (!failed) failed = code; cv.notify_all(); };
  const int dev = ctx->device;
  std::thread U([&]() {
    if (hipSetDevice(dev) != hipSuccess) { fail(-KZ_ERR_DEVICE); return; }
    for (int k = 0; k < nch; k++) {
      { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return failed || encoded >= k - 1; }); if (failed) return; }   // slot k & 1 is free
      const int64_t b0 = (int64_t)k * CH;
      const int cnt = (int)std::min<int64_t>(CH, nblocks - b0);
      ck[k].lens.resize(cnt);
      for (int i = 0; i < cnt; i++) ck[k].lens[i] = (int32_t)std::min<int64_t>(blockSize, n - (b0 + i) * blockSize);
      const uint8_t* cs = src + b0 * blockSize;
      // (a chunk whose TEXT stage runs on the device is not pre-staged: kz_encode_blocks_pre does it from the uploaded blocks)
      ck[k].pre = kz_text_fwd_gpu_applies(ctx, transformType, entropyType, cnt) ? nullptr
                : kz_host_prestage(ctx, transformType, entropyType, blockSize, cs, blockSize, ck[k].lens.data(), cnt, k & 1);
      uint8_t* pin = ctx->pinIn[k & 1].p;
      const int64_t bytes = std::min<int64_t>((int64_t)cnt * blockSize, n - b0 * blockSize);
      const int pieces = (int)((bytes + (8 << 20) - 1) / (8 << 20));
      parallel_blocks(pieces, [&](int q) { const int64_t o = (int64_t)q << 23; memcpy(pin + o, cs + o, (size_t)std::min<int64_t>(8 << 20, bytes - o)); });
      if (hipMemcpyAsync(ctx->devIn[k & 1].p, pin, (size_t)bytes, hipMemcpyHostToDevice, ctx->copyUp) != hipSuccess ||
          hipStreamSynchronize(ctx->copyUp) != hipSuccess) { fail(-KZ_ERR_DEVICE); return; }
      { std::lock_guard<std::mutex> g(mu); uploaded = k + 1; }
      cv.notify_all();
    }
  });
  std::thread D([&]() {
    if (hipSetDevice(dev) != hipSuccess) { fail(-KZ_ERR_DEVICE); return; }
    for (int k = 0; k < nch; k++) {
      { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return failed || encoded >= k + 1; }); if (failed) return; }
      const int cnt = (int)ck[k].lens.size();
      uint8_t* pin = ctx->pinOut[k & 1].p;
      const uint8_t* d = ctx->devOut[k & 1].p;
      bool ok = true;
      for (int i = 0; i < cnt && ok; i++) {
        if (ck[k].res[i].status) { fail(ck[k].res[i].status); return; }
        const size_t nby = (size_t)((ck[k].res[i].bits + 7) >> 3);
        if (nby) ok = hipMemcpyAsync(pin + (size_t)i * oS, d + (size_t)i * oS, nby + 1 <= (size_t)oS ? nby + 1 : nby, hipMemcpyDeviceToHost, ctx->copyDown) == hipSuccess;
      }
      if (!ok || hipStreamSynchronize(ctx->copyDown) != hipSuccess) { fail(-KZ_ERR_DEVICE); return; }
      emit_blocks(bs, pin, oS, ck[k].res.data(), cnt);              // ordered emission (:1024-1035)
      if (bs.overflow) { fail(-KZ_ERR_WRITE_FILE); return; }
      { std::lock_guard<std::mutex> g(mu); emitted = k + 1; }
      cv.notify_all();
    }
  });
  for (int k = 0; k < nch; k++) {
    { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return failed || (uploaded >= k + 1 && emitted >= k - 1); }); if (failed) break; }
    const int cnt = (int)ck[k].lens.size();
    ck[k].res.resize(cnt);
    const int rc = kz_encode_blocks_pre(ctx, transformType, entropyType, blockSize, ctx->devIn[k & 1].p, blockSize, ck[k].lens.data(), cnt,
                                        ctx->devOut[k & 1].p, oS, ck[k].res.data(), KZ_MEM_DEVICE, ck[k].pre);
    kz_host_pre_free(ck[k].pre); ck[k].pre = nullptr;
    if (rc) { fail(rc); break; }
    { std::lock_guard<std::mutex> g(mu); encoded = k + 1; }
    cv.notify_all();
  }
  U.join(); D.join();
  for (auto& c : ck) kz_host_pre_free(c.pre);
  return failed;
}

extern "C" int64_t kz_compress(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                               const uint8_t* src, int64_t n, uint8_t* dst, int64_t dstCap) {
  if (!ctx || !src || !dst || n < 0) return -KZ_ERR_INVALID_PARAM;
  if (blockSize < 1024 || blockSize > (1 << 30) || (blockSize & 15)) return -KZ_ERR_BLOCK_SIZE;   // :165-174
  KZ_HIP(hipSetDevice(ctx->device));
  HostBits bs{dst, dstCap, 0, false};
  // ---- stream header (CompressedOutputStream.java:236-313) ----
  write_stream_header(bs, transformType, entropyType, blockSize, n, ctx->checksum);
  const int64_t nblocks = (n + blockSize - 1) / blockSize;
  BlockSizeScope scope(ctx, blockSize);
  const int CH = stream_chunk_blocks(ctx, blockSize);
  if (nblocks >= 2LL * CH && !ctx->sw.streamSerial) {
    const int64_t rc = compress_pipelined(ctx, transformType, entropyType, blockSize, src, n, bs, nblocks, CH);
    if (rc == -KZ_ERR_WRITE_FILE) snprintf(ctx->err, sizeof(ctx->err), "kz_compress: destination too small");
    if (rc) return rc;
  } else {
    // ---- blocks, one batch after the other ----
    const int NB = batch_blocks(blockSize);
    const int64_t oS = kz_max_block_stream_bytes(blockSize);
    std::unique_ptr<uint8_t[]> outbuf(new uint8_t[(size_t)oS * (size_t)std::min<int64_t>(NB, std::max<int64_t>(nblocks, 1))]);
    std::vector<int32_t> lens(NB);
    std::vector<kz_block_result> res(NB);
    for (int64_t b0 = 0; b0 < nblocks; b0 += NB) {
      const int cnt = (int)std::min<int64_t>(NB, nblocks - b0);
      for (int i = 0; i < cnt; i++) lens[i] = (int32_t)std::min<int64_t>(blockSize, n - (b0 + i) * blockSize);
      int rc = kz_encode_blocks(ctx, transformType, entropyType, src + b0 * blockSize, blockSize, lens.data(), cnt,
                                outbuf.get(), oS, res.data(), KZ_MEM_HOST);
      if (rc) return rc;
      for (int i = 0; i < cnt; i++) if (res[i].status) return res[i].status;
      emit_blocks(bs, outbuf.get(), oS, res.data(), cnt);           // ordered emission (:1024-1035)
      if (bs.overflow) break;
    }
  }
  bs.put(0, 5); bs.put(0, 3);                                   // end marker (:491-492)
  if (bs.overflow) { snprintf(ctx->err, sizeof(ctx->err), "kz_compress: destination too small"); return -KZ_ERR_WRITE_FILE; }
  return (int64_t)((bs.pos + 7) >> 3);
}


// Host restatement of DecodingTask.readBlockHeader + the two checks that follow it
// (CompressedInputStream.java:1025-1095, :1145-1164): the reference validates a block's header on the shared
// bit stream BEFORE it reads the payload, so a truncated or tampered stream is reported with the header's error
// (ERR_CRC_CHECK / ERR_BLOCK_SIZE / ERR_READ_FILE), not as a short read.  Returns 0 or -(error code).
static int precheck_block_header(HostBitsIn bs /* by value: peek */, uint64_t W, int nbFunctions, int blockSize, int chkKind) {
  if (W < 8) return -KZ_ERR_BLOCK_SIZE;
  const uint32_t mode = (uint32_t)bs.get(8);
  uint32_t skipFlags = 0;
  bool hasSkip = false;
  if (mode & 0x80) {
    if (mode & 0x10) { if (nbFunctions > 4) hasSkip = true; else skipFlags = ((mode << 4) | 0x0F) & 0xFF; }
  } else if (mode & 0x10) hasSkip = true;
  else skipFlags = ((mode << 4) | 0x0F) & 0xFF;
  const int dataSize = 1 + (int)((mode >> 5) & 3);
  const int headerSize = 1 + (hasSkip ? 1 : 0) + dataSize + 1;
  if (W < (uint64_t)headerSize * 8) return -KZ_ERR_BLOCK_SIZE;
  if (hasSkip) skipFlags = (uint32_t)bs.get(8);
  uint32_t preLen = 0;
  for (int i = 0; i < dataSize; i++) preLen = (preLen << 8) | (uint32_t)bs.get(8);
  const uint32_t ck = (uint32_t)bs.get(8);
  if (bs.error) return -KZ_ERR_READ_FILE;
  const uint32_t HASH = 0x1E35A7BDu;
  uint32_t c = HASH * 0x01030507u;
  c = mix32(c, HASH, mode & 0xFF);
  c = mix32(c, HASH, skipFlags & 0xFF);
  c = mix32(c, HASH, preLen);
  c = mix32(c, HASH, (uint32_t)(W >> 32));
  c = mix32(c, HASH, (uint32_t)W);
  c = (c >> 23) ^ (c >> 3);
  if (ck != (c & 0xFF)) return -KZ_ERR_CRC_CHECK;
  const int64_t maxTL = std::min<int64_t>(std::max<int64_t>((int64_t)blockSize + blockSize / 2, 2048), 1LL << 30);
  if ((int32_t)preLen < 0 || (int64_t)preLen > maxTL) return -KZ_ERR_READ_FILE;
  const int checksumSize = (chkKind == 2) ? 8 : (chkKind == 1 ? 4 : 0);
  if ((int64_t)((W + 7) >> 3) > (int64_t)preLen + headerSize + checksumSize) return -KZ_ERR_BLOCK_SIZE;
  return 0;
}

// kz_decompress and kz_decompress_range: the blocks [firstBlock, firstBlock + nBlocks) of the stream, nBlocks < 0: from firstBlock
// to the end marker.  Blocks in front of firstBlock get the walk's checks and nothing else; the batches, and with them the place
// where a destination that is too small cuts the stream, start at firstBlock.
static int64_t decompress_host(kz_ctx* ctx, const uint8_t* src, int64_t n, int64_t firstBlock, int64_t nBlocks, uint8_t* dst, int64_t dstCap) {
  KZ_HIP(hipSetDevice(ctx->device));
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, ctx->err, sizeof(ctx->err)); if (hrc) return hrc; }
  const int chkKind = h.chkKind, entropyType = h.entropyType, blockSize = h.blockSize, szMask = h.szMask;
  const uint64_t tt = h.transformType; const int64_t inputSize = h.inputSize;
  const int savedChk = ctx->checksum;
  ctx->checksum = chkKind;
  struct Restore { kz_ctx* c; int v; ~Restore() { c->checksum = v; } } restore_{ctx, savedChk};
  int nbFunctions = 0;
  for (int i = 0; i < 8; i++) if (((tt >> (42 - 6 * i)) & 0x3F) != 0) nbFunctions++;         // Sequence length (TransformFactory.java:240-266)
  if (nbFunctions == 0) nbFunctions = 1;
  int NB = batch_blocks(blockSize);
  // no more staging than the stream can need: declared size if present, else >= 8 bytes of stream per block
  if (szMask && inputSize > 0) NB = (int)std::min<int64_t>(NB, (inputSize + blockSize - 1) / blockSize);
  else NB = (int)std::min<int64_t>(NB, n / 8 + 1);
  const int64_t iS = (int64_t)kz_align((size_t)blockSize + (size_t)(blockSize >> 3) + 1024 + 64, 256);
  if (nBlocks == 0) return 0;
  for (int64_t k = 0; k < firstBlock; k++) {                      // read and skipped (:1126-1165 come before the reader looks at "from")
    const int lr = (int)bs.get(5) + 3;
    const uint64_t rd = bs.get(lr);
    if (bs.error) return -KZ_ERR_READ_FILE;
    if (rd == 0) return 0;                                        // the end marker in front of the range
    int rc = precheck_block_header(bs, rd, nbFunctions, blockSize, chkKind);
    if (!rc && (int64_t)((rd + 7) >> 3) > iS - 64) rc = -KZ_ERR_BLOCK_SIZE;
    if (!rc && bs.pos + rd > bs.nbits) rc = -KZ_ERR_READ_FILE;
    if (rc) return rc;
    bs.pos += rd;
  }
  int64_t left = nBlocks < 0 ? INT64_MAX : nBlocks;               // blocks of the range not walked yet
  std::unique_ptr<uint8_t[]> inbuf;                                // (the unstaged path's strided copy of the payloads)
  std::vector<int64_t> bits(NB);
  std::vector<uint64_t> starts(NB);
  std::vector<kz_block_result> res(NB);
  int64_t produced = 0;
  bool done = false;
  int pending = 0;
  while (!done) {
    int cnt = 0;
    // A fault met while walking the length prefixes is held back until the blocks before it have been decoded:
    // the reference reports the FIRST failing block in stream order (processedBlockId ordering, :1127-1170).
    while (cnt < NB) {                                          // serial walk of block length prefixes (:1127-1129)
      if (left == 0) { done = true; break; }                    // the end of the range: nothing behind it is read
      const int lr = (int)bs.get(5) + 3;
      const uint64_t rd = bs.get(lr);
      if (bs.error) { pending = -KZ_ERR_READ_FILE; break; }
      if (rd == 0) { done = true; break; }
      pending = precheck_block_header(bs, rd, nbFunctions, blockSize, chkKind);
      if (!pending && (int64_t)((rd + 7) >> 3) > iS - 64) pending = -KZ_ERR_BLOCK_SIZE;
      if (!pending && bs.pos + rd > bs.nbits) pending = -KZ_ERR_READ_FILE;
      if (pending) break;
      starts[cnt] = bs.pos;                                     // the payload is extracted below, by several threads
      bs.pos += rd;
      bits[cnt++] = (int64_t)rd;
      left--;
    }
    if (pending) done = true;
    if (cnt == 0) break;
    {
      // Blocks that start past the end of the destination cannot be stored: that is this interface's fault to report
      // (ERR_WRITE_FILE), but only if every block before them decodes -- the reader reports the first failing block.
      const int64_t room = dstCap - produced;
      const int64_t fit = (room <= 0) ? 0 : (room + blockSize - 1) / blockSize;
      if (fit < cnt) { cnt = (int)fit; pending = -KZ_ERR_WRITE_FILE; done = true; }
      if (cnt == 0) break;
    }
    if (cnt >= 16 && !ctx->sw.streamSerial) {
      // ---- staged batch: payloads are extracted (bit-shifted) straight into pinned memory, go to HBM with asynchronous copies,
      //      the batch is decoded HBM -> HBM, and the blocks come back through a pinned ring while host threads move the previous
      //      piece to its place in dst ----
      { int rc = stage_streams(ctx); if (rc) return rc; }
      std::vector<int64_t> off(cnt + 1, 0);
      for (int i = 0; i < cnt; i++) off[i + 1] = off[i] + (int64_t)kz_align((size_t)((bits[i] + 7) >> 3) + 64, 256);
      const int P = (int)std::max<int64_t>(1, std::min<int64_t>(cnt, (256LL << 20) / blockSize));   // blocks per piece of the way back
      int rc = stage_reserve(ctx, ctx->pinIn[0], (size_t)off[cnt], true);
      if (!rc) rc = stage_reserve(ctx, ctx->devIn[0], (size_t)cnt * iS, false);
      if (!rc) rc = stage_reserve(ctx, ctx->devOut[0], (size_t)cnt * blockSize, false);
      for (int q = 0; q < 2 && !rc; q++) rc = stage_reserve(ctx, ctx->pinOut[q], (size_t)P * blockSize, true);
      if (rc) return rc;
      uint8_t* pin = ctx->pinIn[0].p;
      parallel_blocks(cnt, [&](int i) { HostBitsIn t = bs; t.pos = starts[i]; t.error = false; t.getBytes(pin + off[i], (uint64_t)bits[i]); });
      for (int i = 0; i < cnt; i++)
        KZ_HIP(hipMemcpyAsync(ctx->devIn[0].p + (size_t)i * iS, pin + off[i], (size_t)((bits[i] + 7) >> 3), hipMemcpyHostToDevice, ctx->copyUp));
      KZ_HIP(hipStreamSynchronize(ctx->copyUp));
      rc = kz_decode_blocks(ctx, tt, (uint32_t)entropyType, blockSize, ctx->devIn[0].p, iS, bits.data(), cnt,
                            ctx->devOut[0].p, blockSize, res.data(), KZ_MEM_DEVICE);
      if (rc) return rc;
      // where every block goes: the reader appends whatever a block produced (:783-785); the first failing block ends the stream
      std::vector<int64_t> at(cnt + 1, produced);
      int good = 0, code = 0;
      for (; good < cnt; good++) {
        if (res[good].status) { code = res[good].status; break; }
        if (res[good].length > blockSize) { code = -KZ_ERR_PROCESS_BLOCK; break; }              // "incorrectly decompressed" (:756-759)
        if (at[good] + res[good].length > dstCap) { code = -KZ_ERR_WRITE_FILE; break; }
        at[good + 1] = at[good] + res[good].length;
      }
      // a failing block ends the stream, but the blocks in front of it are delivered first, as the unstaged path and the
      // reference's reader do: dst holds the same bytes on error whatever the batch size
      const int ncopy = code ? good : cnt;
      const int pieces = (ncopy + P - 1) / P;
      auto fetch = [&](int p) -> hipError_t {
        const int i0 = p * P, c = std::min(P, ncopy - i0);
        return hipMemcpyAsync(ctx->pinOut[p & 1].p, ctx->devOut[0].p + (size_t)i0 * blockSize, (size_t)c * blockSize, hipMemcpyDeviceToHost, ctx->copyDown);
      };
      if (pieces > 0) KZ_HIP(fetch(0));
      for (int p = 0; p < pieces; p++) {
        KZ_HIP(hipStreamSynchronize(ctx->copyDown));
        if (p + 1 < pieces) KZ_HIP(fetch(p + 1));                       // the next piece travels while this one is put in place
        const int i0 = p * P, c = std::min(P, ncopy - i0);
        const uint8_t* ring = ctx->pinOut[p & 1].p;
        parallel_blocks(c * 4, [&](int q) {                             // four copies per block
          const int i = i0 + (q >> 2);
          const int64_t len = res[i].length, a = (len * (q & 3)) >> 2, b = (len * ((q & 3) + 1)) >> 2;
          if (b > a) memcpy(dst + at[i] + a, ring + (size_t)(i - i0) * blockSize + a, (size_t)(b - a));
        });
      }
      if (code) return code;
      produced = at[cnt];
      continue;
    }
    if (!inbuf) inbuf.reset(new uint8_t[(size_t)iS * NB]);
    parallel_blocks(cnt, [&](int i) { HostBitsIn t = bs; t.pos = starts[i]; t.error = false; t.getBytes(inbuf.get() + (size_t)i * iS, (uint64_t)bits[i]); });
    // decode into a temporary when the tail would overflow dst
    const int64_t room = dstCap - produced;
    if (room >= (int64_t)cnt * blockSize) {
      int rc = kz_decode_blocks(ctx, tt, (uint32_t)entropyType, blockSize, inbuf.get(), iS, bits.data(), cnt,
                                dst + produced, blockSize, res.data(), KZ_MEM_HOST);
      if (rc) return rc;
      const int64_t base = produced;
      for (int i = 0; i < cnt; i++) {
        if (res[i].status) return res[i].status;
        if (res[i].length > blockSize) return -KZ_ERR_PROCESS_BLOCK;                  // "incorrectly decompressed" (:756-759)
        // the reader appends whatever a block produced (:783-785): close up behind a short block (corrupted streams only)
        if (produced != base + (int64_t)i * blockSize && res[i].length > 0)
          memmove(dst + produced, dst + base + (int64_t)i * blockSize, (size_t)res[i].length);
        produced += res[i].length;
      }
    } else {
      std::vector<uint8_t> tmp((size_t)cnt * blockSize);
      int rc = kz_decode_blocks(ctx, tt, (uint32_t)entropyType, blockSize, inbuf.get(), iS, bits.data(), cnt,
                                tmp.data(), blockSize, res.data(), KZ_MEM_HOST);
      if (rc) return rc;
      for (int i = 0; i < cnt; i++) {
        if (res[i].status) return res[i].status;
        if (res[i].length > blockSize) return -KZ_ERR_PROCESS_BLOCK;
        if (produced + res[i].length > dstCap) return -KZ_ERR_WRITE_FILE;
        memcpy(dst + produced, tmp.data() + (size_t)i * blockSize, (size_t)res[i].length);
        produced += res[i].length;
      }
    }
  }
  return pending ? pending : produced;
}

extern "C" int64_t kz_decompress(kz_ctx* ctx, const uint8_t* src, int64_t n, uint8_t* dst, int64_t dstCap) {
  if (!ctx || !src || !dst || n < 0) return -KZ_ERR_INVALID_PARAM;
  return decompress_host(ctx, src, n, 0, -1, dst, dstCap);
}
extern "C" int64_t kz_decompress_range(kz_ctx* ctx, const uint8_t* src, int64_t n, int64_t firstBlock, int64_t nBlocks, uint8_t* dst, int64_t dstCap) {
  if (!ctx || !src || !dst || n < 0 || firstBlock < 0 || nBlocks < 0) return -KZ_ERR_INVALID_PARAM;
  return decompress_host(ctx, src, n, firstBlock, nBlocks, dst, dstCap);
}


// =================================================================================================
// whole .knz stream on device memory: the same container, written and read with source and destination in HBM.  The kernels are in
// kz_knz_gpu.hip; what stays here is what kz_compress / kz_decompress do on the host as well and costs nothing: the stream header
// (write_stream_header / read_stream_header on a copy of at most 26 bytes), the bit-offset arithmetic over results[] (host arrays
// anyway), and precheck_block_header on the 8 header bytes per block that the walk kernel brings back.
namespace {
// per-chunk tables, pinned and their HBM mirror: 64 bytes (the stream header resp. the walk's result), then the entries
int knz_tables(kz_ctx* ctx, size_t entries, size_t entryBytes) {
  const size_t need = 64 + entries * entryBytes;
  int rc = stage_reserve(ctx, ctx->knzPin, need, true);
  if (!rc) rc = stage_reserve(ctx, ctx->knzAux, need, false);
  return rc;
}
// The rows' streams (W[i] bits each, rows `stride` apart, W[i] <= 0: no block) go behind bit `pos` of d_dst, then tailBits zero bits;
// pos moves behind them.  -KZ_ERR_WRITE_FILE, nothing launched, when that does not fit in dstCap bytes.
int knz_pack_rows(kz_ctx* ctx, const uint8_t* d_rows, int64_t stride, const int64_t* W, int cnt, uint8_t* d_dst, int64_t dstCap, int64_t& pos, int tailBits) {
  KnzBlk* t = (KnzBlk*)(ctx->knzPin.p + 64);
  int m = 0;
  int64_t p = pos;
  for (int i = 0; i < cnt; i++) {
    if (W[i] <= 0) continue;
    const int lw = ((uint64_t)W[i] < 8) ? 3 : ilog2((uint32_t)((uint64_t)W[i] >> 3)) + 4;    // write_block
    p += 5 + lw;
    t[m++] = KnzBlk{p, W[i], (int64_t)i * stride};
    p += W[i];
  }
  const int64_t end = p + tailBits;
  if (((end + 7) >> 3) > dstCap) return -KZ_ERR_WRITE_FILE;
  if (m) KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, t, (size_t)m * sizeof(KnzBlk), hipMemcpyHostToDevice, ctx->stream));
  const int rc = kz_knz_pack(ctx, d_rows, (const KnzBlk*)(ctx->knzAux.p + 64), m, d_dst, pos, end);
  pos = end;
  return rc;
}
// the stream header goes up from the front of the pinned table; the caller waits for the stream before it returns
int knz_put_header(kz_ctx* ctx, const uint8_t* hdr, int64_t hdrBytes, uint8_t* d_dst) {
  memcpy(ctx->knzPin.p, hdr, (size_t)hdrBytes);
  KZ_HIP(hipMemcpyAsync(d_dst, ctx->knzPin.p, (size_t)hdrBytes, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}
int knz_get_header(kz_ctx* ctx, const uint8_t* d_src, int64_t n, uint8_t* hdr /*32*/, int64_t& hn) {
  memset(hdr, 0, 32);
  hn = std::min<int64_t>(n, 26);                                 // the longest header: 160 + 48 bits
  if (hn > 0) {
    KZ_HIP(hipMemcpyAsync(hdr, d_src, (size_t)hn, hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  }
  return 0;
}
int knz_chunk_blocks(const kz_ctx* ctx, int blockSize) { return std::min(stream_chunk_blocks(ctx, blockSize), KZ_MAX_BATCH); }
}  // namespace

extern "C" int64_t kz_knz_assemble_device(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                                          int32_t checksumBits, const uint8_t* d_streams, int64_t stride, const int64_t* bits, int32_t nBlocks,
                                          uint8_t* d_dst, int64_t dstCap) {
  if (!ctx || !d_dst || nBlocks < 0 || (nBlocks > 0 && (!d_streams || !bits))) return -KZ_ERR_INVALID_PARAM;
  if (checksumBits != 0 && checksumBits != 32 && checksumBits != 64) return -KZ_ERR_INVALID_PARAM;
  KZ_HIP(hipSetDevice(ctx->device));
  uint8_t hdr[32];
  HostBits hb{hdr, 32, 0, false};
  write_stream_header(hb, transformType, entropyType, blockSize, inputSize, checksumBits == 32 ? 1 : (checksumBits == 64 ? 2 : 0));
  { const int rc = knz_tables(ctx, (size_t)std::max(nBlocks, 1), sizeof(KnzBlk)); if (rc) return rc; }
  int64_t pos = (int64_t)hb.pos;                                // (a whole number of bytes: 160 + 16 k bits)
  const int rc = knz_pack_rows(ctx, d_streams, stride, bits, nBlocks, d_dst, dstCap, pos, 8);   // end marker (:491-492)
  if (rc) return rc;
  { const int hrc = knz_put_header(ctx, hdr, (int64_t)(hb.pos >> 3), d_dst); if (hrc) return hrc; }
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  return (pos + 7) >> 3;
}

extern "C" int64_t kz_compress_device(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                                      const uint8_t* d_src, int64_t n, uint8_t* d_dst, int64_t dstCap) {
  if (!ctx || !d_src || !d_dst || n < 0) return -KZ_ERR_INVALID_PARAM;
  if (blockSize < 1024 || blockSize > (1 << 30) || (blockSize & 15)) return -KZ_ERR_BLOCK_SIZE;   // :165-174
  KZ_HIP(hipSetDevice(ctx->device));
  uint8_t hdr[32];
  HostBits hb{hdr, 32, 0, false};
  write_stream_header(hb, transformType, entropyType, blockSize, n, ctx->checksum);
  const int64_t nblocks = (n + blockSize - 1) / blockSize;
  BlockSizeScope scope(ctx, blockSize);
  const int CH = (int)std::min<int64_t>(knz_chunk_blocks(ctx, blockSize), std::max<int64_t>(nblocks, 1));
  const int64_t oS = kz_max_block_stream_bytes(blockSize);
  {
    int rc = stage_reserve(ctx, ctx->devOut[0], (size_t)CH * oS, false);
    if (!rc) rc = knz_tables(ctx, (size_t)CH, sizeof(KnzBlk));
    if (rc) return rc;
  }
  auto tooSmall = [&]() { snprintf(ctx->err, sizeof(ctx->err), "kz_compress_device: destination too small"); return (int64_t)-KZ_ERR_WRITE_FILE; };
  uint8_t* rows = ctx->devOut[0].p;
  std::vector<int32_t> lens(CH);
  std::vector<kz_block_result> res(CH);
  std::vector<int64_t> W(CH);
  int64_t pos = (int64_t)hb.pos;
  // ---- chunks, one after the other: encode HBM -> HBM rows, pack the rows behind the previous chunk's last bit ----
  for (int64_t b0 = 0; b0 < nblocks; b0 += CH) {
    const int cnt = (int)std::min<int64_t>(CH, nblocks - b0);
    for (int i = 0; i < cnt; i++) lens[i] = (int32_t)std::min<int64_t>(blockSize, n - (b0 + i) * blockSize);
    // a device row may be read up to the call's longest block whatever its own length is (kz_encode_blocks's contract), and behind
    // the stream's last, short block lies memory that is not the caller's: that block goes in a call of its own
    const int full = lens[cnt - 1] < blockSize ? cnt - 1 : cnt;
    int rc = 0;
    if (full) rc = kz_encode_blocks_pre(ctx, transformType, entropyType, blockSize, d_src + b0 * blockSize, blockSize, lens.data(), full,
                                        rows, oS, res.data(), KZ_MEM_DEVICE, nullptr);
    if (!rc && full < cnt) rc = kz_encode_blocks_pre(ctx, transformType, entropyType, blockSize, d_src + (b0 + full) * blockSize, blockSize, lens.data() + full, 1,
                                                     rows + (int64_t)full * oS, oS, res.data() + full, KZ_MEM_DEVICE, nullptr);
    if (rc) return rc;
    for (int i = 0; i < cnt; i++) { if (res[i].status) return res[i].status; W[i] = res[i].bits; }
    rc = knz_pack_rows(ctx, rows, oS, W.data(), cnt, d_dst, dstCap, pos, b0 + cnt >= nblocks ? 8 : 0);   // the last chunk: end marker (:491-492)
    if (rc == -KZ_ERR_WRITE_FILE) return tooSmall();
    if (rc) return rc;
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));                    // the rows and the pinned table are the next chunk's
    kz_ktimer_flush(ctx);
  }
  if (nblocks == 0) {
    const int rc = knz_pack_rows(ctx, rows, oS, W.data(), 0, d_dst, dstCap, pos, 8);
    if (rc == -KZ_ERR_WRITE_FILE) return tooSmall();
    if (rc) return rc;
  }
  { const int hrc = knz_put_header(ctx, hdr, (int64_t)(hb.pos >> 3), d_dst); if (hrc) return hrc; }
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  return (pos + 7) >> 3;
}

// the walk's tables: result at the front, then off[CH], bits[CH], hdr[CH]
namespace {
struct KnzWalk {
  int64_t* res; int64_t* off; int64_t* bits; uint64_t* hdr;         // host (pinned) views
  int64_t* d_res; int64_t* d_off; int64_t* d_bits; uint64_t* d_hdr;
  int cap;
  void bind(kz_ctx* ctx, int CH) {
    cap = CH;
    res = (int64_t*)ctx->knzPin.p; off = (int64_t*)(ctx->knzPin.p + 64); bits = off + CH; hdr = (uint64_t*)(bits + CH);
    d_res = (int64_t*)ctx->knzAux.p; d_off = (int64_t*)(ctx->knzAux.p + 64); d_bits = d_off + CH; d_hdr = (uint64_t*)(d_bits + CH);
  }
};
// walk up to maxCount (<= T.cap) prefixes from bit pos and bring the tables back (arrays = 2: offsets and lengths, 3: the header bytes as well)
int knz_walk_chunk(kz_ctx* ctx, KnzWalk& T, const uint8_t* d_src, int64_t n, int64_t pos, int maxCount, int arrays) {
  const int CH = maxCount;
  { const int rc = kz_knz_walk(ctx, d_src, n, pos, maxCount, T.d_off, T.d_bits, T.d_hdr, T.d_res); if (rc) return rc; }
  KZ_HIP(hipMemcpyAsync(ctx->knzPin.p, ctx->knzAux.p, 64 + (size_t)arrays * T.cap * 8, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  if (T.res[0] < 0 || T.res[0] > CH) { snprintf(ctx->err, sizeof(ctx->err), "knz walk: bad count"); return -KZ_ERR_DEVICE; }
  return 0;
}
}  // namespace

extern "C" int32_t kz_knz_index_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, uint64_t* transformType, uint32_t* entropyType,
                                       int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits, int64_t* blockBitOff, int64_t* blockBits, int32_t cap) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  if (!d_src || n < 20) return -KZ_ERR_INVALID_FILE;
  KZ_HIP(hipSetDevice(ctx->device));
  uint8_t hdr[32]; int64_t hn = 0;
  { const int rc = knz_get_header(ctx, d_src, n, hdr, hn); if (rc) return rc; }
  HostBitsIn bs{hdr, (uint64_t)hn * 8, 0, false};
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, nullptr, 0); if (hrc) return hrc; }
  if (transformType) *transformType = h.transformType;
  if (entropyType) *entropyType = (uint32_t)h.entropyType;
  if (blockSize) *blockSize = h.blockSize;
  if (inputSize) *inputSize = h.inputSize;
  if (checksumBits) *checksumBits = h.chkKind == 1 ? 32 : (h.chkKind == 2 ? 64 : 0);
  const int CH = (int)std::min<int64_t>(16384, n / 8 + 16);
  { const int rc = knz_tables(ctx, (size_t)CH, 24); if (rc) return rc; }
  KnzWalk T; T.bind(ctx, CH);
  int64_t pos = (int64_t)bs.pos, nb = 0;
  for (;;) {
    { const int rc = knz_walk_chunk(ctx, T, d_src, n, pos, CH, 2); if (rc) return rc; }
    const int got = (int)T.res[0], why = (int)T.res[2];
    const int have = got + (why == KNZ_WALK_PAYLOAD ? 1 : 0);       // kz_knz_index records a block before it looks at its end
    for (int i = 0; i < have; i++, nb++)
      if (nb < cap) { if (blockBitOff) blockBitOff[nb] = T.off[i]; if (blockBits) blockBits[nb] = T.bits[i]; }
    if (why == KNZ_WALK_PREFIX || why == KNZ_WALK_PAYLOAD) return -KZ_ERR_READ_FILE;
    if (why == KNZ_WALK_END) break;
    pos = T.res[1];
    if (nb > 0x7FFFFFFF - CH) return -KZ_ERR_INVALID_FILE;
  }
  return (int32_t)nb;
}

namespace {
// kz_decompress's checks on one walked block, in kz_decompress's order: the block header (from the 8 bytes the device brought back), the
// staging-row bound, the end of the stream
int knz_precheck_entry(uint64_t hdr, uint64_t rd, uint64_t at, uint64_t nbits, int nbFunctions, int blockSize, int chkKind, int64_t iS) {
  uint8_t hb8[8];
  for (int k = 0; k < 8; k++) hb8[k] = (uint8_t)(hdr >> (56 - 8 * k));
  HostBitsIn t{hb8, std::min<uint64_t>(64, nbits - at), 0, false};             // the header is 7 bytes at the most
  int rc = precheck_block_header(t, rd, nbFunctions, blockSize, chkKind);
  if (!rc && (int64_t)((rd + 7) >> 3) > iS - 64) rc = -KZ_ERR_BLOCK_SIZE;
  if (!rc && at + rd > nbits) rc = -KZ_ERR_READ_FILE;
  return rc;
}
}  // namespace

// kz_decompress_device and kz_decompress_range_device: decompress_host's contract, source and destination in HBM
static int64_t decompress_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, int64_t firstBlock, int64_t nBlocks, uint8_t* d_dst, int64_t dstCap) {
  KZ_HIP(hipSetDevice(ctx->device));
  uint8_t hdr[32]; int64_t hn = 0;
  { const int rc = knz_get_header(ctx, d_src, n, hdr, hn); if (rc) return rc; }
  HostBitsIn bs{hdr, (uint64_t)hn * 8, 0, false};
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, ctx->err, sizeof(ctx->err)); if (hrc) return hrc; }
  const int chkKind = h.chkKind, entropyType = h.entropyType, blockSize = h.blockSize;
  const uint64_t tt = h.transformType;
  const int savedChk = ctx->checksum;
  ctx->checksum = chkKind;
  struct Restore { kz_ctx* c; int v; ~Restore() { c->checksum = v; } } restore_{ctx, savedChk};
  int nbFunctions = 0;
  for (int i = 0; i < 8; i++) if (((tt >> (42 - 6 * i)) & 0x3F) != 0) nbFunctions++;         // Sequence length (TransformFactory.java:240-266)
  if (nbFunctions == 0) nbFunctions = 1;
  const uint64_t nbits = (uint64_t)n * 8;
  // kz_decompress's own batch: 8 GiB of blocks, 2048 at the most, and no more than the stream can need (declared size if present,
  // else >= 8 bytes of stream per block).  The decoder's serial per-block chains want that many blocks in flight: in chunks of the
  // writer's size (about 1 GiB) a 2048 x 4 MiB stream decodes at a quarter of the speed.  KZ_STREAM_CHUNK makes the
  // chunks smaller (the tests' seams); kz_decompress looks at the room left in dst once per batch of ITS size, so chunks never
  // straddle those batches and carry the batch's count of blocks that may still start inside dst: both calls cut a stream at the
  // same block.
  int64_t NB = batch_blocks(blockSize);
  if (h.szMask && h.inputSize > 0) NB = std::min<int64_t>(NB, (h.inputSize + blockSize - 1) / blockSize);
  else NB = std::min<int64_t>(NB, n / 8 + 1);
  const int CH = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->sw.streamChunk > 0 ? ctx->sw.streamChunk : NB, std::min<int64_t>(NB, KZ_MAX_BATCH)));
  const int64_t iS = (int64_t)kz_align((size_t)blockSize + (size_t)(blockSize >> 3) + 1024 + 64, 256);
  if (nBlocks == 0) return 0;
  // blocks in front of the range are walked in the index call's chunks (the walk is all that happens to them), unless
  // KZ_STREAM_CHUNK says otherwise
  const int SK = firstBlock == 0 ? 0 : (ctx->sw.streamChunk > 0 ? CH : (int)std::min<int64_t>(16384, n / 8 + 16));
  { const int rc = knz_tables(ctx, (size_t)std::max(CH, SK), 24); if (rc) return rc; }
  KnzWalk T;
  int64_t pos = (int64_t)bs.pos, produced = 0;
  if (SK) T.bind(ctx, SK);
  for (int64_t k = 0; k < firstBlock;) {                         // read and skipped: prefix and block header, not the payload
    { const int rc = knz_walk_chunk(ctx, T, d_src, n, pos, (int)std::min<int64_t>(SK, firstBlock - k), 3); if (rc) return rc; }
    const int why = (int)T.res[2];
    const int have = (int)T.res[0] + (why == KNZ_WALK_PAYLOAD ? 1 : 0);
    for (int i = 0; i < have; i++) {
      const int rc = knz_precheck_entry(T.hdr[i], (uint64_t)T.bits[i], (uint64_t)T.off[i], nbits, nbFunctions, blockSize, chkKind, iS);
      if (rc) return rc;
    }
    if (why == KNZ_WALK_PREFIX) return -KZ_ERR_READ_FILE;
    if (why == KNZ_WALK_END) return 0;                            // the end marker in front of the range
    pos = T.res[1];
    k += have;
  }
  T.bind(ctx, CH);
  std::vector<kz_block_result> res(CH);
  bool done = false;
  int pending = 0;
  int64_t batchLeft = 0, fitLeft = 0;
  int64_t left = nBlocks < 0 ? INT64_MAX : nBlocks;               // blocks of the range not walked yet
  while (!done) {
    if (left == 0) break;                                         // the end of the range: nothing behind it is read
    if (batchLeft == 0) {
      batchLeft = NB;
      const int64_t room = dstCap - produced;
      fitLeft = (room <= 0) ? 0 : (room + blockSize - 1) / blockSize;
    }
    const int want = (int)std::min<int64_t>(std::min<int64_t>(CH, batchLeft), left);
    // ---- the walk on the device, then kz_decompress's checks in kz_decompress's order on what it recorded.  A fault met here is
    //      held back until the blocks before it have been decoded: the reference reports the FIRST failing block in stream order ----
    { const int rc = knz_walk_chunk(ctx, T, d_src, n, pos, want, 3); if (rc) return rc; }
    const int why = (int)T.res[2];
    const int have = (int)T.res[0] + (why == KNZ_WALK_PAYLOAD ? 1 : 0);
    pos = T.res[1];
    int cnt = 0;
    for (; cnt < have; cnt++) {
      pending = knz_precheck_entry(T.hdr[cnt], (uint64_t)T.bits[cnt], (uint64_t)T.off[cnt], nbits, nbFunctions, blockSize, chkKind, iS);
      if (pending) break;
    }
    left -= cnt;
    if (!pending) { if (why == KNZ_WALK_PREFIX) pending = -KZ_ERR_READ_FILE; else if (why == KNZ_WALK_END) done = true; }
    if (pending) done = true;
    if (cnt == 0) break;
    // blocks that start past the end of the destination cannot be stored (kz_decompress)
    if (fitLeft < cnt) { cnt = (int)fitLeft; pending = -KZ_ERR_WRITE_FILE; done = true; }
    if (cnt == 0) break;
    fitLeft -= cnt; batchLeft -= cnt;
    int64_t maxBytes = 0;
    for (int i = 0; i < cnt; i++) maxBytes = std::max<int64_t>(maxBytes, (T.bits[i] + 7) >> 3);
    { const int rc = stage_reserve(ctx, ctx->devIn[0], (size_t)cnt * iS, false); if (rc) return rc; }   // (grow-only: the blocks walked, not the chunk's most)
    { const int rc = kz_knz_unpack(ctx, d_src, n, T.d_off, T.d_bits, cnt, maxBytes, ctx->devIn[0].p, iS); if (rc) return rc; }
    // ---- blocks whose whole blockSize row lies inside what is left of dst are decoded in place; the others (as a rule the last
    //      block of a destination of the exact size) into staging rows ----
    const int nd = (int)std::min<int64_t>(cnt, (dstCap - produced) / blockSize);
    if (cnt > nd) { const int rc = stage_reserve(ctx, ctx->devOut[0], (size_t)(cnt - nd) * blockSize, false); if (rc) return rc; }
    int rc = 0;
    if (nd) rc = kz_decode_blocks(ctx, tt, (uint32_t)entropyType, blockSize, ctx->devIn[0].p, iS, T.bits, nd,
                                  d_dst + produced, blockSize, res.data(), KZ_MEM_DEVICE);
    if (!rc && cnt > nd) rc = kz_decode_blocks(ctx, tt, (uint32_t)entropyType, blockSize, ctx->devIn[0].p + (int64_t)nd * iS, iS, T.bits + nd, cnt - nd,
                                               ctx->devOut[0].p, blockSize, res.data() + nd, KZ_MEM_DEVICE);
    if (rc) return rc;
    // ---- the reader appends whatever a block produced (:783-785): a block behind a short one moves left, in stream order; the
    //      first failing block ends the stream, the blocks in front of it are delivered ----
    const int64_t base = produced;
    int code = 0;
    for (int i = 0; i < cnt; i++) {
      if (res[i].status) { code = res[i].status; break; }
      if (res[i].length > blockSize) { code = -KZ_ERR_PROCESS_BLOCK; break; }                    // "incorrectly decompressed" (:756-759)
      if (produced + res[i].length > dstCap) { code = -KZ_ERR_WRITE_FILE; break; }
      const int64_t len = res[i].length;
      const uint8_t* from = i < nd ? d_dst + base + (int64_t)i * blockSize : ctx->devOut[0].p + (int64_t)(i - nd) * blockSize;
      uint8_t* to = d_dst + produced;
      if (len > 0 && from != to) {
        if (i < nd && from - to < len) {                          // overlapping move: through the staging rows, which are done with
          KZ_HIP(hipMemcpyAsync(ctx->devIn[0].p, from, (size_t)len, hipMemcpyDeviceToDevice, ctx->stream));
          from = ctx->devIn[0].p;
        }
        KZ_HIP(hipMemcpyAsync(to, from, (size_t)len, hipMemcpyDeviceToDevice, ctx->stream));
      }
      produced += len;
    }
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
    if (code) return code;
  }
  return pending ? pending : produced;
}

extern "C" int64_t kz_decompress_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, uint8_t* d_dst, int64_t dstCap) {
  if (!ctx || !d_src || !d_dst || n < 0) return -KZ_ERR_INVALID_PARAM;
  return decompress_device(ctx, d_src, n, 0, -1, d_dst, dstCap);
}
extern "C" int64_t kz_decompress_range_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, int64_t firstBlock, int64_t nBlocks, uint8_t* d_dst, int64_t dstCap) {
  if (!ctx || !d_src || !d_dst || n < 0 || firstBlock < 0 || nBlocks < 0) return -KZ_ERR_INVALID_PARAM;
  return decompress_device(ctx, d_src, n, firstBlock, nBlocks, d_dst, dstCap);
}


// =================================================================================================
// many .knz streams on device memory: kz_compress_device / kz_decompress_device for N (segment, slot) pairs in one call.  Whole
// streams are collected into groups of at most one chunk's blocks; the blocks of a group go through ONE batched encode (one decode
// per distinct header), and the container kernels (kz_knz_gpu.hip: gather, pack, heads, walk, unpack, scatter) take a table with an
// entry per segment, slot or row, so launches and host waits per group do not grow with the streams in it.  A stream with more
// blocks than a group takes goes through the single-stream call, which is the definition of every result here.
namespace {
// `need` bytes of pinned table and of its HBM mirror (the single-stream calls use the same two buffers: nothing is kept in them
// across one of those calls)
int knz_many_tables(kz_ctx* ctx, size_t need) {
  int rc = stage_reserve(ctx, ctx->knzPin, need + 64, true);
  if (!rc) rc = stage_reserve(ctx, ctx->knzAux, need + 64, false);
  return rc;
}
int knz_many_args(const void* ctx, const void* d_src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams,
                  const void* d_dst, const int64_t* dstOff, const int64_t* dstCap, const int64_t* dstLen) {
  if (!ctx || nStreams < 0) return -KZ_ERR_INVALID_PARAM;
  if (nStreams == 0) return 0;
  if (!d_src || !srcOff || !srcLen || !d_dst || !dstOff || !dstCap || !dstLen) return -KZ_ERR_INVALID_PARAM;
  for (int s = 0; s < nStreams; s++) if (srcOff[s] < 0 || srcLen[s] < 0 || dstOff[s] < 0 || dstCap[s] < 0) return -KZ_ERR_INVALID_PARAM;
  return 0;
}
inline int64_t knz_units16(const uint8_t* p, int64_t len) {        // 16-byte aligned units of memory that [p, p + len) touches
  const uintptr_t a = (uintptr_t)p;
  return (int64_t)((((a + (uintptr_t)len + 15) & ~(uintptr_t)15) - (a & ~(uintptr_t)15)) >> 4);
}

// streams [s0, s1) of a kz_compress_many_device call: together at most one chunk's blocks
int compress_group(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize, const uint8_t* d_src, const int64_t* srcOff,
                   const int64_t* srcLen, int s0, int s1, uint8_t* d_dst, const int64_t* dstOff, const int64_t* dstCap, int64_t* dstLen) {
  const int ns = s1 - s0;
  int64_t nbTot = 0;
  for (int s = s0; s < s1; s++) nbTot += (srcLen[s] + blockSize - 1) / blockSize;
  const int NBk = (int)nbTot;
  const int64_t oS = kz_max_block_stream_bytes(blockSize);
  const size_t gatherBytes = kz_align((size_t)NBk * sizeof(KnzCopy) + 64, 64), segBytes = (size_t)ns * sizeof(KnzSeg);
  {
    int rc = stage_reserve(ctx, ctx->devIn[0], (size_t)std::max(NBk, 1) * (size_t)blockSize, false);
    if (!rc) rc = stage_reserve(ctx, ctx->devOut[0], (size_t)std::max(NBk, 1) * (size_t)oS, false);
    if (!rc) rc = knz_many_tables(ctx, gatherBytes + segBytes + (size_t)NBk * sizeof(KnzBlk));
    if (rc) return rc;
  }
  uint8_t* rowsIn = ctx->devIn[0].p;
  uint8_t* rows = ctx->devOut[0].p;
  std::vector<int32_t> lens(NBk);
  std::vector<kz_block_result> res(NBk);
  int erc = 0;
  if (NBk) {
    // ---- gather: every block into a row of its own, blockSize apart (the encoder may read a device row up to the call's longest
    //      block, and behind a stream's last block lies memory that is not that stream's) ----
    KnzCopy* g = (KnzCopy*)ctx->knzPin.p;
    int r = 0;
    for (int s = s0; s < s1; s++)
      for (int64_t o = 0; o < srcLen[s]; o += blockSize, r++) {
        lens[r] = (int32_t)std::min<int64_t>(blockSize, srcLen[s] - o);
        g[r] = KnzCopy{srcOff[s] + o, (int64_t)r * blockSize, lens[r]};
      }
    KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, g, (size_t)NBk * sizeof(KnzCopy), hipMemcpyHostToDevice, ctx->stream));
    { const int rc = kz_knz_gather(ctx, d_src, (const KnzCopy*)ctx->knzAux.p, NBk, blockSize, rowsIn); if (rc) return rc; }
    // the encoder takes device input to be complete when it is called: chains led by TEXT / UTF copy rows back on another stream
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
    BlockSizeScope scope(ctx, blockSize);
    erc = kz_encode_blocks_pre(ctx, transformType, entropyType, blockSize, rowsIn, blockSize, lens.data(), NBk, rows, oS, res.data(), KZ_MEM_DEVICE, nullptr);
    if (erc == -KZ_ERR_DEVICE) return erc;
  }
  // ---- per stream what kz_compress_device does per stream: header, bit offsets over results[], the fit in the slot ----
  KnzSeg* seg = (KnzSeg*)(ctx->knzPin.p + gatherBytes);
  KnzBlk* blk = (KnzBlk*)(ctx->knzPin.p + gatherBytes + segBytes);
  int m = 0, nseg = 0, r0 = 0;
  int64_t units = 0;
  for (int s = s0; s < s1; s++) {
    const int nb = (int)((srcLen[s] + blockSize - 1) / blockSize);
    const int first = r0;
    r0 += nb;
    int64_t code = nb ? erc : 0;                                  // (an empty stream asks nothing of the encoder)
    for (int i = 0; i < nb && !code; i++) code = res[first + i].status;
    if (code) { dstLen[s] = code; continue; }
    KnzSeg S;
    memset(&S, 0, sizeof(S));
    uint8_t hdr[32] = {0};
    HostBits hb{hdr, 32, 0, false};
    write_stream_header(hb, transformType, entropyType, blockSize, srcLen[s], ctx->checksum);
    int64_t p = (int64_t)hb.pos;
    const int m0 = m;
    for (int i = 0; i < nb; i++) {
      const int64_t W = res[first + i].bits;
      if (W <= 0) continue;
      const int lw = ((uint64_t)W < 8) ? 3 : ilog2((uint32_t)((uint64_t)W >> 3)) + 4;          // write_block
      p += 5 + lw;
      blk[m++] = KnzBlk{p, W, (int64_t)(first + i) * oS};
      p += W;
    }
    const int64_t end = p + 8;                                    // end marker (:491-492)
    if (((end + 7) >> 3) > dstCap[s]) {
      m = m0;
      snprintf(ctx->err, sizeof(ctx->err), "kz_compress_many_device: destination %d too small", s);
      dstLen[s] = -KZ_ERR_WRITE_FILE;
      continue;
    }
    S.dst = dstOff[s]; S.endBit = end; S.unit0 = units; S.blk0 = m0; S.nblk = m - m0; S.hdrBytes = (int32_t)(hb.pos >> 3);
    memcpy(S.hdr, hdr, 28);
    seg[nseg++] = S;
    units += knz_units16(d_dst + dstOff[s], (end + 7) >> 3);
    dstLen[s] = (end + 7) >> 3;
  }
  if (nseg) {
    uint8_t* a = ctx->knzAux.p + gatherBytes;
    KZ_HIP(hipMemcpyAsync(a, seg, segBytes + (size_t)m * sizeof(KnzBlk), hipMemcpyHostToDevice, ctx->stream));
    const int rc = kz_knz_pack_many(ctx, rows, (const KnzSeg*)a, nseg, (const KnzBlk*)(a + segBytes), d_dst, units);
    if (rc) return rc;
  }
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  return 0;
}
}  // namespace

extern "C" int64_t kz_compress_many_bound(const int64_t* srcLen, int32_t nStreams, int32_t blockSize) {
  if (nStreams < 0 || (nStreams > 0 && !srcLen)) return -KZ_ERR_INVALID_PARAM;
  int64_t total = 0;
  for (int s = 0; s < nStreams; s++) {
    const int64_t b = kz_compress_bound(srcLen[s], blockSize);
    if (b < 0) return b;
    total += b;
  }
  return total;
}

extern "C" int32_t kz_compress_many_device(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize,
                                           const uint8_t* d_src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams,
                                           uint8_t* d_dst, const int64_t* dstOff, const int64_t* dstCap, int64_t* dstLen) {
  { const int rc = knz_many_args(ctx, d_src, srcOff, srcLen, nStreams, d_dst, dstOff, dstCap, dstLen); if (rc || nStreams == 0) return rc; }
  if (blockSize < 1024 || blockSize > (1 << 30) || (blockSize & 15)) return -KZ_ERR_BLOCK_SIZE;   // kz_compress_device's check
  KZ_HIP(hipSetDevice(ctx->device));
  const int64_t G = knz_chunk_blocks(ctx, blockSize);
  auto blocksOf = [&](int s) { return (srcLen[s] + blockSize - 1) / blockSize; };
  for (int s0 = 0; s0 < nStreams;) {
    if (blocksOf(s0) > G) {                                       // larger than a group: the single-stream call, on its own
      dstLen[s0] = kz_compress_device(ctx, transformType, entropyType, blockSize, d_src + srcOff[s0], srcLen[s0], d_dst + dstOff[s0], dstCap[s0]);
      if (dstLen[s0] == -KZ_ERR_DEVICE) return -KZ_ERR_DEVICE;
      s0++;
      continue;
    }
    int s1 = s0;
    int64_t tot = 0;                                              // (an empty stream counts as one block: a group's tables stay bounded)
    while (s1 < nStreams && blocksOf(s1) <= G && (s1 == s0 || tot + std::max<int64_t>(blocksOf(s1), 1) <= G)) { tot += std::max<int64_t>(blocksOf(s1), 1); s1++; }
    const int rc = compress_group(ctx, transformType, entropyType, blockSize, d_src, srcOff, srcLen, s0, s1, d_dst, dstOff, dstCap, dstLen);
    if (rc) return rc;
    s0 = s1;
  }
  return 0;
}

namespace {
struct KnzManyStream {                                             // a stream of a kz_decompress_many_device call after the header parse
  KnzHeader h; int code; int64_t startBit; int nbFunctions; int CH; int64_t iS;
  int cnt, why;                                                    // the count pass
};
// the streams ids[0 .. ng) of a kz_decompress_many_device call: their walk stops inside a single-stream chunk, and together they
// hold at most a group's blocks (have[k] entries each, the one of a payload that does not fit included)
int decompress_group(kz_ctx* ctx, const std::vector<KnzManyStream>& st, const int* ids, const int* have, int ng, const uint8_t* d_src, const int64_t* srcOff,
                     const int64_t* srcLen, uint8_t* d_dst, const int64_t* dstOff, const int64_t* dstCap, int64_t* dstLen) {
  int64_t E = 0;
  for (int k = 0; k < ng; k++) E += have[k];
  // ---- fill pass: the entries of all streams in one table, at the exclusive scan of the counts ----
  const size_t tBytes = kz_align((size_t)ng * sizeof(KnzSrc), 64), outBytes = (size_t)ng * 24 + (size_t)E * 24;
  { const int rc = knz_many_tables(ctx, tBytes + outBytes); if (rc) return rc; }
  {
    KnzSrc* t = (KnzSrc*)ctx->knzPin.p;
    int64_t base = 0;
    for (int k = 0; k < ng; k++) {
      const int s = ids[k];
      t[k] = KnzSrc{srcOff[s], srcLen[s], st[s].startBit, base, st[s].CH + 1, have[k]};
      base += have[k];
    }
  }
  int64_t* d_res = (int64_t*)(ctx->knzAux.p + tBytes);
  int64_t* d_off = d_res + 3 * (int64_t)ng;
  const int64_t* res = (const int64_t*)(ctx->knzPin.p + tBytes);
  const int64_t* off = res + 3 * (int64_t)ng;
  const int64_t* bits = off + E;
  const uint64_t* hdr = (const uint64_t*)(bits + E);
  KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, ctx->knzPin.p, (size_t)ng * sizeof(KnzSrc), hipMemcpyHostToDevice, ctx->stream));
  { const int rc = kz_knz_walk_many(ctx, d_src, (const KnzSrc*)ctx->knzAux.p, ng, d_off, d_off + E, (uint64_t*)(d_off + 2 * E), d_res); if (rc) return rc; }
  KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + tBytes, ctx->knzAux.p + tBytes, outBytes, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  // ---- per stream kz_decompress_device's checks on its one chunk, in its order; a fault is held back behind the blocks in front ----
  struct Part { int s, first, cnt, pending, cls; int64_t base; };
  struct Cls { uint64_t tt; int et, bs, chk; int64_t iS; int rows; int64_t inBase, outBase; int first; };
  std::vector<Part> parts(ng);
  std::vector<Cls> cls;
  int64_t base = 0;
  for (int k = 0; k < ng; k++) {
    const int s = ids[k];
    const KnzManyStream& S = st[s];
    const int64_t got = res[3 * k], why = res[3 * k + 2];
    if (got < 0 || got > S.CH + 1) { snprintf(ctx->err, sizeof(ctx->err), "knz walk: bad count"); return -KZ_ERR_DEVICE; }
    const int hv = (int)std::min<int64_t>(got + (why == KNZ_WALK_PAYLOAD ? 1 : 0), have[k]);
    const uint64_t nbits = (uint64_t)srcLen[s] * 8;
    int cnt = 0, pending = 0;
    for (; cnt < hv; cnt++) {
      pending = knz_precheck_entry(hdr[base + cnt], (uint64_t)bits[base + cnt], (uint64_t)off[base + cnt], nbits, S.nbFunctions, S.h.blockSize, S.h.chkKind, S.iS);
      if (pending) break;
    }
    if (!pending && why != KNZ_WALK_END) pending = -KZ_ERR_READ_FILE;     // a prefix that does not fit
    if (cnt > 0) {                                                // blocks that start past the end of the destination cannot be stored
      const int64_t fit = dstCap[s] <= 0 ? 0 : (dstCap[s] + S.h.blockSize - 1) / S.h.blockSize;
      if (fit < cnt) { cnt = (int)fit; pending = -KZ_ERR_WRITE_FILE; }
    }
    int c = 0;
    for (; c < (int)cls.size(); c++) if (cls[c].tt == S.h.transformType && cls[c].et == S.h.entropyType && cls[c].bs == S.h.blockSize && cls[c].chk == S.h.chkKind) break;
    if (c == (int)cls.size()) cls.push_back(Cls{S.h.transformType, S.h.entropyType, S.h.blockSize, S.h.chkKind, S.iS, 0, 0, 0, 0});
    parts[k] = Part{s, cls[c].rows, cnt, pending, c, base};
    cls[c].rows += cnt;
    base += have[k];
  }
  int64_t inBytes = 0, outBytes2 = 0;
  int R = 0;
  for (Cls& c : cls) { c.inBase = inBytes; c.outBase = outBytes2; c.first = R; inBytes += (int64_t)c.rows * c.iS; outBytes2 += (int64_t)c.rows * c.bs; R += c.rows; }
  std::vector<int64_t> W((size_t)std::max(R, 1));
  std::vector<kz_block_result> bres((size_t)std::max(R, 1));
  // the walk's tables are read for the last time while the unpack table is built: it goes behind them
  const size_t rowBytes = kz_align((size_t)R * sizeof(KnzRow), 64), copyBytes = (size_t)R * sizeof(KnzCopy);
  std::vector<KnzRow> rowT((size_t)R);
  int64_t maxBytes = 0;
  for (int k = 0; k < ng; k++) {
    const Part& P = parts[k];
    const Cls& c = cls[P.cls];
    for (int i = 0; i < P.cnt; i++) {
      const int r = c.first + P.first + i;
      W[r] = bits[P.base + i];
      maxBytes = std::max<int64_t>(maxBytes, (W[r] + 7) >> 3);
      rowT[r] = KnzRow{srcOff[P.s], srcLen[P.s], off[P.base + i], W[r], c.inBase + (int64_t)(P.first + i) * c.iS};
    }
  }
  if (R) {
    int rc = stage_reserve(ctx, ctx->devIn[0], (size_t)inBytes + 64, false);
    if (!rc) rc = stage_reserve(ctx, ctx->devOut[0], (size_t)outBytes2 + 64, false);
    if (!rc) rc = knz_many_tables(ctx, rowBytes + copyBytes);     // (may move the tables: everything needed from them is in W / rowT / parts)
    if (rc) return rc;
    memcpy(ctx->knzPin.p, rowT.data(), (size_t)R * sizeof(KnzRow));
    KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, ctx->knzPin.p, (size_t)R * sizeof(KnzRow), hipMemcpyHostToDevice, ctx->stream));
    rc = kz_knz_unpack_many(ctx, d_src, (const KnzRow*)ctx->knzAux.p, R, maxBytes, ctx->devIn[0].p);
    if (rc) return rc;
  }
  // ---- one decode per distinct header, into staging rows ----
  std::vector<int> crc(cls.size(), 0);
  {
    const int savedChk = ctx->checksum;
    struct Restore { kz_ctx* c; int v; ~Restore() { c->checksum = v; } } restore_{ctx, savedChk};
    for (size_t c = 0; c < cls.size(); c++) {
      const Cls& C = cls[c];
      if (!C.rows) continue;
      ctx->checksum = C.chk;
      crc[c] = kz_decode_blocks(ctx, C.tt, (uint32_t)C.et, C.bs, ctx->devIn[0].p + C.inBase, C.iS, W.data() + C.first, C.rows,
                                ctx->devOut[0].p + C.outBase, C.bs, bres.data() + C.first, KZ_MEM_DEVICE);
      if (crc[c] == -KZ_ERR_DEVICE) return crc[c];
    }
  }
  // ---- scatter: each stream's blocks into its slot back to back, cut where kz_decompress_device cuts it ----
  KnzCopy* ct = R ? (KnzCopy*)(ctx->knzPin.p + rowBytes) : nullptr;
  int nc = 0;
  int64_t maxLen = 0;
  for (int k = 0; k < ng; k++) {
    const Part& P = parts[k];
    const Cls& C = cls[P.cls];
    if (P.cnt > 0 && crc[P.cls]) { dstLen[P.s] = crc[P.cls]; continue; }
    int64_t produced = 0;
    int code = 0;
    for (int i = 0; i < P.cnt; i++) {
      const kz_block_result& b = bres[C.first + P.first + i];
      if (b.status) { code = b.status; break; }
      if (b.length > C.bs) { code = -KZ_ERR_PROCESS_BLOCK; break; }
      if (produced + b.length > dstCap[P.s]) { code = -KZ_ERR_WRITE_FILE; break; }
      if (b.length > 0) {
        ct[nc++] = KnzCopy{C.outBase + (int64_t)(P.first + i) * C.bs, dstOff[P.s] + produced, b.length};
        maxLen = std::max<int64_t>(maxLen, b.length);
      }
      produced += b.length;
    }
    dstLen[P.s] = code ? code : (P.pending ? P.pending : produced);
  }
  if (nc) {
    KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + rowBytes, ct, (size_t)nc * sizeof(KnzCopy), hipMemcpyHostToDevice, ctx->stream));
    const int rc = kz_knz_scatter(ctx, ctx->devOut[0].p, (const KnzCopy*)(ctx->knzAux.p + rowBytes), nc, maxLen, d_dst);
    if (rc) return rc;
  }
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  return 0;
}
}  // namespace

extern "C" int32_t kz_decompress_many_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams,
                                             uint8_t* d_dst, const int64_t* dstOff, const int64_t* dstCap, int64_t* dstLen) {
  { const int rc = knz_many_args(ctx, d_src, srcOff, srcLen, nStreams, d_dst, dstOff, dstCap, dstLen); if (rc || nStreams == 0) return rc; }
  KZ_HIP(hipSetDevice(ctx->device));
  const int ns = nStreams;
  std::vector<KnzManyStream> st((size_t)ns);
  // ---- the first bytes of every stream in one table, one copy; the headers are parsed here with kz_decompress_device's codes ----
  const size_t tBytes = kz_align((size_t)ns * sizeof(KnzSrc), 64), headBytes = (size_t)ns * 32, resBytes = (size_t)ns * 24;
  { const int rc = knz_many_tables(ctx, tBytes + std::max(headBytes, resBytes)); if (rc) return rc; }
  KnzSrc* t = (KnzSrc*)ctx->knzPin.p;
  const KnzSrc* d_t = (const KnzSrc*)ctx->knzAux.p;
  for (int s = 0; s < ns; s++) t[s] = KnzSrc{srcOff[s], srcLen[s], 0, 0, 0, 0};
  KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, t, (size_t)ns * sizeof(KnzSrc), hipMemcpyHostToDevice, ctx->stream));
  { const int rc = kz_knz_heads(ctx, d_src, d_t, ns, ctx->knzAux.p + tBytes); if (rc) return rc; }
  KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + tBytes, ctx->knzAux.p + tBytes, headBytes, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  bool firstFault = true;
  for (int s = 0; s < ns; s++) {
    KnzManyStream& S = st[s];
    memset(&S, 0, sizeof(S));
    const int64_t n = srcLen[s], hn = std::min<int64_t>(n, 26);
    HostBitsIn bs{ctx->knzPin.p + tBytes + (size_t)s * 32, (uint64_t)hn * 8, 0, false};
    S.code = read_stream_header(bs, S.h, firstFault ? ctx->err : nullptr, sizeof(ctx->err));   // (the text of the first failing stream stays)
    if (S.code) { firstFault = false; t[s].maxCount = 0; continue; }
    const int blockSize = S.h.blockSize;
    for (int i = 0; i < 8; i++) if (((S.h.transformType >> (42 - 6 * i)) & 0x3F) != 0) S.nbFunctions++;
    if (S.nbFunctions == 0) S.nbFunctions = 1;
    int64_t NB = batch_blocks(blockSize);                         // decompress_device's batch and chunk
    if (S.h.szMask && S.h.inputSize > 0) NB = std::min<int64_t>(NB, (S.h.inputSize + blockSize - 1) / blockSize);
    else NB = std::min<int64_t>(NB, n / 8 + 1);
    S.CH = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->sw.streamChunk > 0 ? ctx->sw.streamChunk : NB, std::min<int64_t>(NB, KZ_MAX_BATCH)));
    S.iS = (int64_t)kz_align((size_t)blockSize + (size_t)(blockSize >> 3) + 1024 + 64, 256);
    S.startBit = (int64_t)bs.pos;
    t[s].startBit = S.startBit; t[s].maxCount = S.CH + 1;
  }
  // ---- count pass: one lane per stream walks one block further than a single-stream chunk goes.  A walk that stops by itself
  //      (end marker or fault) is what kz_decompress_device sees in its one chunk with blocks: such a stream can join a group ----
  KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, t, (size_t)ns * sizeof(KnzSrc), hipMemcpyHostToDevice, ctx->stream));
  { const int rc = kz_knz_walk_many(ctx, d_src, d_t, ns, nullptr, nullptr, nullptr, (int64_t*)(ctx->knzAux.p + tBytes)); if (rc) return rc; }
  KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + tBytes, ctx->knzAux.p + tBytes, resBytes, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  {
    const int64_t* res = (const int64_t*)(ctx->knzPin.p + tBytes);
    for (int s = 0; s < ns; s++) {
      if (st[s].code) continue;
      if (res[3 * s] < 0 || res[3 * s] > st[s].CH + 1) { snprintf(ctx->err, sizeof(ctx->err), "knz walk: bad count"); return -KZ_ERR_DEVICE; }
      st[s].cnt = (int)res[3 * s]; st[s].why = (int)res[3 * s + 2];
    }
  }
  // ---- groups of whole streams: at most a chunk's blocks (decompress_device's batch: 2048 blocks, 8 GiB) ----
  const int64_t capBlocks = ctx->sw.streamChunk > 0 ? ctx->sw.streamChunk : 2048, capBytes = 8LL << 30;
  std::vector<int> ids, have;
  int64_t gBlocks = 0, gBytes = 0;
  auto flush = [&]() -> int {
    if (ids.empty()) return 0;
    const int rc = decompress_group(ctx, st, ids.data(), have.data(), (int)ids.size(), d_src, srcOff, srcLen, d_dst, dstOff, dstCap, dstLen);
    ids.clear(); have.clear(); gBlocks = 0; gBytes = 0;
    return rc;
  };
  for (int s = 0; s < ns; s++) {
    const KnzManyStream& S = st[s];
    if (S.code) { dstLen[s] = S.code; continue; }
    if (S.why == KNZ_WALK_COUNT) {                                // more blocks than a group takes: the single-stream call, on its own
      dstLen[s] = decompress_device(ctx, d_src + srcOff[s], srcLen[s], 0, -1, d_dst + dstOff[s], dstCap[s]);
      if (dstLen[s] == -KZ_ERR_DEVICE) return -KZ_ERR_DEVICE;
      continue;
    }
    const int hv = S.cnt + (S.why == KNZ_WALK_PAYLOAD ? 1 : 0);
    const int64_t blocks = std::max(hv, 1), bytes = blocks * S.h.blockSize;
    if (!ids.empty() && (gBlocks + blocks > capBlocks || gBytes + bytes > capBytes)) { const int rc = flush(); if (rc) return rc; }
    ids.push_back(s); have.push_back(hv);
    gBlocks += blocks; gBytes += bytes;
  }
  return flush();
}


// =================================================================================================
// indexed reads: blocks of a stream by their (bit offset, bit length) pairs, as kz_knz_index / kz_knz_index_device return them, in
// any order.  No walk: every pair is checked against the stream on its own (k_knz_check on the device, knz_check_entry here), which
// makes the call memory safe for any index and brings the block-header bytes for the prechecks; it does not prove that a pair lies
// on the chain of prefixes that starts behind the stream header.
namespace {
// the 5 + lr bits in front of bit `off` read (lr - 3, W) for some lr in 3 .. 34, and lie behind bit hdrEnd; W > 0 ends inside the stream
bool knz_check_entry(const uint8_t* src, int64_t n, int64_t hdrEnd, int64_t off, int64_t W) {
  const int64_t nbits = n * 8;
  if (W <= 0 || W >= (1LL << 34) || off < hdrEnd + 8 || off > nbits || W > nbits - off) return false;
  const int lo = std::max(3, 64 - __builtin_clzll((unsigned long long)W));
  for (int lr = lo; lr <= 34; lr++) {
    const int64_t at = off - 5 - lr;
    if (at < hdrEnd) break;
    HostBitsIn t{src, (uint64_t)nbits, (uint64_t)at, false};
    if ((int)t.get(5) + 3 == lr && (int64_t)t.get(lr) == W) return true;
  }
  return false;
}
struct IndexedCall {                                               // what both forms take from the stream header
  KnzHeader h; int nbFunctions; int64_t hdrEnd, iS; int CH;
};
int indexed_open(kz_ctx* ctx, HostBitsIn& bs, int64_t dstStride, IndexedCall& c) {
  { const int hrc = read_stream_header(bs, c.h, ctx->err, sizeof(ctx->err)); if (hrc) return hrc; }
  if (dstStride < c.h.blockSize) {
    snprintf(ctx->err, sizeof(ctx->err), "dstStride %lld is less than the stream's block size %d", (long long)dstStride, c.h.blockSize);
    return -KZ_ERR_INVALID_PARAM;
  }
  c.nbFunctions = 0;
  for (int i = 0; i < 8; i++) if (((c.h.transformType >> (42 - 6 * i)) & 0x3F) != 0) c.nbFunctions++;
  if (c.nbFunctions == 0) c.nbFunctions = 1;
  c.hdrEnd = (int64_t)bs.pos;
  c.iS = (int64_t)kz_align((size_t)c.h.blockSize + (size_t)(c.h.blockSize >> 3) + 1024 + 64, 256);
  c.CH = knz_chunk_blocks(ctx, c.h.blockSize);
  return 0;
}
int indexed_mismatch(kz_ctx* ctx, int64_t i) {
  snprintf(ctx->err, sizeof(ctx->err), "index entry %lld does not match the stream", (long long)i);
  return -KZ_ERR_INVALID_PARAM;
}
// Decode the chunk's entries that passed their prechecks (res[i].status == 0 on entry), rows `iS` apart at `rows`, into out rows
// `dstStride` apart: one kz_decode_blocks call per run of neighbours, so that every block lands in its own row.
int indexed_decode_runs(kz_ctx* ctx, const IndexedCall& c, const uint8_t* rows, const int64_t* W, int cnt, uint8_t* out, int64_t dstStride,
                        kz_block_result* res, int memKind) {
  for (int i = 0; i < cnt;) {
    if (res[i].status) { i++; continue; }
    int j = i + 1;
    while (j < cnt && !res[j].status) j++;
    const int rc = kz_decode_blocks(ctx, c.h.transformType, (uint32_t)c.h.entropyType, c.h.blockSize, rows + (int64_t)i * c.iS, c.iS, W + i, j - i,
                                    out + (int64_t)i * dstStride, dstStride, res + i, memKind);
    if (rc) return rc;
    i = j;
  }
  return 0;
}
}  // namespace

extern "C" int32_t kz_decode_indexed(kz_ctx* ctx, const uint8_t* src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, int32_t nBlocks,
                                     uint8_t* dst, int64_t dstStride, kz_block_result* results) {
  if (!ctx || !src || n < 0 || nBlocks < 0 || (nBlocks > 0 && (!blockBitOff || !blockBits || !dst || !results))) return -KZ_ERR_INVALID_PARAM;
  KZ_HIP(hipSetDevice(ctx->device));
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  IndexedCall c;
  { const int rc = indexed_open(ctx, bs, dstStride, c); if (rc) return rc; }
  if (nBlocks == 0) return 0;
  for (int64_t i = 0; i < nBlocks; i++) if (!knz_check_entry(src, n, c.hdrEnd, blockBitOff[i], blockBits[i])) return indexed_mismatch(ctx, i);
  const int savedChk = ctx->checksum;
  ctx->checksum = c.h.chkKind;
  struct Restore { kz_ctx* c; int v; ~Restore() { c->checksum = v; } } restore_{ctx, savedChk};
  const int CH = (int)std::min<int64_t>(c.CH, nBlocks);
  std::unique_ptr<uint8_t[]> inbuf(new uint8_t[(size_t)c.iS * CH]);
  for (int64_t b0 = 0; b0 < nBlocks; b0 += CH) {
    const int cnt = (int)std::min<int64_t>(CH, nBlocks - b0);
    const int64_t* off = blockBitOff + b0; const int64_t* W = blockBits + b0;
    kz_block_result* res = results + b0;
    for (int i = 0; i < cnt; i++) {
      HostBitsIn t = bs; t.pos = (uint64_t)off[i]; t.error = false;
      int rc = precheck_block_header(t, (uint64_t)W[i], c.nbFunctions, c.h.blockSize, c.h.chkKind);
      if (!rc && ((W[i] + 7) >> 3) > c.iS - 64) rc = -KZ_ERR_BLOCK_SIZE;
      memset(&res[i], 0, sizeof(res[i]));
      res[i].bits = W[i]; res[i].status = rc;
    }
    parallel_blocks(cnt, [&](int i) {
      if (res[i].status) return;
      HostBitsIn t = bs; t.pos = (uint64_t)off[i]; t.error = false; t.getBytes(inbuf.get() + (size_t)i * c.iS, (uint64_t)W[i]);
    });
    const int rc = indexed_decode_runs(ctx, c, inbuf.get(), W, cnt, dst + b0 * dstStride, dstStride, res, KZ_MEM_HOST);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int32_t kz_decode_indexed_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, int32_t nBlocks,
                                            uint8_t* d_dst, int64_t dstStride, kz_block_result* results) {
  if (!ctx || !d_src || n < 0 || nBlocks < 0 || (nBlocks > 0 && (!blockBitOff || !blockBits || !d_dst || !results))) return -KZ_ERR_INVALID_PARAM;
  KZ_HIP(hipSetDevice(ctx->device));
  uint8_t hdr[32]; int64_t hn = 0;
  { const int rc = knz_get_header(ctx, d_src, n, hdr, hn); if (rc) return rc; }
  HostBitsIn bs{hdr, (uint64_t)hn * 8, 0, false};
  IndexedCall c;
  { const int rc = indexed_open(ctx, bs, dstStride, c); if (rc) return rc; }
  if (nBlocks == 0) return 0;
  const int savedChk = ctx->checksum;
  ctx->checksum = c.h.chkKind;
  struct Restore { kz_ctx* c; int v; ~Restore() { c->checksum = v; } } restore_{ctx, savedChk};
  const int CH = (int)std::min<int64_t>(c.CH, nBlocks);
  // the chunk's tables, pinned and in HBM: 64 spare bytes, then off[CH], bits[CH], hdr[CH], bad[CH]
  { const int rc = knz_tables(ctx, (size_t)CH, 32); if (rc) return rc; }
  int64_t* p_off = (int64_t*)(ctx->knzPin.p + 64); int64_t* p_bits = p_off + CH;
  const uint64_t* p_hdr = (const uint64_t*)(p_bits + CH); const int64_t* p_bad = (const int64_t*)(p_hdr + CH);
  int64_t* d_off = (int64_t*)(ctx->knzAux.p + 64); int64_t* d_bits = d_off + CH;
  uint64_t* d_hdr = (uint64_t*)(d_bits + CH); int64_t* d_bad = (int64_t*)(d_hdr + CH);
  // ---- every entry against the stream, before anything is unpacked; the block-header bytes stay on the host for the second pass ----
  std::vector<uint64_t> hdrs((size_t)nBlocks);
  for (int64_t b0 = 0; b0 < nBlocks; b0 += CH) {
    const int cnt = (int)std::min<int64_t>(CH, nBlocks - b0);
    memcpy(p_off, blockBitOff + b0, (size_t)cnt * 8);
    memcpy(p_bits, blockBits + b0, (size_t)cnt * 8);
    KZ_HIP(hipMemcpyAsync(d_off, p_off, (size_t)cnt * 8, hipMemcpyHostToDevice, ctx->stream));
    KZ_HIP(hipMemcpyAsync(d_bits, p_bits, (size_t)cnt * 8, hipMemcpyHostToDevice, ctx->stream));
    { const int rc = kz_knz_check(ctx, d_src, n, c.hdrEnd, d_off, d_bits, cnt, d_hdr, d_bad); if (rc) return rc; }
    KZ_HIP(hipMemcpyAsync((void*)p_hdr, d_hdr, (size_t)cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipMemcpyAsync((void*)p_bad, d_bad, (size_t)cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
    kz_ktimer_flush(ctx);
    for (int i = 0; i < cnt; i++) {
      if (p_bad[i]) return indexed_mismatch(ctx, b0 + i);
      hdrs[(size_t)(b0 + i)] = p_hdr[i];
    }
  }
  // ---- chunks: prechecks on the host, unpack the entries that pass into staging rows, decode them into their rows of d_dst ----
  const uint64_t nbits = (uint64_t)n * 8;
  for (int64_t b0 = 0; b0 < nBlocks; b0 += CH) {
    const int cnt = (int)std::min<int64_t>(CH, nBlocks - b0);
    kz_block_result* res = results + b0;
    int64_t maxBytes = 0;
    for (int i = 0; i < cnt; i++) {
      const int64_t W = blockBits[b0 + i];
      const int rc = knz_precheck_entry(hdrs[(size_t)(b0 + i)], (uint64_t)W, (uint64_t)blockBitOff[b0 + i], nbits, c.nbFunctions, c.h.blockSize, c.h.chkKind, c.iS);
      memset(&res[i], 0, sizeof(res[i]));
      res[i].bits = W; res[i].status = rc;
      p_off[i] = blockBitOff[b0 + i];
      p_bits[i] = rc ? 0 : W;                                       // a row of no bits: nothing of it is unpacked
      if (!rc) maxBytes = std::max<int64_t>(maxBytes, (W + 7) >> 3);
    }
    if (maxBytes == 0) continue;
    KZ_HIP(hipMemcpyAsync(d_off, p_off, (size_t)cnt * 8, hipMemcpyHostToDevice, ctx->stream));
    KZ_HIP(hipMemcpyAsync(d_bits, p_bits, (size_t)cnt * 8, hipMemcpyHostToDevice, ctx->stream));
    { const int rc = stage_reserve(ctx, ctx->devIn[0], (size_t)cnt * c.iS, false); if (rc) return rc; }
    { const int rc = kz_knz_unpack(ctx, d_src, n, d_off, d_bits, cnt, maxBytes, ctx->devIn[0].p, c.iS); if (rc) return rc; }
    { const int rc = indexed_decode_runs(ctx, c, ctx->devIn[0].p, blockBits + b0, cnt, d_dst + b0 * dstStride, dstStride, res, KZ_MEM_DEVICE); if (rc) return rc; }
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));                      // the pinned table is the next chunk's
    kz_ktimer_flush(ctx);
  }
  return 0;
}
