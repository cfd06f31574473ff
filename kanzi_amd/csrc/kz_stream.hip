// kz_stream.hip -- host side of the .knz container around the HIP block pipeline, source and destination in host memory: the part of
// K/io/CompressedOutputStream.java (writeHeader :236-313, ordered block emission :1024-1035, end
// marker :483-493) and K/io/CompressedInputStream.java (readHeader :359-515, block length prefix
// :1127-1129) that stays on the CPU.  Blocks go to the GPU in batches (kz_encode_blocks /
// kz_decode_blocks); only the bit-granular concatenation happens here.  The container's parsing and its rules are in
// kz_knz_host.h, the calls with source and destination in HBM in kz_stream_device.hip.
#include "kz_knz_stream.h"
#include <stdlib.h>
#include <memory>
#include <thread>
#include <atomic>
#include <mutex>
#include <condition_variable>

// ---- host-only container calls (no GPU needed): used by multi-GPU gathers ----
// Assemble a complete .knz stream from per-block private streams (e.g. gathered from several GPUs
// in block-id order).  Pure host code.
extern "C" int64_t kz_knz_assemble(uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                                   int32_t checksumBits, const uint8_t* streams, int64_t stride, const int64_t* bits, int32_t nBlocks,
                                   uint8_t* dst, int64_t dstCap) {
  if (!dst || nBlocks < 0 || (nBlocks > 0 && (!streams || !bits))) return -KZ_ERR_INVALID_PARAM;
  if (knz_chk_kind(checksumBits) < 0) return -KZ_ERR_INVALID_PARAM;
  HostBits bs{dst, dstCap, 0, false};
  // the block streams carry 4 / 8 hash bytes in their headers when they were coded with kz_ctx_set_checksum(32 / 64): the
  // stream header must say so (CompressedOutputStream.java:244-250) or no reader can parse them
  write_stream_header(bs, transformType, entropyType, blockSize, inputSize, knz_chk_kind(checksumBits));
  for (int i = 0; i < nBlocks; i++) if (bits[i] > 0) write_block(bs, streams + (int64_t)i * stride, (uint64_t)bits[i]);
  write_end_marker(bs);
  if (bs.overflow) return -KZ_ERR_WRITE_FILE;
  return (int64_t)((bs.pos + 7) >> 3);
}

// The same, block by block: a gatherer (rank 0 of a multi-GPU job) appends block streams in block-id order as they arrive instead
// of holding all of them first; memory is one block plus the destination.
struct kz_knz_writer { HostBits bs; };
extern "C" kz_knz_writer* kz_knz_writer_open(uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                                             int32_t checksumBits, uint8_t* dst, int64_t dstCap) {
  if (!dst || dstCap < 32 || knz_chk_kind(checksumBits) < 0) return nullptr;
  kz_knz_writer* w = new kz_knz_writer{HostBits{dst, dstCap, 0, false}};
  write_stream_header(w->bs, transformType, entropyType, blockSize, inputSize, knz_chk_kind(checksumBits));
  return w;
}
extern "C" int32_t kz_knz_writer_add(kz_knz_writer* w, const uint8_t* stream, int64_t bits) {
  if (!w || bits < 0 || (bits > 0 && !stream)) return -KZ_ERR_INVALID_PARAM;
  if (bits > 0) write_block(w->bs, stream, (uint64_t)bits);
  return w->bs.overflow ? -KZ_ERR_WRITE_FILE : 0;
}
extern "C" int64_t kz_knz_writer_close(kz_knz_writer* w) {          // end marker (:491-492); returns the stream's size in bytes
  if (!w) return -KZ_ERR_INVALID_PARAM;
  write_end_marker(w->bs);
  const int64_t r = w->bs.overflow ? -KZ_ERR_WRITE_FILE : (int64_t)((w->bs.pos + 7) >> 3);
  delete w;
  return r;
}

// Parse the stream header and walk the block length prefixes: blockBitOff[i] = bit offset of block
// i's private stream inside src, blockBits[i] = its length W.  Returns the number of blocks or <0.
extern "C" int32_t kz_knz_index(const uint8_t* src, int64_t n, uint64_t* transformType, uint32_t* entropyType,
                                int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits, int64_t* blockBitOff, int64_t* blockBits, int32_t cap) {
  if (!src || n < 20) return -KZ_ERR_INVALID_FILE;
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, nullptr, 0); if (hrc) return hrc; }
  knz_header_out(h, transformType, entropyType, blockSize, inputSize, checksumBits);
  int nb = 0;
  for (;;) {
    uint64_t rd;
    const int prc = knz_read_prefix(bs, rd);
    if (prc < 0) return prc;
    if (prc == KNZ_PREFIX_END) break;
    if (nb < cap) { if (blockBitOff) blockBitOff[nb] = (int64_t)bs.pos; if (blockBits) blockBits[nb] = (int64_t)rd; }
    nb++;
    if (bs.pos + rd > bs.nbits) return -KZ_ERR_READ_FILE;
    bs.pos += rd;
  }
  return nb;
}

// The blocks of a stream found without the walk, in host memory: the rule, the link step and the loop are in kz_knz_host.h.
extern "C" int64_t kz_knz_scan(const uint8_t* src, int64_t n, int32_t minChain, uint64_t* transformType, uint32_t* entropyType, int32_t* blockSize, int64_t* inputSize,
                               int32_t* checksumBits, int64_t* prefixBitOff, int64_t* blockBitOff, int64_t* blockBits, int64_t* next, int64_t cap, int64_t* head) {
  return knz_scan_host(src, n, minChain, transformType, entropyType, blockSize, inputSize, checksumBits, prefixBitOff, blockBitOff, blockBits, next, cap, head);
}

// A new stream out of blocks of existing streams, all in host memory: the plan and the copy are in kz_knz_host.h.
extern "C" int64_t kz_knz_splice_bound(const int64_t* pieceBits, int32_t nPieces) { return knz_splice_bound(pieceBits, nPieces); }
extern "C" int64_t kz_knz_splice(const uint8_t* src, const int64_t* srcOff, const int64_t* srcLen, int32_t nSrc,
                                 const int32_t* pieceSrc, const int64_t* pieceBitOff, const int64_t* pieceBits, int32_t nPieces,
                                 int64_t inputSize, uint8_t* dst, int64_t dstCap) {
  return knz_splice_host(src, srcOff, srcLen, nSrc, pieceSrc, pieceBitOff, pieceBits, nPieces, inputSize, dst, dstCap);
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
    const int lw = knz_prefix_width(W);
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
static int stage_streams(kz_ctx* ctx) {
  if (!ctx->copyUp) KZ_HIP(hipStreamCreateWithFlags(&ctx->copyUp, hipStreamNonBlocking));
  if (!ctx->copyDown) KZ_HIP(hipStreamCreateWithFlags(&ctx->copyDown, hipStreamNonBlocking));
  return 0;
}

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
    int rc = kz_stage_reserve(ctx, ctx->pinIn[i], (size_t)CH * blockSize, true);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->devIn[i], (size_t)CH * blockSize, false);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->devOut[i], (size_t)CH * oS, false);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->pinOut[i], (size_t)CH * oS, true);
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
  if (!knz_block_size_ok(blockSize)) return -KZ_ERR_BLOCK_SIZE;
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
  write_end_marker(bs);
  if (bs.overflow) { snprintf(ctx->err, sizeof(ctx->err), "kz_compress: destination too small"); return -KZ_ERR_WRITE_FILE; }
  return (int64_t)((bs.pos + 7) >> 3);
}


// kz_decompress and kz_decompress_range: the blocks [firstBlock, firstBlock + nBlocks) of the stream, nBlocks < 0: from firstBlock
// to the end marker.  Blocks in front of firstBlock get the walk's checks and nothing else; the batches, and with them the place
// where a destination that is too small cuts the stream, start at firstBlock.
static int64_t decompress_host(kz_ctx* ctx, const uint8_t* src, int64_t n, int64_t firstBlock, int64_t nBlocks, uint8_t* dst, int64_t dstCap) {
  KZ_HIP(hipSetDevice(ctx->device));
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, ctx->err, sizeof(ctx->err)); if (hrc) return hrc; }
  const KnzPlan plan = knz_plan(ctx, h, n, (int64_t)bs.pos);
  const int entropyType = h.entropyType, blockSize = h.blockSize, NB = (int)plan.NB;   // (no more staging than the stream can need)
  const uint64_t tt = h.transformType;
  const int64_t iS = plan.iS;
  ChecksumScope chk(ctx, h.chkKind);
  if (nBlocks == 0) return 0;
  for (int64_t k = 0; k < firstBlock; k++) {                      // read and skipped (:1126-1165 come before the reader looks at "from")
    uint64_t rd;
    const int rc = knz_next_block(bs, plan, rd);
    if (rc == KNZ_PREFIX_END) return 0;                           // the end marker in front of the range
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
      uint64_t rd;
      const int rc = knz_next_block(bs, plan, rd);
      if (rc == KNZ_PREFIX_END) { done = true; break; }
      if (rc) { pending = rc; break; }
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
      const int64_t fit = knz_fit_blocks(dstCap - produced, blockSize);
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
      int rc = kz_stage_reserve(ctx, ctx->pinIn[0], (size_t)off[cnt], true);
      if (!rc) rc = kz_stage_reserve(ctx, ctx->devIn[0], (size_t)cnt * iS, false);
      if (!rc) rc = kz_stage_reserve(ctx, ctx->devOut[0], (size_t)cnt * blockSize, false);
      for (int q = 0; q < 2 && !rc; q++) rc = kz_stage_reserve(ctx, ctx->pinOut[q], (size_t)P * blockSize, true);
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
        code = knz_block_verdict(res[good], blockSize, at[good], dstCap);
        if (code) break;
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
        const int code = knz_block_verdict(res[i], blockSize, produced, dstCap);      // (there is room for whole rows: no ERR_WRITE_FILE here)
        if (code) return code;
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
        const int code = knz_block_verdict(res[i], blockSize, produced, dstCap);
        if (code) return code;
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

// ---- the calls that read a stream by a caller's index: kz_decode_indexed, kz_read_bytes, kz_write_bytes.  Their steps, each once: the
//      open (kz_knz_stream.h), every entry the call uses against the stream before anything is decoded, and the decode of a chunk.
//      kz_stream_device.hip has the same three steps for device memory ----
// entry(i) for i < count = the number of an entry in the caller's index, or -1 for one that the call does not look at
template <class F> static int indexed_check_entries(kz_ctx* ctx, const uint8_t* src, int64_t n, const KnzPlan& P, const int64_t* blockBitOff, const int64_t* blockBits,
                                                    int64_t count, F entry) {
  for (int64_t i = 0; i < count; i++) {
    const int64_t k = entry(i);
    if (k >= 0 && !knz_check_entry(src, n, P.hdrEnd, blockBitOff[k], blockBits[k])) return indexed_mismatch(ctx, k);
  }
  return 0;
}
// A chunk of cnt entries (off[i], W[i]), bs a reader over the stream: the block-header prechecks into res[], the payloads of those
// that pass into inbuf (rows P.iS apart), their decode into out rows `stride` apart.  An entry with leftOut[i] (may be null) is not
// looked at: its res[i] is the caller's, with a status that is not 0.
static int indexed_chunk(kz_ctx* ctx, const HostBitsIn& bs, const KnzPlan& P, const int64_t* off, const int64_t* W, const uint8_t* leftOut, int cnt,
                         uint8_t* inbuf, uint8_t* out, int64_t stride, kz_block_result* res) {
  for (int i = 0; i < cnt; i++) {
    if (leftOut && leftOut[i]) continue;
    HostBitsIn t = bs; t.pos = (uint64_t)off[i]; t.error = false;
    const int rc = knz_check_block(t, (uint64_t)W[i], (uint64_t)off[i], t.nbits, P, false);   // (knz_check_entry saw the payload's end)
    memset(&res[i], 0, sizeof(res[i]));
    res[i].bits = W[i]; res[i].status = rc;
  }
  parallel_blocks(cnt, [&](int i) {
    if (res[i].status) return;
    HostBitsIn t = bs; t.pos = (uint64_t)off[i]; t.error = false; t.getBytes(inbuf + (size_t)i * P.iS, (uint64_t)W[i]);
  });
  return indexed_decode_runs(ctx, P, inbuf, W, cnt, out, stride, res, KZ_MEM_HOST);
}
// segments [s0, s1) of a chunk in up to 64 runs on the host pool: copy(i) per segment, in any order
template <class F> static void segment_runs(int64_t s0, int64_t s1, F copy) {
  const int64_t runs = std::min<int64_t>(s1 - s0, 64);
  parallel_blocks((int)runs, [&](int q) { for (int64_t i = s0 + (s1 - s0) * q / runs; i < s0 + (s1 - s0) * (q + 1) / runs; i++) copy(i); });
}

// Indexed read: blocks of a stream by their (bit offset, bit length) pairs, as kz_knz_index / kz_knz_index_device return them, in
// any order.  No walk: every pair is checked against the stream on its own (knz_check_entry), which makes the call memory safe for
// any index; it does not prove that a pair lies on the chain of prefixes that starts behind the stream header.
extern "C" int32_t kz_decode_indexed(kz_ctx* ctx, const uint8_t* src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, int32_t nBlocks,
                                     uint8_t* dst, int64_t dstStride, kz_block_result* results) {
  if (!ctx || !src || n < 0 || nBlocks < 0 || (nBlocks > 0 && (!blockBitOff || !blockBits || !dst || !results))) return -KZ_ERR_INVALID_PARAM;
  KZ_HIP(hipSetDevice(ctx->device));
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  KnzPlan P;
  { int rc = knz_open_plan(ctx, bs, n, P); if (!rc) rc = indexed_stride(ctx, dstStride, P); if (rc) return rc; }
  if (nBlocks == 0) return 0;
  { const int rc = indexed_check_entries(ctx, src, n, P, blockBitOff, blockBits, nBlocks, [](int64_t i) { return i; }); if (rc) return rc; }
  ChecksumScope chk(ctx, P.h.chkKind);
  const int CH = (int)std::min<int64_t>(knz_chunk_blocks(ctx, P.h.blockSize), nBlocks);
  std::unique_ptr<uint8_t[]> inbuf(new uint8_t[(size_t)P.iS * CH]);
  for (int64_t b0 = 0; b0 < nBlocks; b0 += CH) {
    const int cnt = (int)std::min<int64_t>(CH, nBlocks - b0);
    const int rc = indexed_chunk(ctx, bs, P, blockBitOff + b0, blockBits + b0, nullptr, cnt, inbuf.get(), dst + b0 * dstStride, dstStride, results + b0);
    if (rc) return rc;
  }
  return 0;
}

// Byte-addressed read: many ranges [off, off + len) of the original data in one call.  The plan (kz_knz_host.h) names the distinct
// covering blocks and the range x block segments, chunk by chunk; the shared steps above do the open, the check of every entry the
// plan uses and the decode of a chunk into host rows; what is the read's own is a memcpy per segment out of those rows.
// kz_read_bytes_device (kz_stream_device.hip) is the same call on device memory.
extern "C" int64_t kz_read_bytes(kz_ctx* ctx, const uint8_t* src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, const int64_t* blockByteOff,
                                 int32_t nIndex, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges, uint8_t* dst, int64_t dstCap, int64_t* got) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_read_args(src, n, blockBitOff, blockBits, nIndex, rangeOff, rangeLen, nRanges, dst, dstCap, got); if (rc) return rc; }
  KZ_HIP(hipSetDevice(ctx->device));
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  KnzPlan P;
  { const int rc = knz_open_plan(ctx, bs, n, P); if (rc) return rc; }
  const int32_t blockSize = P.h.blockSize;
  { const int rc = knz_table_refusal(ctx, "kz_read_bytes", blockByteOff, nIndex, blockSize); if (rc) return rc; }
  const int64_t total = knz_read_total(rangeLen, nRanges, dstCap);
  if (total < 0) { snprintf(ctx->err, sizeof(ctx->err), "kz_read_bytes: destination too small"); return total; }
  if (nRanges == 0) return 0;
  const int CH = knz_chunk_blocks(ctx, blockSize);
  KnzReadPlan R;
  knz_read_plan(blockByteOff, nIndex, blockSize, rangeOff, rangeLen, nRanges, CH, 0, R);
  for (int32_t i = 0; i < nRanges; i++) got[i] = 0;
  const int64_t nb = (int64_t)R.blocks.size();
  if (nb == 0) return total;
  { const int rc = indexed_check_entries(ctx, src, n, P, blockBitOff, blockBits, nb, [&](int64_t i) { return (int64_t)R.blocks[(size_t)i]; }); if (rc) return rc; }
  ChecksumScope chk(ctx, P.h.chkKind);
  const int cmax = (int)std::min<int64_t>(CH, nb);
  std::unique_ptr<uint8_t[]> inbuf(new uint8_t[(size_t)P.iS * cmax]), rows(new uint8_t[(size_t)blockSize * cmax]);
  std::vector<kz_block_result> res((size_t)cmax);
  std::vector<int64_t> W((size_t)cmax), off((size_t)cmax);
  for (int64_t b0 = 0, c = 0; b0 < nb; b0 += CH, c++) {
    const int cnt = (int)std::min<int64_t>(CH, nb - b0);
    knz_chunk_entries(&R.blocks[(size_t)b0], nullptr, cnt, blockBitOff, blockBits, off.data(), W.data());
    { const int rc = indexed_chunk(ctx, bs, P, off.data(), W.data(), nullptr, cnt, inbuf.get(), rows.get(), blockSize, res.data()); if (rc) return rc; }
    knz_read_settle(R, c, CH, blockByteOff, nIndex, blockSize, res.data(), got);
    segment_runs(R.first[(size_t)c], R.first[(size_t)c + 1], [&](int64_t i) {
      const KnzReadSeg& g = R.segs[(size_t)i];
      if (g.len > 0) memcpy(dst + g.dst, rows.get() + (size_t)g.slot * blockSize + g.off, (size_t)g.len);
    });
  }
  return total;
}

// Byte-addressed write: many ranges [off, off + len) of the original data replaced by new bytes in one call, the result a new stream.
// The plan (kz_knz_host.h) resolves "the later range wins" into disjoint segments and names the touched blocks and which of them are
// wholly covered.  The shared steps above do the open, the check of every entry the call uses (a wholly covered block's is not looked
// at) and, per chunk of touched blocks, the decode into host rows; the write's own are a memcpy per segment into those rows, one
// batched encode of the rows, and the bit copy of every kept block since the previous chunk with the recoded ones, laid out by
// knz_write_walk (kz_knz_host.h).  kz_write_bytes_device (kz_stream_device.hip) is the same call on device memory, and this one is its
// reference.
extern "C" int64_t kz_write_bytes_bound(const int64_t* blockBits, int32_t nIndex, int32_t blockSize) { return knz_write_bound(blockBits, nIndex, blockSize); }
extern "C" int64_t kz_write_bytes(kz_ctx* ctx, const uint8_t* src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, const int64_t* blockByteOff,
                                  int32_t nIndex, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges, const uint8_t* data, int64_t dataLen,
                                  uint8_t* dst, int64_t dstCap, int64_t* newBitOff, int64_t* newBits) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_write_args(src, n, blockBitOff, blockBits, nIndex, rangeOff, rangeLen, nRanges, data, dataLen, dst, dstCap, newBitOff, newBits); if (rc) return rc; }
  KZ_HIP(hipSetDevice(ctx->device));
  HostBitsIn bs{src, (uint64_t)n * 8, 0, false};
  KnzPlan P;
  { const int rc = knz_open_plan(ctx, bs, n, P); if (rc) return rc; }
  const KnzHeader& h = P.h;
  const int32_t blockSize = h.blockSize;
  { const int rc = knz_table_refusal(ctx, "kz_write_bytes", blockByteOff, nIndex, blockSize); if (rc) return rc; }
  const int CH = knz_chunk_blocks(ctx, blockSize);
  KnzWritePlan R;
  { const int32_t bad = knz_write_plan(blockByteOff, nIndex, blockSize, rangeOff, rangeLen, nRanges, CH, INT64_MAX, R); if (bad >= 0) return knz_write_behind(bad, ctx->err, sizeof(ctx->err)); }
  const int64_t nb = (int64_t)R.blocks.size();
  {                                                                // every entry the call uses: the kept blocks' and the decoded ones'
    int64_t t = 0;
    const int rc = indexed_check_entries(ctx, src, n, P, blockBitOff, blockBits, nIndex,
                                         [&](int64_t k) { return (t < nb && R.blocks[(size_t)t] == k && R.covered[(size_t)t++]) ? (int64_t)-1 : k; });
    if (rc) return rc;
  }
  ChecksumScope chk(ctx, h.chkKind);
  BlockSizeScope scope(ctx, blockSize);
  const int cmax = (int)std::max<int64_t>(1, std::min<int64_t>(CH, nb));
  const int64_t oS = kz_max_block_stream_bytes(blockSize);
  std::unique_ptr<uint8_t[]> inbuf, rows, enc;
  if (nb) { inbuf.reset(new uint8_t[(size_t)P.iS * cmax]); rows.reset(new uint8_t[(size_t)blockSize * cmax]); enc.reset(new uint8_t[(size_t)oS * cmax]); }
  std::vector<kz_block_result> res((size_t)cmax), eres((size_t)cmax);
  std::vector<int64_t> W((size_t)cmax), off((size_t)cmax), eW((size_t)cmax);
  std::vector<int32_t> lens((size_t)cmax);
  auto tooSmall = [&]() { snprintf(ctx->err, sizeof(ctx->err), "kz_write_bytes: destination too small"); return (int64_t)-KZ_ERR_WRITE_FILE; };
  HostBits out{dst, dstCap, 0, false};
  int64_t pos = 0;                                                // the bit behind what has been laid out (out.pos follows it)
  {
    uint8_t nh[32];
    HostBits hb{nh, 32, 0, false};
    write_stream_header(hb, h.transformType, (uint32_t)h.entropyType, blockSize, h.inputSize, h.chkKind);
    pos = (int64_t)hb.pos;
  }
  // blocks [k0, k1) behind what has been written, the touched ones t0 .. t1 of the list from the encoder's rows; then tailBits zero
  // bits.  Decided from the bit arithmetic before a bit of them is written: -KZ_ERR_WRITE_FILE when they do not fit.
  auto emit = [&](int64_t k0, int64_t k1, int64_t t0, int64_t t1, int tailBits) -> int {
    int64_t t = t0;
    const int64_t end = knz_write_walk(blockBits, R.blocks.data(), k0, k1, t, t1, eW.data(), pos, knz_write_walk_only);
    if (((end + tailBits + 7) >> 3) > dstCap) return -KZ_ERR_WRITE_FILE;
    if (out.pos == 0) write_stream_header(out, h.transformType, (uint32_t)h.entropyType, blockSize, h.inputSize, h.chkKind);
    t = t0;
    knz_write_walk(blockBits, R.blocks.data(), k0, k1, t, t1, eW.data(), pos, [&](int64_t k, int64_t r, int64_t w, int64_t pay) {
      const int lw = knz_prefix_width((uint64_t)w);
      out.put((uint64_t)(lw - 3), 5);
      out.put((uint64_t)w, lw);
      if (newBitOff) { newBitOff[k] = pay; newBits[k] = w; }
      if (r >= 0) out.putBytes(enc.get() + (size_t)(r - t0) * oS, (uint64_t)w);
      else knz_copy_bits(out, src, n, blockBitOff[k], w);
    });
    if (tailBits) write_end_marker(out);
    pos = end + tailBits;
    return out.overflow ? -KZ_ERR_WRITE_FILE : 0;
  };
  int64_t next = 0;                                               // the first block not yet in the new stream
  for (int64_t b0 = 0, c = 0; b0 < nb; b0 += CH, c++) {
    const int cnt = (int)std::min<int64_t>(CH, nb - b0);
    const uint8_t* covered = &R.covered[(size_t)b0];
    knz_chunk_entries(&R.blocks[(size_t)b0], covered, cnt, blockBitOff, blockBits, off.data(), W.data());
    knz_write_covered(R, b0, cnt, blockByteOff, false, res.data());
    { const int rc = indexed_chunk(ctx, bs, P, off.data(), W.data(), covered, cnt, inbuf.get(), rows.get(), blockSize, res.data()); if (rc) return rc; }
    knz_write_covered(R, b0, cnt, blockByteOff, true, res.data());
    { const int rc = knz_write_settle(R, c, CH, blockByteOff, nIndex, blockSize, res.data(), lens.data(), ctx->err, sizeof(ctx->err)); if (rc) return rc; }
    segment_runs(R.first[(size_t)c], R.first[(size_t)c + 1], [&](int64_t i) {           // disjoint, so in any order
      const KnzWriteSeg& g = R.segs[(size_t)i];
      memcpy(rows.get() + (size_t)g.slot * blockSize + g.off, data + g.src, (size_t)g.len);
    });
    {
      int rc = kz_encode_blocks_pre(ctx, h.transformType, (uint32_t)h.entropyType, blockSize, rows.get(), blockSize, lens.data(), cnt, enc.get(), oS, eres.data(), KZ_MEM_HOST, nullptr);
      if (!rc) rc = knz_recoded_bits(ctx, &R.blocks[(size_t)b0], eres.data(), cnt, eW.data());
      if (rc) return rc;
    }
    const int64_t k1 = (int64_t)R.blocks[(size_t)(b0 + cnt - 1)] + 1;
    if (emit(next, k1, b0, b0 + cnt, 0)) return tooSmall();
    next = k1;
  }
  if (emit(next, nIndex, nb, nb, 8)) return tooSmall();            // the kept tail and the end marker
  return (int64_t)((out.pos + 7) >> 3);
}
