// kz_stream_device.hip -- the .knz container with source and destination in HBM: the same streams as kz_stream.hip's calls write and
// read, whole, by block range, by index, and many at a time, edits them without recoding (the splice), and reads and rewrites byte
// ranges of their data (kz_read_bytes_device, kz_write_bytes_device), and indexes and reads many of them in one call
// (kz_knz_index_many_device, kz_read_bytes_many_device), and rewrites ranges of many of them in one call
// (kz_write_bytes_many_device).  The kernels are in kz_knz_gpu.hip; what stays on the host is what
// kz_compress / kz_decompress do there as well and costs nothing: the stream header (kz_knz_host.h, on a copy of at most 26 bytes),
// the bit-offset arithmetic over results[] (host arrays anyway), and the block checks on the 8 header bytes per block that the walk
// kernel brings back.  The rules shared with the host-buffer calls are in kz_knz_host.h and kz_knz_stream.h.
#include "kz_knz_stream.h"

namespace {
// `need` bytes of pinned table and of its HBM mirror behind 64 bytes of front (the stream header resp. a walk's result).  All device
// calls use the same two buffers: nothing is kept in them across a call.
int knz_tables(kz_ctx* ctx, size_t need) {
  int rc = kz_stage_reserve(ctx, ctx->knzPin, need + 64, true);
  if (!rc) rc = kz_stage_reserve(ctx, ctx->knzAux, need + 64, false);
  return rc;
}
// A view of those tables from byte `at` of both: `front` bytes, then columns of cap 8-byte entries each.  The walk's tables are
// (off, bits, hdr), the index check's (off, bits, hdr, bad); the d_ forms are the HBM mirror's.
struct KnzTable {
  uint8_t* pin; uint8_t* dev; size_t front; int64_t cap;
  KnzTable(kz_ctx* ctx, int64_t cap_, size_t at = 0, size_t front_ = 64) : pin(ctx->knzPin.p + at), dev(ctx->knzAux.p + at), front(front_), cap(cap_) {}
  size_t bytes(int cols) const { return front + (size_t)cols * (size_t)cap * 8; }
  int64_t* head() const { return (int64_t*)pin; }
  int64_t* col(int k) const { return (int64_t*)(pin + front) + k * cap; }
  int64_t* d_head() const { return (int64_t*)dev; }
  int64_t* d_col(int k) const { return (int64_t*)(dev + front) + k * cap; }
  int64_t* off() const { return col(0); }
  int64_t* bits() const { return col(1); }
  uint64_t* hdr() const { return (uint64_t*)col(2); }
  int64_t* bad() const { return col(3); }
  int64_t* d_off() const { return d_col(0); }
  int64_t* d_bits() const { return d_col(1); }
  uint64_t* d_hdr() const { return (uint64_t*)d_col(2); }
  int64_t* d_bad() const { return d_col(3); }
};
// The layout of a run of blocks behind bit `pos` of a stream: rows of W[i] bits (W[i] <= 0: no block), the row of block i at byte
// rowBase + i * stride.  Per block its length prefix, then its payload, entered at t[m++].  Returns the bit behind the last payload.
int64_t knz_layout_rows(const int64_t* W, int cnt, int64_t pos, int64_t rowBase, int64_t stride, KnzBlk* t, int& m) {
  for (int i = 0; i < cnt; i++) {
    if (W[i] <= 0) continue;
    pos += 5 + knz_prefix_width((uint64_t)W[i]);
    t[m++] = KnzBlk{pos, W[i], rowBase + (int64_t)i * stride};
    pos += W[i];
  }
  return pos;
}
// The rows' streams (W[i] bits each, rows `stride` apart, W[i] <= 0: no block) go behind bit `pos` of d_dst, then tailBits zero bits;
// pos moves behind them.  -KZ_ERR_WRITE_FILE, nothing launched, when that does not fit in dstCap bytes.
int knz_pack_rows(kz_ctx* ctx, const uint8_t* d_rows, int64_t stride, const int64_t* W, int cnt, uint8_t* d_dst, int64_t dstCap, int64_t& pos, int tailBits) {
  KnzBlk* t = (KnzBlk*)(ctx->knzPin.p + 64);
  int m = 0;
  const int64_t end = knz_layout_rows(W, cnt, pos, 0, stride, t, m) + tailBits;
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
// a reader over the first bytes of d_src (hdr: the 32 bytes that hold them), for the stream header of a reading call
int knz_open(kz_ctx* ctx, const uint8_t* d_src, int64_t n, uint8_t* hdr /*32*/, HostBitsIn& bs) {
  int64_t hn = 0;
  { const int rc = knz_get_header(ctx, d_src, n, hdr, hn); if (rc) return rc; }
  bs = HostBitsIn{hdr, (uint64_t)hn * 8, 0, false};
  return 0;
}
// the open of a reading call: the stream header of d_src with its faults and texts, and the plan
int knz_open_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, KnzPlan& P) {
  uint8_t hdr[32]; HostBitsIn bs;
  { const int rc = knz_open(ctx, d_src, n, hdr, bs); if (rc) return rc; }
  return knz_open_plan(ctx, bs, n, P);
}
}  // namespace

extern "C" int64_t kz_knz_assemble_device(kz_ctx* ctx, uint64_t transformType, uint32_t entropyType, int32_t blockSize, int64_t inputSize,
                                          int32_t checksumBits, const uint8_t* d_streams, int64_t stride, const int64_t* bits, int32_t nBlocks,
                                          uint8_t* d_dst, int64_t dstCap) {
  if (!ctx || !d_dst || nBlocks < 0 || (nBlocks > 0 && (!d_streams || !bits))) return -KZ_ERR_INVALID_PARAM;
  if (knz_chk_kind(checksumBits) < 0) return -KZ_ERR_INVALID_PARAM;
  KZ_HIP(hipSetDevice(ctx->device));
  uint8_t hdr[32];
  HostBits hb{hdr, 32, 0, false};
  write_stream_header(hb, transformType, entropyType, blockSize, inputSize, knz_chk_kind(checksumBits));
  { const int rc = knz_tables(ctx, (size_t)std::max(nBlocks, 1) * sizeof(KnzBlk)); if (rc) return rc; }
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
  if (!knz_block_size_ok(blockSize)) return -KZ_ERR_BLOCK_SIZE;
  KZ_HIP(hipSetDevice(ctx->device));
  uint8_t hdr[32];
  HostBits hb{hdr, 32, 0, false};
  write_stream_header(hb, transformType, entropyType, blockSize, n, ctx->checksum);
  const int64_t nblocks = (n + blockSize - 1) / blockSize;
  BlockSizeScope scope(ctx, blockSize);
  const int CH = (int)std::min<int64_t>(knz_chunk_blocks(ctx, blockSize), std::max<int64_t>(nblocks, 1));
  const int64_t oS = kz_max_block_stream_bytes(blockSize);
  {
    int rc = kz_stage_reserve(ctx, ctx->devOut[0], (size_t)CH * oS, false);
    if (!rc) rc = knz_tables(ctx, (size_t)CH * sizeof(KnzBlk));
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

namespace {
// walk up to maxCount (<= T.cap) prefixes from bit pos and bring the tables back (arrays = 2: offsets and lengths, 3: the header bytes as well)
int knz_walk_chunk(kz_ctx* ctx, const KnzTable& T, const uint8_t* d_src, int64_t n, int64_t pos, int maxCount, int arrays) {
  { const int rc = kz_knz_walk(ctx, d_src, n, pos, maxCount, T.d_off(), T.d_bits(), T.d_hdr(), T.d_head()); if (rc) return rc; }
  KZ_HIP(hipMemcpyAsync(T.pin, T.dev, T.bytes(arrays), hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  if (T.head()[0] < 0 || T.head()[0] > maxCount) { snprintf(ctx->err, sizeof(ctx->err), "knz walk: bad count"); return -KZ_ERR_DEVICE; }
  return 0;
}
// the entries a walk recorded: the blocks walked whole, and the one whose payload does not fit (recorded before its end is looked at)
inline int knz_walk_have(int64_t got, int64_t why) { return (int)got + (why == KNZ_WALK_PAYLOAD ? 1 : 0); }
// knz_check_block on a block that the device walked or checked: the block header is read from the 8 bytes it brought back
int knz_check_walked(uint64_t hdr, uint64_t rd, uint64_t at, uint64_t nbits, const KnzPlan& P) {
  uint8_t hb8[8];
  for (int k = 0; k < 8; k++) hb8[k] = (uint8_t)(hdr >> (56 - 8 * k));
  const HostBitsIn t{hb8, std::min<uint64_t>(64, nbits - at), 0, false};          // the header is 7 bytes at the most
  return knz_check_block(t, rd, at, nbits, P);
}
}  // namespace

extern "C" int32_t kz_knz_index_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, uint64_t* transformType, uint32_t* entropyType,
                                       int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits, int64_t* blockBitOff, int64_t* blockBits, int32_t cap) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  if (!d_src || n < 20) return -KZ_ERR_INVALID_FILE;
  KZ_HIP(hipSetDevice(ctx->device));
  uint8_t hdr[32]; HostBitsIn bs;
  { const int rc = knz_open(ctx, d_src, n, hdr, bs); if (rc) return rc; }
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, nullptr, 0); if (hrc) return hrc; }
  knz_header_out(h, transformType, entropyType, blockSize, inputSize, checksumBits);
  const int CH = (int)std::min<int64_t>(16384, n / 8 + 16);
  { const int rc = knz_tables(ctx, (size_t)CH * 24); if (rc) return rc; }
  const KnzTable T(ctx, CH);
  int64_t pos = (int64_t)bs.pos, nb = 0;
  for (;;) {
    { const int rc = knz_walk_chunk(ctx, T, d_src, n, pos, CH, 2); if (rc) return rc; }
    const int why = (int)T.head()[2], have = knz_walk_have(T.head()[0], why);     // kz_knz_index records a block before it looks at its end
    for (int i = 0; i < have; i++, nb++)
      if (nb < cap) { if (blockBitOff) blockBitOff[nb] = T.off()[i]; if (blockBits) blockBits[nb] = T.bits()[i]; }
    if (why == KNZ_WALK_PREFIX || why == KNZ_WALK_PAYLOAD) return -KZ_ERR_READ_FILE;
    if (why == KNZ_WALK_END) break;
    pos = T.head()[1];
    if (nb > 0x7FFFFFFF - CH) return -KZ_ERR_INVALID_FILE;
  }
  return (int32_t)nb;
}

// kz_knz_scan with the stream in HBM: kz_knz_host.h's rule at every bit position (pass 1, in tiles) and its link step over the
// accepted positions (kz_knz_gpu.hip).  Three waits whatever n is: the stream header, the number A of accepted positions (the
// scratch is proportional to it; when the tables grow for it, the count pass runs once more), the results.  The table buffers hold, behind 64 bytes of front: the tiles' first indices and counts,
// the four result columns of min(A, cap) entries, the link passes' columns.
extern "C" int64_t kz_knz_scan_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, int32_t minChain, uint64_t* transformType, uint32_t* entropyType, int32_t* blockSize,
                                      int64_t* inputSize, int32_t* checksumBits, int64_t* prefixBitOff, int64_t* blockBitOff, int64_t* blockBits, int64_t* next,
                                      int64_t cap, int64_t* head) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_scan_args(d_src, n, minChain, prefixBitOff, blockBitOff, blockBits, next, cap, head); if (rc) return rc; }
  if (n < 20) return -KZ_ERR_INVALID_FILE;
  KZ_HIP(hipSetDevice(ctx->device));
  KnzPlan P;
  { const int rc = knz_open_device(ctx, d_src, n, P); if (rc) return rc; }
  knz_header_out(P.h, transformType, entropyType, blockSize, inputSize, checksumBits);
  const KnzScanRule R = knz_scan_rule(P.h, P.hdrEnd, n);
  const int64_t nTiles = kz_knz_scan_tiles_of(d_src, n);
  const size_t offAt = 64, cntAt = offAt + (size_t)(nTiles + 1) * 8, outAt = cntAt + kz_align((size_t)nTiles * 4, 8);
  auto count = [&]() { return kz_knz_scan_count(ctx, d_src, n, R, nTiles, (int32_t*)(ctx->knzAux.p + cntAt), (int64_t*)(ctx->knzAux.p + offAt)); };
  {                                                                                 // (the pinned side: the front, later the result columns)
    int rc = kz_stage_reserve(ctx, ctx->knzPin, 64, true);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->knzAux, outAt, false);
    if (!rc) rc = count();
    if (rc) return rc;
  }
  KZ_HIP(hipMemcpyAsync(ctx->knzPin.p, ctx->knzAux.p + offAt + (size_t)nTiles * 8, 8, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  const int64_t A = *(const int64_t*)ctx->knzPin.p;
  if (A < 0 || A > n * 8 || A > 0x7FFFFFF0LL) { snprintf(ctx->err, sizeof(ctx->err), "knz scan: bad count"); return -KZ_ERR_DEVICE; }
  const int64_t M = std::min(A, cap);
  const size_t colsAt = outAt + (size_t)M * 32;
  {
    // A table that grows is a new allocation (kz_stage_reserve frees the old one first, so the same address may come back with other
    // contents): whether it grew is decided by its capacity, and the tiles' first indices are then counted once more.
    const size_t had = ctx->knzAux.cap;
    int rc = kz_stage_reserve(ctx, ctx->knzPin, 64 + (size_t)M * 32, true);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->knzAux, colsAt + kz_knz_scan_cols_bytes(A), false);
    if (!rc && ctx->knzAux.cap != had) rc = count();
    if (rc) return rc;
  }
  const int mc = (int)std::min<int64_t>(minChain, A + 1);                           // (no path is longer than A)
  int64_t* d_res = (int64_t*)ctx->knzAux.p;
  int rc = kz_knz_scan_links(ctx, d_src, n, R, nTiles, (const int64_t*)(ctx->knzAux.p + offAt), ctx->knzAux.p + colsAt, A, mc);
  if (!rc) rc = kz_knz_scan_emit(ctx, d_src, n, R, ctx->knzAux.p + colsAt, A, cap, (int64_t*)(ctx->knzAux.p + outAt), M, d_res);
  if (rc) return rc;
  KZ_HIP(hipMemcpyAsync(ctx->knzPin.p, d_res, 64, hipMemcpyDeviceToHost, ctx->stream));
  if (M) KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + 64, ctx->knzAux.p + outAt, (size_t)M * 32, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  const int64_t K = ((const int64_t*)ctx->knzPin.p)[0];
  if (K < 0 || K > A) { snprintf(ctx->err, sizeof(ctx->err), "knz scan: bad count"); return -KZ_ERR_DEVICE; }
  *head = ((const int64_t*)ctx->knzPin.p)[1];
  const int64_t got = std::min(K, cap);
  const int64_t* out = (const int64_t*)(ctx->knzPin.p + 64);
  int64_t* const cols[4] = {prefixBitOff, blockBitOff, blockBits, next};
  for (int k = 0; k < 4; k++) if (got) memcpy(cols[k], out + k * M, (size_t)got * 8);
  return K;
}

// kz_decompress_device and kz_decompress_range_device: decompress_host's contract (kz_stream.hip), source and destination in HBM.
// kz_decompress looks at the room left in dst once per batch of ITS size (KnzPlan::NB), so chunks never straddle those batches and
// carry the batch's count of blocks that may still start inside dst: both calls cut a stream at the same block.
static int64_t decompress_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, int64_t firstBlock, int64_t nBlocks, uint8_t* d_dst, int64_t dstCap) {
  KZ_HIP(hipSetDevice(ctx->device));
  KnzPlan P;
  { const int rc = knz_open_device(ctx, d_src, n, P); if (rc) return rc; }
  const KnzHeader& h = P.h;
  const int entropyType = h.entropyType, blockSize = h.blockSize, CH = P.CH;
  const uint64_t tt = h.transformType, nbits = (uint64_t)n * 8;
  const int64_t iS = P.iS;
  ChecksumScope chk(ctx, h.chkKind);
  if (nBlocks == 0) return 0;
  // blocks in front of the range are walked in the index call's chunks (the walk is all that happens to them), unless
  // KZ_STREAM_CHUNK says otherwise
  const int SK = firstBlock == 0 ? 0 : (ctx->sw.streamChunk > 0 ? CH : (int)std::min<int64_t>(16384, n / 8 + 16));
  { const int rc = knz_tables(ctx, (size_t)std::max(CH, SK) * 24); if (rc) return rc; }
  int64_t pos = P.hdrEnd, produced = 0;
  for (int64_t k = 0; k < firstBlock;) {                         // read and skipped: prefix and block header, not the payload
    const KnzTable T(ctx, SK);
    { const int rc = knz_walk_chunk(ctx, T, d_src, n, pos, (int)std::min<int64_t>(SK, firstBlock - k), 3); if (rc) return rc; }
    const int why = (int)T.head()[2], have = knz_walk_have(T.head()[0], why);
    for (int i = 0; i < have; i++) {
      const int rc = knz_check_walked(T.hdr()[i], (uint64_t)T.bits()[i], (uint64_t)T.off()[i], nbits, P);
      if (rc) return rc;
    }
    if (why == KNZ_WALK_PREFIX) return -KZ_ERR_READ_FILE;
    if (why == KNZ_WALK_END) return 0;                            // the end marker in front of the range
    pos = T.head()[1];
    k += have;
  }
  const KnzTable T(ctx, CH);
  std::vector<kz_block_result> res(CH);
  bool done = false;
  int pending = 0;
  int64_t batchLeft = 0, fitLeft = 0;
  int64_t left = nBlocks < 0 ? INT64_MAX : nBlocks;               // blocks of the range not walked yet
  while (!done) {
    if (left == 0) break;                                         // the end of the range: nothing behind it is read
    if (batchLeft == 0) { batchLeft = P.NB; fitLeft = knz_fit_blocks(dstCap - produced, blockSize); }
    const int want = (int)std::min<int64_t>(std::min<int64_t>(CH, batchLeft), left);
    // ---- the walk on the device, then kz_decompress's checks in kz_decompress's order on what it recorded.  A fault met here is
    //      held back until the blocks before it have been decoded: the reference reports the FIRST failing block in stream order ----
    { const int rc = knz_walk_chunk(ctx, T, d_src, n, pos, want, 3); if (rc) return rc; }
    const int why = (int)T.head()[2], have = knz_walk_have(T.head()[0], why);
    pos = T.head()[1];
    int cnt = 0;
    for (; cnt < have; cnt++) {
      pending = knz_check_walked(T.hdr()[cnt], (uint64_t)T.bits()[cnt], (uint64_t)T.off()[cnt], nbits, P);
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
    for (int i = 0; i < cnt; i++) maxBytes = std::max<int64_t>(maxBytes, (T.bits()[i] + 7) >> 3);
    { const int rc = kz_stage_reserve(ctx, ctx->devIn[0], (size_t)cnt * iS, false); if (rc) return rc; }   // (grow-only: the blocks walked, not the chunk's most)
    { const int rc = kz_knz_unpack(ctx, d_src, n, T.d_off(), T.d_bits(), cnt, maxBytes, ctx->devIn[0].p, iS); if (rc) return rc; }
    // ---- blocks whose whole blockSize row lies inside what is left of dst are decoded in place; the others (as a rule the last
    //      block of a destination of the exact size) into staging rows ----
    const int nd = (int)std::min<int64_t>(cnt, (dstCap - produced) / blockSize);
    if (cnt > nd) { const int rc = kz_stage_reserve(ctx, ctx->devOut[0], (size_t)(cnt - nd) * blockSize, false); if (rc) return rc; }
    int rc = 0;
    if (nd) rc = kz_decode_blocks(ctx, tt, (uint32_t)entropyType, blockSize, ctx->devIn[0].p, iS, T.bits(), nd,
                                  d_dst + produced, blockSize, res.data(), KZ_MEM_DEVICE);
    if (!rc && cnt > nd) rc = kz_decode_blocks(ctx, tt, (uint32_t)entropyType, blockSize, ctx->devIn[0].p + (int64_t)nd * iS, iS, T.bits() + nd, cnt - nd,
                                               ctx->devOut[0].p, blockSize, res.data() + nd, KZ_MEM_DEVICE);
    if (rc) return rc;
    // ---- the reader appends whatever a block produced (:783-785): a block behind a short one moves left, in stream order; the
    //      first failing block ends the stream, the blocks in front of it are delivered ----
    const int64_t base = produced;
    int code = 0;
    for (int i = 0; i < cnt; i++) {
      code = knz_block_verdict(res[i], blockSize, produced, dstCap);
      if (code) break;
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
    int rc = kz_stage_reserve(ctx, ctx->devIn[0], (size_t)std::max(NBk, 1) * (size_t)blockSize, false);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->devOut[0], (size_t)std::max(NBk, 1) * (size_t)oS, false);
    if (!rc) rc = knz_tables(ctx, gatherBytes + segBytes + (size_t)NBk * sizeof(KnzBlk));
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
  std::vector<int64_t> W((size_t)NBk);
  for (int i = 0; i < NBk; i++) W[i] = res[i].bits;
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
    const int m0 = m;
    const int64_t end = knz_layout_rows(W.data() + first, nb, (int64_t)hb.pos, (int64_t)first * oS, oS, blk, m) + 8;   // end marker (:491-492)
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
  if (!knz_block_size_ok(blockSize)) return -KZ_ERR_BLOCK_SIZE;   // kz_compress_device's check
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
  KnzPlan plan; int code;                                          // (the walk starts at plan.hdrEnd)
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
  { const int rc = knz_tables(ctx, tBytes + outBytes); if (rc) return rc; }
  const KnzTable T(ctx, E, tBytes, (size_t)ng * 24);              // behind the KnzSrc entries: res[3 ng], then off[E], bits[E], hdr[E]
  {
    KnzSrc* t = (KnzSrc*)ctx->knzPin.p;
    int64_t base = 0;
    for (int k = 0; k < ng; k++) {
      const int s = ids[k];
      t[k] = KnzSrc{srcOff[s], srcLen[s], st[s].plan.hdrEnd, base, st[s].plan.CH + 1, have[k]};
      base += have[k];
    }
  }
  const int64_t* res = T.head();
  const int64_t* off = T.off();
  const int64_t* bits = T.bits();
  const uint64_t* hdr = T.hdr();
  KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, ctx->knzPin.p, (size_t)ng * sizeof(KnzSrc), hipMemcpyHostToDevice, ctx->stream));
  { const int rc = kz_knz_walk_many(ctx, d_src, (const KnzSrc*)ctx->knzAux.p, ng, T.d_off(), T.d_bits(), T.d_hdr(), T.d_head()); if (rc) return rc; }
  KZ_HIP(hipMemcpyAsync(T.pin, T.dev, outBytes, hipMemcpyDeviceToHost, ctx->stream));
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
    const KnzPlan& S = st[s].plan;
    const int64_t got = res[3 * k], why = res[3 * k + 2];
    if (got < 0 || got > S.CH + 1) { snprintf(ctx->err, sizeof(ctx->err), "knz walk: bad count"); return -KZ_ERR_DEVICE; }
    const int hv = std::min(knz_walk_have(got, why), have[k]);
    const uint64_t nbits = (uint64_t)srcLen[s] * 8;
    int cnt = 0, pending = 0;
    for (; cnt < hv; cnt++) {
      pending = knz_check_walked(hdr[base + cnt], (uint64_t)bits[base + cnt], (uint64_t)off[base + cnt], nbits, S);
      if (pending) break;
    }
    if (!pending && why != KNZ_WALK_END) pending = -KZ_ERR_READ_FILE;     // a prefix that does not fit
    if (cnt > 0) {                                                // blocks that start past the end of the destination cannot be stored
      const int64_t fit = knz_fit_blocks(dstCap[s], S.h.blockSize);
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
    int rc = kz_stage_reserve(ctx, ctx->devIn[0], (size_t)inBytes + 64, false);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->devOut[0], (size_t)outBytes2 + 64, false);
    if (!rc) rc = knz_tables(ctx, rowBytes + copyBytes);          // (may move the tables: everything needed from them is in W / rowT / parts)
    if (rc) return rc;
    memcpy(ctx->knzPin.p, rowT.data(), (size_t)R * sizeof(KnzRow));
    KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, ctx->knzPin.p, (size_t)R * sizeof(KnzRow), hipMemcpyHostToDevice, ctx->stream));
    rc = kz_knz_unpack_many(ctx, d_src, (const KnzRow*)ctx->knzAux.p, R, maxBytes, ctx->devIn[0].p);
    if (rc) return rc;
  }
  // ---- one decode per distinct header, into staging rows ----
  std::vector<int> crc(cls.size(), 0);
  {
    ChecksumScope chk(ctx, ctx->checksum);                        // each class decodes under its own header's kind
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
      code = knz_block_verdict(b, C.bs, produced, dstCap[P.s]);
      if (code) break;
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
  { const int rc = knz_tables(ctx, tBytes + std::max(headBytes, resBytes)); if (rc) return rc; }
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
    KnzHeader h;
    S.code = read_stream_header(bs, h, firstFault ? ctx->err : nullptr, sizeof(ctx->err));   // (the text of the first failing stream stays)
    if (S.code) { firstFault = false; t[s].maxCount = 0; continue; }
    S.plan = knz_plan(ctx, h, n, (int64_t)bs.pos);                // decompress_device's batch and chunk
    t[s].startBit = S.plan.hdrEnd; t[s].maxCount = S.plan.CH + 1;
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
      if (res[3 * s] < 0 || res[3 * s] > st[s].plan.CH + 1) { snprintf(ctx->err, sizeof(ctx->err), "knz walk: bad count"); return -KZ_ERR_DEVICE; }
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
    const int hv = knz_walk_have(S.cnt, S.why);
    const int64_t blocks = std::max(hv, 1), bytes = blocks * S.plan.h.blockSize;
    if (!ids.empty() && (gBlocks + blocks > capBlocks || gBytes + bytes > capBytes)) { const int rc = flush(); if (rc) return rc; }
    ids.push_back(s); have.push_back(hv);
    gBlocks += blocks; gBytes += bytes;
  }
  return flush();
}

namespace {
// the first bytes of the streams ids[0 .. nn) of a many-stream call in one table, one copy (k_knz_heads): stream ids[k]'s 32 bytes are
// at knzPin + tBytes + 32 k when the call returns, behind the nn KnzSrc entries (tBytes = those, in whole 64 bytes), which stay the caller's
int knz_many_heads(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff, const int64_t* srcLen, const int32_t* ids, int nn, size_t tBytes) {
  KnzSrc* t = (KnzSrc*)ctx->knzPin.p;
  for (int k = 0; k < nn; k++) t[k] = KnzSrc{srcOff[ids[k]], srcLen[ids[k]], 0, 0, 0, 0};
  KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, t, (size_t)nn * sizeof(KnzSrc), hipMemcpyHostToDevice, ctx->stream));
  { const int rc = kz_knz_heads(ctx, d_src, (const KnzSrc*)ctx->knzAux.p, nn, ctx->knzAux.p + tBytes); if (rc) return rc; }
  KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + tBytes, ctx->knzAux.p + tBytes, (size_t)nn * 32, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  return 0;
}
// The faults of single streams of a many-stream reading call: code[s], and the text of the first failing stream in stream order,
// whichever step of the call finds it.
struct KnzStreamFaults {
  std::vector<int> code; int first; char text[256];
  explicit KnzStreamFaults(int ns) : code((size_t)ns, 0), first(-1) { text[0] = 0; }
  void fail(int s, int c, const char* call, const char* why) {
    code[(size_t)s] = c;
    if (first >= 0 && first < s) return;
    first = s;
    snprintf(text, sizeof(text), "%s: stream %d: %s (%d)", call, s, why, c);
  }
  void tell(kz_ctx* ctx) const { if (first >= 0) snprintf(ctx->err, sizeof(ctx->err), "%s", text); }
};
}  // namespace

// kz_knz_index_device for N streams: the heads in one copy (k_knz_heads) and the host's header parse, then decompress_group's two walk
// passes with a lane per stream (k_knz_walk_many): the count pass, and the fill pass with the exclusive scan of the counts as the base.
// Three launches and three waits whatever nStreams is.  Of a call whose cap is below the total only the entries below cap are filled.
extern "C" int64_t kz_knz_index_many_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams,
                                            uint64_t* transformType, uint32_t* entropyType, int32_t* blockSize, int64_t* inputSize, int32_t* checksumBits,
                                            int32_t* status, int64_t* indexFirst, int64_t* blockBitOff, int64_t* blockBits, int64_t cap) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_many_src_args(d_src, srcOff, srcLen, nStreams); if (rc) return rc; }
  if (nStreams == 0) return 0;
  if (!status || !indexFirst || cap < 0 || (cap > 0 && (!blockBitOff || !blockBits))) return -KZ_ERR_INVALID_PARAM;
  KZ_HIP(hipSetDevice(ctx->device));
  const int ns = nStreams;
  const char* call = "kz_knz_index_many_device";
  const int maxBlocks = 0x7FFFFFFF - 16384;                        // kz_knz_index_device's bound on a stream's blocks
  KnzStreamFaults F(ns);
  const size_t tBytes = kz_align((size_t)ns * sizeof(KnzSrc), 64);
  { const int rc = knz_tables(ctx, tBytes + (size_t)ns * 32); if (rc) return rc; }
  std::vector<int32_t> ids((size_t)ns);
  for (int s = 0; s < ns; s++) ids[(size_t)s] = s;
  { const int rc = knz_many_heads(ctx, d_src, srcOff, srcLen, ids.data(), ns, tBytes); if (rc) return rc; }
  KnzSrc* t = (KnzSrc*)ctx->knzPin.p;
  for (int s = 0; s < ns; s++) {
    t[s].maxCount = 0;                                             // (a stream with a fault is not walked)
    if (srcLen[s] < 20) { F.fail(s, -KZ_ERR_INVALID_FILE, call, "shorter than a stream header"); continue; }
    HostBitsIn bs{ctx->knzPin.p + tBytes + (size_t)s * 32, (uint64_t)std::min<int64_t>(srcLen[s], 26) * 8, 0, false};
    KnzHeader h;
    char why[96] = "";
    const int hrc = read_stream_header(bs, h, why, sizeof(why));
    if (hrc) { F.fail(s, hrc, call, why[0] ? why : "not a stream header"); continue; }
    knz_header_out(h, transformType ? transformType + s : nullptr, entropyType ? entropyType + s : nullptr, blockSize ? blockSize + s : nullptr,
                   inputSize ? inputSize + s : nullptr, checksumBits ? checksumBits + s : nullptr);
    t[s].startBit = (int64_t)bs.pos; t[s].maxCount = maxBlocks;
  }
  // ---- count pass (cap = 0: res only) ----
  const KnzSrc* d_t = (const KnzSrc*)ctx->knzAux.p;
  KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, t, (size_t)ns * sizeof(KnzSrc), hipMemcpyHostToDevice, ctx->stream));
  { const int rc = kz_knz_walk_many(ctx, d_src, d_t, ns, nullptr, nullptr, nullptr, (int64_t*)(ctx->knzAux.p + tBytes)); if (rc) return rc; }
  KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + tBytes, ctx->knzAux.p + tBytes, (size_t)ns * 24, hipMemcpyDeviceToHost, ctx->stream));
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  int64_t E = 0;
  {
    const int64_t* res = (const int64_t*)(ctx->knzPin.p + tBytes);
    for (int s = 0; s < ns; s++) {
      indexFirst[s] = E;
      if (F.code[(size_t)s]) { status[s] = F.code[(size_t)s]; continue; }
      const int64_t cnt = res[3 * s], why = res[3 * s + 2];
      if (cnt < 0 || cnt > maxBlocks) { snprintf(ctx->err, sizeof(ctx->err), "knz walk: bad count"); return -KZ_ERR_DEVICE; }
      if (why == KNZ_WALK_PREFIX || why == KNZ_WALK_PAYLOAD) F.fail(s, -KZ_ERR_READ_FILE, call, "a block does not fit in the stream");
      else if (why != KNZ_WALK_END) F.fail(s, -KZ_ERR_INVALID_FILE, call, "too many blocks");
      status[s] = F.code[(size_t)s] ? F.code[(size_t)s] : (int32_t)cnt;
      if (!F.code[(size_t)s]) E += cnt;
    }
    indexFirst[ns] = E;
  }
  // ---- fill pass: stream s's entries from index indexFirst[s] on, those below cap ----
  const int64_t M = std::min(E, cap);
  if (M > 0) {
    std::vector<KnzSrc> keep(t, t + ns);                           // (the tables may move when they grow)
    const size_t outBytes = (size_t)ns * 24 + (size_t)M * 24;
    { const int rc = knz_tables(ctx, tBytes + outBytes); if (rc) return rc; }
    t = (KnzSrc*)ctx->knzPin.p;
    for (int s = 0; s < ns; s++) {
      t[s] = keep[(size_t)s];
      t[s].base = indexFirst[s];
      t[s].maxCount = status[s] > 0 ? status[s] : 0;
      t[s].cap = (int32_t)std::max<int64_t>(0, std::min<int64_t>(t[s].maxCount, M - indexFirst[s]));
    }
    const KnzTable T(ctx, M, tBytes, (size_t)ns * 24);             // behind the KnzSrc entries: res[3 ns], then off[M], bits[M], hdr[M]
    KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, t, (size_t)ns * sizeof(KnzSrc), hipMemcpyHostToDevice, ctx->stream));
    { const int rc = kz_knz_walk_many(ctx, d_src, (const KnzSrc*)ctx->knzAux.p, ns, T.d_off(), T.d_bits(), T.d_hdr(), T.d_head()); if (rc) return rc; }
    KZ_HIP(hipMemcpyAsync(T.pin, T.dev, T.bytes(2), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
    kz_ktimer_flush(ctx);
    for (int s = 0; s < ns; s++)                                   // the same streams, walked twice: the same counts
      if (status[s] > 0 && T.head()[3 * s] != status[s]) { snprintf(ctx->err, sizeof(ctx->err), "knz walk: the fill pass counts other blocks than the count pass"); return -KZ_ERR_DEVICE; }
    memcpy(blockBitOff, T.off(), (size_t)M * 8);
    memcpy(blockBits, T.bits(), (size_t)M * 8);
  }
  F.tell(ctx);
  return E;
}


// =================================================================================================
// indexed reads: blocks of a stream by their (bit offset, bit length) pairs, as kz_knz_index / kz_knz_index_device return them, in
// any order.  No walk: every pair is checked against the stream on its own (k_knz_check), which makes the call memory safe for any
// index and brings the block-header bytes for the prechecks; it does not prove that a pair lies on the chain of prefixes that
// starts behind the stream header.
// The indexed read, the byte-addressed read and the byte-addressed write share three steps, each written once here: the open
// (knz_open_device), the check of every entry the call uses, and the decode of a chunk.  kz_stream.hip has the same three for host memory.
namespace {
// What entry i of a call's list is: its number in the caller's index (-1: an entry the call does not look at) and where its
// block-header word is kept for the prechecks (null: nowhere).
struct KnzEntry { int64_t k; uint64_t* hdr; };
// Every entry the call uses against the stream (k_knz_check), T.cap entries per launch, before anything is unpacked: entry(i) for
// i < count, called once each and in order.  The code and the text of the first entry that does not match, or 0.
template <class F> int knz_check_entries(kz_ctx* ctx, const KnzTable& T, const uint8_t* d_src, int64_t n, const KnzPlan& P, const int64_t* blockBitOff,
                                         const int64_t* blockBits, int64_t count, F entry) {
  std::vector<KnzEntry> e((size_t)T.cap);
  for (int64_t b0 = 0; b0 < count; b0 += T.cap) {
    const int cnt = (int)std::min<int64_t>(T.cap, count - b0);
    for (int i = 0; i < cnt; i++) {
      e[i] = entry(b0 + i);
      T.off()[i] = e[i].k < 0 ? 0 : blockBitOff[e[i].k]; T.bits()[i] = e[i].k < 0 ? 0 : blockBits[e[i].k];
    }
    KZ_HIP(hipMemcpyAsync(T.d_off(), T.off(), (size_t)cnt * 8, hipMemcpyHostToDevice, ctx->stream));
    KZ_HIP(hipMemcpyAsync(T.d_bits(), T.bits(), (size_t)cnt * 8, hipMemcpyHostToDevice, ctx->stream));
    { const int rc = kz_knz_check(ctx, d_src, n, P.hdrEnd, T.d_off(), T.d_bits(), cnt, T.d_hdr(), T.d_bad()); if (rc) return rc; }
    KZ_HIP(hipMemcpyAsync(T.hdr(), T.d_hdr(), (size_t)cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(hipMemcpyAsync(T.bad(), T.d_bad(), (size_t)cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));                      // the pinned table is the next launch's
    kz_ktimer_flush(ctx);
    for (int i = 0; i < cnt; i++) {
      if (e[i].k < 0) continue;
      if (T.bad()[i]) return indexed_mismatch(ctx, e[i].k);
      if (e[i].hdr) *e[i].hdr = T.hdr()[i];
    }
  }
  return 0;
}
// A chunk of cnt <= T.cap entries (off[i], W[i]) with their block-header words hdrs[i]: the prechecks on the host into res[], the
// unpack of the entries that pass into staging rows (ctx->devIn[0], P.iS apart), their decode into rows `stride` apart at d_out.  An
// entry with leftOut[i] (may be null) is not looked at: its res[i] is the caller's, with a status that is not 0.  A chunk in which
// nothing passes launches nothing.
// The rows may come from one stream or from many of one header (P: what that header gives; its hdrEnd and its batch are not looked
// at): bytesOf(i) = the bytes of row i's stream, put(i, off, bits) enters the row in the caller's pinned table (bits == 0: a row of
// no bits, nothing of it is unpacked), unpack(maxBytes) sends the table up and launches the unpack into ctx->devIn[0].
template <class N, class E, class U>
int knz_chunk_decode_rows(kz_ctx* ctx, const KnzPlan& P, N bytesOf, const int64_t* off, const int64_t* W, const uint64_t* hdrs, const uint8_t* leftOut, int cnt,
                          E put, U unpack, uint8_t* d_out, int64_t stride, kz_block_result* res) {
  int64_t maxBytes = 0;
  for (int i = 0; i < cnt; i++) {
    if (leftOut && leftOut[i]) { put(i, off[i], (int64_t)0); continue; }
    const int rc = knz_check_walked(hdrs[i], (uint64_t)W[i], (uint64_t)off[i], (uint64_t)bytesOf(i) * 8, P);
    memset(&res[i], 0, sizeof(res[i]));
    res[i].bits = W[i]; res[i].status = rc;
    put(i, off[i], rc ? (int64_t)0 : W[i]);
    if (!rc) maxBytes = std::max<int64_t>(maxBytes, (W[i] + 7) >> 3);
  }
  if (maxBytes == 0) return 0;
  { const int rc = kz_stage_reserve(ctx, ctx->devIn[0], (size_t)cnt * P.iS, false); if (rc) return rc; }
  { const int rc = unpack(maxBytes); if (rc) return rc; }
  { const int rc = indexed_decode_runs(ctx, P, ctx->devIn[0].p, W, cnt, d_out, stride, res, KZ_MEM_DEVICE); if (rc) return rc; }
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));                        // the pinned table is the caller's again
  kz_ktimer_flush(ctx);
  return 0;
}
// the rows of one stream d_src[0 .. n): the table is T's (off, bits) columns, the unpack k_knz_unpack
int knz_chunk_decode(kz_ctx* ctx, const KnzTable& T, const uint8_t* d_src, int64_t n, const KnzPlan& P, const int64_t* off, const int64_t* W, const uint64_t* hdrs,
                     const uint8_t* leftOut, int cnt, uint8_t* d_out, int64_t stride, kz_block_result* res) {
  return knz_chunk_decode_rows(ctx, P, [&](int) { return n; }, off, W, hdrs, leftOut, cnt,
    [&](int i, int64_t o, int64_t bits) { T.off()[i] = o; T.bits()[i] = bits; },
    [&](int64_t maxBytes) -> int {
      KZ_HIP(hipMemcpyAsync(T.d_off(), T.off(), (size_t)cnt * 8, hipMemcpyHostToDevice, ctx->stream));
      KZ_HIP(hipMemcpyAsync(T.d_bits(), T.bits(), (size_t)cnt * 8, hipMemcpyHostToDevice, ctx->stream));
      return kz_knz_unpack(ctx, d_src, n, T.d_off(), T.d_bits(), cnt, maxBytes, ctx->devIn[0].p, P.iS);
    }, d_out, stride, res);
}
}  // namespace

extern "C" int32_t kz_decode_indexed_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, int32_t nBlocks,
                                            uint8_t* d_dst, int64_t dstStride, kz_block_result* results) {
  if (!ctx || !d_src || n < 0 || nBlocks < 0 || (nBlocks > 0 && (!blockBitOff || !blockBits || !d_dst || !results))) return -KZ_ERR_INVALID_PARAM;
  KZ_HIP(hipSetDevice(ctx->device));
  KnzPlan P;
  { int rc = knz_open_device(ctx, d_src, n, P); if (!rc) rc = indexed_stride(ctx, dstStride, P); if (rc) return rc; }
  if (nBlocks == 0) return 0;
  ChecksumScope chk(ctx, P.h.chkKind);
  const int CH = (int)std::min<int64_t>(knz_chunk_blocks(ctx, P.h.blockSize), nBlocks);
  // the chunk's tables, pinned and in HBM: 64 spare bytes, then off[CH], bits[CH], hdr[CH], bad[CH]
  { const int rc = knz_tables(ctx, (size_t)CH * 32); if (rc) return rc; }
  const KnzTable T(ctx, CH);
  std::vector<uint64_t> hdrs((size_t)nBlocks);                     // the block-header bytes stay on the host for the chunks' prechecks
  { const int rc = knz_check_entries(ctx, T, d_src, n, P, blockBitOff, blockBits, nBlocks, [&](int64_t i) { return KnzEntry{i, &hdrs[(size_t)i]}; }); if (rc) return rc; }
  for (int64_t b0 = 0; b0 < nBlocks; b0 += CH) {
    const int cnt = (int)std::min<int64_t>(CH, nBlocks - b0);
    const int rc = knz_chunk_decode(ctx, T, d_src, n, P, blockBitOff + b0, blockBits + b0, &hdrs[(size_t)b0], nullptr, cnt, d_dst + b0 * dstStride, dstStride, results + b0);
    if (rc) return rc;
  }
  return 0;
}


// =================================================================================================
// splice: a new stream out of blocks of existing streams, all in HBM (kz_knz_splice_device).  The plan is the host form's
// (kz_knz_host.h) on the first bytes of every source (k_knz_heads, one copy); every piece is checked against its own source on the
// device (k_knz_check_many) before the layout is made and the room decided, and only then is anything written: the stream header,
// and per chunk of pieces one k_knz_splice launch that copies payload bits straight from the sources to their place in d_dst.
extern "C" int64_t kz_knz_splice_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff, const int64_t* srcLen, int32_t nSrc,
                                        const int32_t* pieceSrc, const int64_t* pieceBitOff, const int64_t* pieceBits, int32_t nPieces,
                                        int64_t inputSize, uint8_t* d_dst, int64_t dstCap) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_splice_args(d_src, srcOff, srcLen, nSrc, pieceSrc, pieceBitOff, pieceBits, nPieces, inputSize, d_dst, dstCap); if (rc) return rc; }
  KZ_HIP(hipSetDevice(ctx->device));
  // ---- the first bytes of every source in one table, one copy; the headers are parsed and compared on the host ----
  KnzSplice P;
  std::vector<int64_t> hdrEnd((size_t)nSrc), pre((size_t)nPieces + 1);
  {
    const size_t tBytes = kz_align((size_t)nSrc * sizeof(KnzSrc), 64), headBytes = (size_t)nSrc * 32;
    { const int rc = knz_tables(ctx, tBytes + headBytes); if (rc) return rc; }
    KnzSrc* t = (KnzSrc*)ctx->knzPin.p;
    for (int s = 0; s < nSrc; s++) t[s] = KnzSrc{srcOff[s], srcLen[s], 0, 0, 0, 0};
    KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, t, (size_t)nSrc * sizeof(KnzSrc), hipMemcpyHostToDevice, ctx->stream));
    { const int rc = kz_knz_heads(ctx, d_src, (const KnzSrc*)ctx->knzAux.p, nSrc, ctx->knzAux.p + tBytes); if (rc) return rc; }
    KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + tBytes, ctx->knzAux.p + tBytes, headBytes, hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
    kz_ktimer_flush(ctx);
    std::vector<int64_t> headOff((size_t)nSrc);
    for (int s = 0; s < nSrc; s++) headOff[s] = (int64_t)s * 32;
    const int rc = knz_splice_sources(ctx->knzPin.p + tBytes, headOff.data(), srcLen, nSrc, P, hdrEnd.data(), ctx->err, sizeof(ctx->err));
    if (rc) return rc;
  }
  // ---- chunks of pieces: a table entry per piece (pinned and in HBM), behind it the check's verdicts ----
  const int CH = (int)std::max<int64_t>(1, std::min<int64_t>(knz_chunk_blocks(ctx, P.h.blockSize), nPieces));
  const size_t pcBytes = kz_align((size_t)CH * sizeof(KnzPiece), 64);
  { const int rc = knz_tables(ctx, pcBytes + (size_t)CH * sizeof(int32_t)); if (rc) return rc; }
  KnzPiece* pc = (KnzPiece*)ctx->knzPin.p;
  const KnzPiece* d_pc = (const KnzPiece*)ctx->knzAux.p;
  auto fill = [&](int64_t b0, int cnt, bool placed) {
    for (int i = 0; i < cnt; i++) {
      const int64_t k = b0 + i;
      const int s = pieceSrc[k];
      pc[i] = KnzPiece{placed ? pre[k] + 5 + knz_prefix_width((uint64_t)pieceBits[k]) : 0, pieceBits[k], srcOff[s], srcLen[s], pieceBitOff[k], hdrEnd[s]};
    }
  };
  for (int64_t b0 = 0; b0 < nPieces; b0 += CH) {                  // every piece against its own source, before a bit is copied
    const int cnt = (int)std::min<int64_t>(CH, nPieces - b0);
    fill(b0, cnt, false);
    const int32_t* bad = (const int32_t*)(ctx->knzPin.p + pcBytes);
    KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, pc, (size_t)cnt * sizeof(KnzPiece), hipMemcpyHostToDevice, ctx->stream));
    { const int rc = kz_knz_check_many(ctx, d_src, d_pc, cnt, (int32_t*)(ctx->knzAux.p + pcBytes)); if (rc) return rc; }
    KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + pcBytes, ctx->knzAux.p + pcBytes, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));
    kz_ktimer_flush(ctx);
    for (int i = 0; i < cnt; i++) if (bad[i]) return knz_splice_mismatch(b0 + i, ctx->err, sizeof(ctx->err));
  }
  if (knz_splice_layout(pieceBits, nPieces, inputSize, dstCap, P, pre.data())) {
    snprintf(ctx->err, sizeof(ctx->err), "kz_knz_splice_device: destination too small");
    return -KZ_ERR_WRITE_FILE;
  }
  // ---- the copy: a launch per chunk owns the bits from its first prefix to the next chunk's (the last: to behind the end marker) ----
  for (int64_t b0 = 0; b0 < nPieces || b0 == 0; b0 += CH) {
    const int cnt = (int)std::min<int64_t>(CH, nPieces - b0);
    fill(b0, cnt, true);
    if (cnt) KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, pc, (size_t)cnt * sizeof(KnzPiece), hipMemcpyHostToDevice, ctx->stream));
    const bool last = b0 + cnt >= nPieces;
    { const int rc = kz_knz_splice_launch(ctx, d_src, d_pc, cnt, d_dst, pre[b0], last ? P.endBit : pre[b0 + cnt]); if (rc) return rc; }
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));                      // the pinned table is the next chunk's
    kz_ktimer_flush(ctx);
    if (last) break;
  }
  { const int hrc = knz_put_header(ctx, P.hdr, P.hdrBits >> 3, d_dst); if (hrc) return hrc; }
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  return (P.endBit + 7) >> 3;
}


// =================================================================================================
// byte-addressed reads: many ranges [off, off + len) of the original data in one call, stream and destination in HBM
// (kz_read_bytes_device).  The plan is the host form's (kz_knz_host.h: the distinct covering blocks, and the range x block segments
// grouped by chunk); the shared steps of the indexed calls (above the indexed read) do the open, the check of every index entry the
// plan uses and, per chunk of blocks, the decode into staging rows; the read's own is one k_knz_read launch that copies the chunk's
// segments from the rows to their places in d_dst.
namespace {
const int KNZ_READ_LAUNCH = 1 << 20;                               // segments per k_knz_read launch: bounds the table at 32 MiB
}
extern "C" int64_t kz_read_bytes_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, const int64_t* blockByteOff,
                                        int32_t nIndex, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges, uint8_t* d_dst, int64_t dstCap, int64_t* got) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_read_args(d_src, n, blockBitOff, blockBits, nIndex, rangeOff, rangeLen, nRanges, d_dst, dstCap, got); if (rc) return rc; }
  KZ_HIP(hipSetDevice(ctx->device));
  KnzPlan P;
  { const int rc = knz_open_device(ctx, d_src, n, P); if (rc) return rc; }
  const int32_t blockSize = P.h.blockSize;
  { const int rc = knz_table_refusal(ctx, "kz_read_bytes_device", blockByteOff, nIndex, blockSize); if (rc) return rc; }
  const int64_t total = knz_read_total(rangeLen, nRanges, dstCap);
  if (total < 0) { snprintf(ctx->err, sizeof(ctx->err), "kz_read_bytes_device: destination too small"); return total; }
  if (nRanges == 0) return 0;
  const int CH = knz_chunk_blocks(ctx, blockSize);
  KnzReadPlan R;
  knz_read_plan(blockByteOff, nIndex, blockSize, rangeOff, rangeLen, nRanges, CH, (int)((uintptr_t)d_dst & 15), R);
  for (int32_t i = 0; i < nRanges; i++) got[i] = 0;
  const int64_t nb = (int64_t)R.blocks.size();
  if (nb == 0) return total;
  ChecksumScope chk(ctx, P.h.chkKind);
  const int cmax = (int)std::min<int64_t>(CH, nb);
  int64_t segMax = 0;
  for (size_t c = 0; c + 1 < R.first.size(); c++) segMax = std::max(segMax, std::min<int64_t>(R.first[c + 1] - R.first[c], KNZ_READ_LAUNCH));
  // the chunk's tables, pinned and in HBM: 64 spare bytes, then off[cmax], bits[cmax], hdr[cmax], bad[cmax]; the segment table of a
  // launch (32 bytes per segment) takes their place when the chunk has been decoded
  { const int rc = knz_tables(ctx, std::max((size_t)cmax * 32, (size_t)segMax * sizeof(KnzReadSeg))); if (rc) return rc; }
  const KnzTable T(ctx, cmax);
  std::vector<uint64_t> hdrs((size_t)nb);
  { const int rc = knz_check_entries(ctx, T, d_src, n, P, blockBitOff, blockBits, nb, [&](int64_t i) { return KnzEntry{R.blocks[(size_t)i], &hdrs[(size_t)i]}; }); if (rc) return rc; }
  // ---- chunks of blocks, ascending: the decode into staging rows blockSize apart, then the copy of the chunk's segments ----
  std::vector<kz_block_result> res((size_t)cmax);
  std::vector<int64_t> W((size_t)cmax), off((size_t)cmax);
  { const int rc = kz_stage_reserve(ctx, ctx->devOut[0], (size_t)cmax * (size_t)blockSize, false); if (rc) return rc; }
  for (int64_t b0 = 0, c = 0; b0 < nb; b0 += CH, c++) {
    const int cnt = (int)std::min<int64_t>(CH, nb - b0);
    knz_chunk_entries(&R.blocks[(size_t)b0], nullptr, cnt, blockBitOff, blockBits, off.data(), W.data());
    // (behind it the pinned table becomes the segments')
    { const int rc = knz_chunk_decode(ctx, T, d_src, n, P, off.data(), W.data(), &hdrs[(size_t)b0], nullptr, cnt, ctx->devOut[0].p, blockSize, res.data()); if (rc) return rc; }
    knz_read_settle(R, c, CH, blockByteOff, nIndex, blockSize, res.data(), got);
    for (int64_t s0 = R.first[(size_t)c]; s0 < R.first[(size_t)c + 1]; s0 += KNZ_READ_LAUNCH) {
      const int ns = (int)std::min<int64_t>(KNZ_READ_LAUNCH, R.first[(size_t)c + 1] - s0);
      const int64_t uEnd = s0 + ns < R.first[(size_t)c + 1] ? R.segs[(size_t)(s0 + ns)].unit0 : R.units[(size_t)c];
      if (ctx->sw.readScatter) {                                   // the yardstick: the same segments through the ragged copy, a workgroup column each
        KnzCopy* t = (KnzCopy*)(ctx->knzPin.p + 64);
        int64_t maxLen = 0;
        for (int i = 0; i < ns; i++) {
          const KnzReadSeg& g = R.segs[(size_t)(s0 + i)];
          t[i] = KnzCopy{(int64_t)g.slot * blockSize + g.off, g.dst, g.len};
          maxLen = std::max<int64_t>(maxLen, g.len);
        }
        KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, t, (size_t)ns * sizeof(KnzCopy), hipMemcpyHostToDevice, ctx->stream));
        { const int rc = kz_knz_scatter(ctx, ctx->devOut[0].p, (const KnzCopy*)(ctx->knzAux.p + 64), ns, maxLen, d_dst); if (rc) return rc; }
      } else {
        memcpy(ctx->knzPin.p + 64, &R.segs[(size_t)s0], (size_t)ns * sizeof(KnzReadSeg));
        KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, ctx->knzPin.p + 64, (size_t)ns * sizeof(KnzReadSeg), hipMemcpyHostToDevice, ctx->stream));
        const int rc = kz_knz_read(ctx, ctx->devOut[0].p, blockSize, blockSize, (const KnzReadSeg*)(ctx->knzAux.p + 64), ns, d_dst, R.segs[(size_t)s0].unit0, uEnd - R.segs[(size_t)s0].unit0);
        if (rc) return rc;
      }
      KZ_HIP(kz_stream_sync(ctx, ctx->stream));                    // the pinned table is the next launch's
      kz_ktimer_flush(ctx);
    }
  }
  return total;
}

// kz_read_bytes_device for ranges of N streams in one call.  The open is the many-stream decoder's (k_knz_heads over the streams that
// some range names, one copy, parsed here); the plan is the merged one (kz_knz_host.h: every stream's distinct covering blocks in one
// list of rows by header group, stream and block, cut into chunks inside a group); every used entry is checked against its own stream
// (k_knz_check_rows, which brings the block-header words); a chunk is the indexed calls' decode step over rows of many streams
// (k_knz_unpack_many), the per-stream settle and the read's own copy launch.  A fault that ends the single-stream call ends only its
// stream here: the stream leaves the plan, and the others are planned as if it were not there.
namespace {
const int KNZ_CHECK_LAUNCH = 1 << 18;                              // entries per k_knz_check_rows launch: bounds its table at 14 MiB
}
extern "C" int64_t kz_read_bytes_many_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams,
                                             const int64_t* indexFirst, const int64_t* blockBitOff, const int64_t* blockBits,
                                             const int64_t* tableFirst, const int64_t* blockByteOff,
                                             const int32_t* rangeStream, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges,
                                             uint8_t* d_dst, int64_t dstCap, int64_t* got, int32_t* streamStatus) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  {
    const int rc = knz_read_many_args(d_src, srcOff, srcLen, nStreams, indexFirst, blockBitOff, blockBits, tableFirst, blockByteOff, rangeStream, rangeOff, rangeLen,
                                      nRanges, d_dst, dstCap, got);
    if (rc) return rc;
  }
  const char* call = "kz_read_bytes_many_device";
  const int64_t total = knz_read_total(rangeLen, nRanges, dstCap);
  if (total < 0) { snprintf(ctx->err, sizeof(ctx->err), "%s: destination too small", call); return total; }
  if (streamStatus) for (int s = 0; s < nStreams; s++) streamStatus[s] = 0;
  if (nRanges == 0) return 0;
  KZ_HIP(hipSetDevice(ctx->device));
  const int ns = nStreams;
  // ---- the streams that some range names, ascending; their heads in one copy; per stream the single call's open and table check ----
  std::vector<int32_t> ids;
  {
    std::vector<uint8_t> named((size_t)ns, 0);
    for (int32_t i = 0; i < nRanges; i++) named[(size_t)rangeStream[i]] = 1;
    for (int s = 0; s < ns; s++) if (named[(size_t)s]) ids.push_back(s);
  }
  const int nn = (int)ids.size();
  KnzStreamFaults F(ns);
  std::vector<KnzManyStreamIn> st((size_t)ns, KnzManyStreamIn{false, -1, 0, 0, nullptr});
  std::vector<KnzPlan> plan((size_t)ns);
  {
    const size_t tBytes = kz_align((size_t)nn * sizeof(KnzSrc), 64);
    { const int rc = knz_tables(ctx, tBytes + (size_t)nn * 32); if (rc) return rc; }
    { const int rc = knz_many_heads(ctx, d_src, srcOff, srcLen, ids.data(), nn, tBytes); if (rc) return rc; }
    for (int k = 0; k < nn; k++) {
      const int s = ids[(size_t)k];
      HostBitsIn bs{ctx->knzPin.p + tBytes + (size_t)k * 32, (uint64_t)std::min<int64_t>(srcLen[s], 26) * 8, 0, false};
      KnzHeader h;
      char why[96] = "";
      const int hrc = read_stream_header(bs, h, why, sizeof(why));
      if (hrc) { F.fail(s, hrc, call, why[0] ? why : "not a stream header"); continue; }
      plan[(size_t)s] = knz_plan(ctx, h, srcLen[s], (int64_t)bs.pos);
      KnzManyStreamIn& S = st[(size_t)s];
      S.nIndex = (int32_t)(indexFirst[s + 1] - indexFirst[s]);
      S.blockSize = h.blockSize;
      S.B = (tableFirst && tableFirst[s] >= 0) ? blockByteOff + tableFirst[s] : nullptr;
      if (knz_read_table(S.B, S.nIndex, S.blockSize)) { F.fail(s, -KZ_ERR_INVALID_PARAM, call, "blockByteOff is not a table of block starts"); continue; }
      S.use = true;
    }
  }
  KnzManyReadPlan R;
  std::vector<KnzPlan> groups;                                     // a group's plan: its first stream's (the header's four fields, the staging row)
  std::vector<int> chunkBlocks;
  std::vector<uint64_t> hdrs;
  // ---- the plan, and every entry it uses against its own stream before anything is unpacked.  A stream with an entry that does not
  //      match leaves the plan, which is then made again without it (and checked again: the rows have other places) ----
  for (;;) {
    groups.clear(); chunkBlocks.clear();
    for (int k = 0; k < nn; k++) {
      const int s = ids[(size_t)k];
      if (!st[(size_t)s].use) continue;
      const KnzHeader& h = plan[(size_t)s].h;
      size_t g = 0;
      for (; g < groups.size(); g++) if (groups[g].h.transformType == h.transformType && groups[g].h.entropyType == h.entropyType && groups[g].h.blockSize == h.blockSize && groups[g].h.chkKind == h.chkKind) break;
      if (g == groups.size()) { groups.push_back(plan[(size_t)s]); chunkBlocks.push_back(knz_chunk_blocks(ctx, h.blockSize)); }
      st[(size_t)s].group = (int32_t)g;
    }
    knz_read_many_plan(st.data(), ns, rangeStream, rangeOff, rangeLen, nRanges, chunkBlocks.data(), (int)((uintptr_t)d_dst & 15), R);
    const int64_t nr = (int64_t)R.rowStream.size();
    hdrs.assign((size_t)nr, 0);
    const int CK = (int)std::min<int64_t>(KNZ_CHECK_LAUNCH, nr);
    const size_t rowBytes = kz_align((size_t)CK * sizeof(KnzCheckRow), 64);
    { const int rc = knz_tables(ctx, rowBytes + (size_t)CK * 16); if (rc) return rc; }
    bool dropped = false;
    for (int64_t r0 = 0; r0 < nr; r0 += CK) {
      const int cnt = (int)std::min<int64_t>(CK, nr - r0);
      KnzCheckRow* t = (KnzCheckRow*)ctx->knzPin.p;
      for (int i = 0; i < cnt; i++) {
        const int s = R.rowStream[(size_t)(r0 + i)];
        const int64_t e = indexFirst[s] + R.rowBlock[(size_t)(r0 + i)];
        t[i] = KnzCheckRow{srcOff[s], srcLen[s], blockBitOff[e], blockBits[e], plan[(size_t)s].hdrEnd};
      }
      uint64_t* d_hdr = (uint64_t*)(ctx->knzAux.p + rowBytes);
      KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, t, (size_t)cnt * sizeof(KnzCheckRow), hipMemcpyHostToDevice, ctx->stream));
      { const int rc = kz_knz_check_rows(ctx, d_src, (const KnzCheckRow*)ctx->knzAux.p, cnt, d_hdr, (int64_t*)(d_hdr + CK)); if (rc) return rc; }
      KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + rowBytes, ctx->knzAux.p + rowBytes, (size_t)CK * 8 + (size_t)cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
      KZ_HIP(kz_stream_sync(ctx, ctx->stream));                    // the pinned table is the next launch's
      kz_ktimer_flush(ctx);
      const uint64_t* hw = (const uint64_t*)(ctx->knzPin.p + rowBytes);
      const int64_t* bad = (const int64_t*)(hw + CK);
      for (int i = 0; i < cnt; i++) {
        const int s = R.rowStream[(size_t)(r0 + i)];
        hdrs[(size_t)(r0 + i)] = hw[i];
        if (!bad[i] || !st[(size_t)s].use) continue;               // (of a stream's bad entries the first in block order is named)
        char why[96];
        snprintf(why, sizeof(why), "index entry %d does not match the stream", (int)R.rowBlock[(size_t)(r0 + i)]);
        F.fail(s, -KZ_ERR_INVALID_PARAM, call, why);
        st[(size_t)s].use = false;
        dropped = true;
      }
    }
    if (!dropped) break;
  }
  for (int32_t i = 0; i < nRanges; i++) got[i] = F.code[(size_t)rangeStream[i]];   // 0, or the fault of the range's stream
  if (streamStatus) for (int s = 0; s < ns; s++) streamStatus[s] = F.code[(size_t)s];
  F.tell(ctx);
  const int64_t nChunks = (int64_t)R.chunkGroup.size();
  if (nChunks == 0) return total;
  // ---- staging and tables for the largest chunk ----
  int cmax = 0;
  int64_t segMax = 0;
  size_t inMax = 0, outMax = 0;
  for (int64_t c = 0; c < nChunks; c++) {
    const int cnt = (int)(R.chunkRow[(size_t)c + 1] - R.chunkRow[(size_t)c]);
    const KnzPlan& G = groups[(size_t)R.chunkGroup[(size_t)c]];
    cmax = std::max(cmax, cnt);
    inMax = std::max(inMax, (size_t)cnt * (size_t)G.iS);
    outMax = std::max(outMax, (size_t)cnt * (size_t)G.h.blockSize);
    segMax = std::max(segMax, std::min<int64_t>(R.first[(size_t)c + 1] - R.first[(size_t)c], KNZ_READ_LAUNCH));
  }
  {
    int rc = kz_stage_reserve(ctx, ctx->devIn[0], inMax, false);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->devOut[0], outMax, false);
    if (!rc) rc = knz_tables(ctx, std::max((size_t)cmax * sizeof(KnzRow), (size_t)segMax * sizeof(KnzReadSeg)));
    if (rc) return rc;
  }
  // ---- chunks: the decode of the chunk's rows under its group's header, the settle per stream, the copy of the chunk's segments ----
  ChecksumScope chk(ctx, ctx->checksum);                           // each chunk decodes under its own group's kind
  std::vector<kz_block_result> res((size_t)cmax);
  std::vector<int64_t> W((size_t)cmax), off((size_t)cmax);
  for (int64_t c = 0; c < nChunks; c++) {
    const int64_t r0 = R.chunkRow[(size_t)c];
    const int cnt = (int)(R.chunkRow[(size_t)c + 1] - r0);
    const KnzPlan& G = groups[(size_t)R.chunkGroup[(size_t)c]];
    const int32_t blockSize = G.h.blockSize;
    ctx->checksum = G.h.chkKind;
    for (int i = 0; i < cnt; i++) {
      const int s = R.rowStream[(size_t)(r0 + i)];
      const int64_t e = indexFirst[s] + R.rowBlock[(size_t)(r0 + i)];
      off[(size_t)i] = blockBitOff[e]; W[(size_t)i] = blockBits[e];
    }
    KnzRow* t = (KnzRow*)(ctx->knzPin.p + 64);
    // (behind it the pinned table becomes the segments')
    const int rc = knz_chunk_decode_rows(ctx, G, [&](int i) { return srcLen[R.rowStream[(size_t)(r0 + i)]]; }, off.data(), W.data(), &hdrs[(size_t)r0], nullptr, cnt,
      [&](int i, int64_t o, int64_t bits) { const int s = R.rowStream[(size_t)(r0 + i)]; t[i] = KnzRow{srcOff[s], srcLen[s], o, bits, (int64_t)i * G.iS}; },
      [&](int64_t maxBytes) -> int {
        KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, t, (size_t)cnt * sizeof(KnzRow), hipMemcpyHostToDevice, ctx->stream));
        return kz_knz_unpack_many(ctx, d_src, (const KnzRow*)(ctx->knzAux.p + 64), cnt, maxBytes, ctx->devIn[0].p);
      }, ctx->devOut[0].p, blockSize, res.data());
    if (rc) return rc;
    for (int i = 0; i < cnt;) {                                    // the rows of a stream lie side by side
      const int s = R.rowStream[(size_t)(r0 + i)];
      int j = i + 1;
      while (j < cnt && R.rowStream[(size_t)(r0 + j)] == s) j++;
      knz_read_settle_blocks(&R.rowBlock[(size_t)(r0 + i)], j - i, st[(size_t)s].B, st[(size_t)s].nIndex, blockSize, res.data() + i);
      i = j;
    }
    knz_read_settle_segs(R.segs.data(), R.first[(size_t)c], R.first[(size_t)c + 1], res.data(), got);
    for (int64_t s0 = R.first[(size_t)c]; s0 < R.first[(size_t)c + 1]; s0 += KNZ_READ_LAUNCH) {
      const int nseg = (int)std::min<int64_t>(KNZ_READ_LAUNCH, R.first[(size_t)c + 1] - s0);
      const int64_t uEnd = s0 + nseg < R.first[(size_t)c + 1] ? R.segs[(size_t)(s0 + nseg)].unit0 : R.units[(size_t)c];
      memcpy(ctx->knzPin.p + 64, &R.segs[(size_t)s0], (size_t)nseg * sizeof(KnzReadSeg));
      KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, ctx->knzPin.p + 64, (size_t)nseg * sizeof(KnzReadSeg), hipMemcpyHostToDevice, ctx->stream));
      const int rrc = kz_knz_read(ctx, ctx->devOut[0].p, blockSize, blockSize, (const KnzReadSeg*)(ctx->knzAux.p + 64), nseg, d_dst, R.segs[(size_t)s0].unit0, uEnd - R.segs[(size_t)s0].unit0);
      if (rrc) return rrc;
      KZ_HIP(kz_stream_sync(ctx, ctx->stream));                    // the pinned table is the next launch's
      kz_ktimer_flush(ctx);
    }
  }
  F.tell(ctx);                                                     // (a decode may have left a block's text there)
  return total;
}


// =================================================================================================
// byte-addressed writes: many ranges [off, off + len) of the original data replaced by new bytes in one call, stream, new bytes and
// the new stream in HBM (kz_write_bytes_device).  The plan is the host form's (kz_knz_host.h: later wins resolved into disjoint
// segments, the touched blocks, which of them are wholly covered).  The shared steps of the indexed calls (above the indexed read) do
// the open, the check of every index entry the call uses (a wholly covered block's is not looked at) and, per chunk of touched
// blocks, the decode into staging rows; the write's own are k_knz_write launches that patch the rows, kz_compress_device's batched
// encode of the rows, and the splice's copy (k_knz_splice) of every kept block since the previous chunk together with the recoded
// ones, laid out by knz_write_walk (kz_knz_host.h).  A piece's payload lies in
// d_src (kept) or in an encoder row (recoded): the launch's base is d_src, a row is named by its distance from it.
namespace {
const int KNZ_WRITE_LAUNCH = 1 << 20;                              // segments per k_knz_write launch: bounds the table at 32 MiB
}
extern "C" int64_t kz_write_bytes_device(kz_ctx* ctx, const uint8_t* d_src, int64_t n, const int64_t* blockBitOff, const int64_t* blockBits, const int64_t* blockByteOff,
                                         int32_t nIndex, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges, const uint8_t* d_data, int64_t dataLen,
                                         uint8_t* d_dst, int64_t dstCap, int64_t* newBitOff, int64_t* newBits) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  { const int rc = knz_write_args(d_src, n, blockBitOff, blockBits, nIndex, rangeOff, rangeLen, nRanges, d_data, dataLen, d_dst, dstCap, newBitOff, newBits); if (rc) return rc; }
  KZ_HIP(hipSetDevice(ctx->device));
  KnzPlan P;
  { const int rc = knz_open_device(ctx, d_src, n, P); if (rc) return rc; }
  const KnzHeader& h = P.h;
  const int32_t blockSize = h.blockSize;
  { const int rc = knz_table_refusal(ctx, "kz_write_bytes_device", blockByteOff, nIndex, blockSize); if (rc) return rc; }
  const int CH = knz_chunk_blocks(ctx, blockSize);
  KnzWritePlan R;
  { const int32_t bad = knz_write_plan(blockByteOff, nIndex, blockSize, rangeOff, rangeLen, nRanges, CH, KNZ_WRITE_LAUNCH, R); if (bad >= 0) return knz_write_behind(bad, ctx->err, sizeof(ctx->err)); }
  uint8_t nh[32];                                                  // the new stream's header: the old one's parameters and size
  HostBits hb{nh, 32, 0, false};
  write_stream_header(hb, h.transformType, (uint32_t)h.entropyType, blockSize, h.inputSize, h.chkKind);
  ChecksumScope chk(ctx, h.chkKind);
  BlockSizeScope scope(ctx, blockSize);
  const int64_t nb = (int64_t)R.blocks.size();
  const int cmax = (int)std::max<int64_t>(1, std::min<int64_t>(CH, nb));
  const int PL = (int)std::max<int64_t>(1, std::min<int64_t>(CH, nIndex));        // entries per check launch, pieces per copy launch: the splice's chunk
  const int64_t oS = kz_max_block_stream_bytes(blockSize);
  int64_t segMax = 0;
  for (size_t l = 0; l + 1 < R.cuts.size(); l++) segMax = std::max(segMax, R.cuts[l + 1] - R.cuts[l]);
  // the tables, pinned and in HBM, one after the other in the same place: the check's (off, bits, hdr, bad), a chunk's, the segments of
  // a patch launch, the pieces of a copy launch
  { const int rc = knz_tables(ctx, std::max(std::max((size_t)std::max(PL, cmax) * 32, (size_t)segMax * sizeof(KnzWriteSeg)), (size_t)PL * sizeof(KnzPiece))); if (rc) return rc; }
  // ---- every entry the call uses against the stream, before anything is unpacked: the kept blocks' and the decoded ones' ----
  std::vector<uint64_t> hdrs((size_t)nb);
  {
    int64_t ti = 0;                                               // the next touched block
    const int rc = knz_check_entries(ctx, KnzTable(ctx, PL), d_src, n, P, blockBitOff, blockBits, nIndex, [&](int64_t k) {
      if (ti >= nb || R.blocks[(size_t)ti] != k) return KnzEntry{k, nullptr};                          // a kept block
      uint64_t* keep = &hdrs[(size_t)ti];
      return R.covered[(size_t)ti++] ? KnzEntry{-1, nullptr} : KnzEntry{k, keep};                       // a wholly covered block's entry is not looked at
    });
    if (rc) return rc;
  }
  {
    int rc = kz_stage_reserve(ctx, ctx->devOut[0], (size_t)cmax * (size_t)blockSize, false);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->devOut[1], (size_t)cmax * (size_t)oS, false);
    if (rc) return rc;
  }
  uint8_t* rows = ctx->devOut[0].p;
  uint8_t* enc = ctx->devOut[1].p;
  if ((uintptr_t)rows & 15) { snprintf(ctx->err, sizeof(ctx->err), "kz_write_bytes_device: staging rows off a 16-byte boundary"); return -KZ_ERR_DEVICE; }   // (unit0 counts on it)
  auto tooSmall = [&]() { snprintf(ctx->err, sizeof(ctx->err), "kz_write_bytes_device: destination too small"); return (int64_t)-KZ_ERR_WRITE_FILE; };
  // blocks [k0, k1) of the new stream from bit `pos` on, in launches of PL pieces: the blocks t0 .. of the touched list (ascending) come
  // from the encoder's rows (eW: their bits), all others from where they lie in d_src; then tailBits zero bits.  knz_write_walk
  // (kz_knz_host.h) lays them out, first for the room, which is decided before a bit is written, then launch by launch.
  int64_t pos = (int64_t)hb.pos;
  auto emit = [&](int64_t k0, int64_t k1, int64_t t0, int64_t t1, const int64_t* eW, int tailBits) -> int64_t {
    KnzPiece* pc = (KnzPiece*)(ctx->knzPin.p + 64);
    int64_t t = t0;
    if (((knz_write_walk(blockBits, R.blocks.data(), k0, k1, t, t1, eW, pos, knz_write_walk_only) + tailBits + 7) >> 3) > dstCap) return tooSmall();
    t = t0;
    for (int64_t a = k0; a < k1 || (a == k0 && tailBits); a += PL) {
      const int cnt = (int)std::max<int64_t>(0, std::min<int64_t>(PL, k1 - a));
      const int64_t start = pos;
      pos = knz_write_walk(blockBits, R.blocks.data(), a, a + cnt, t, t1, eW + (t - t0), pos, [&](int64_t k, int64_t r, int64_t W, int64_t pay) {
        pc[k - a] = r >= 0 ? KnzPiece{pay, W, (int64_t)((intptr_t)(enc + (r - t0) * oS) - (intptr_t)d_src), (W + 7) >> 3, 0, 0}
                           : KnzPiece{pay, W, 0, n, blockBitOff[k], P.hdrEnd};
        if (newBitOff) { newBitOff[k] = pay; newBits[k] = W; }
      });
      const bool last = a + cnt >= k1;
      if (last) pos += tailBits;
      if (cnt) KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, pc, (size_t)cnt * sizeof(KnzPiece), hipMemcpyHostToDevice, ctx->stream));
      { const int rc = kz_knz_splice_launch(ctx, d_src, (const KnzPiece*)(ctx->knzAux.p + 64), cnt, d_dst, start, pos); if (rc) return rc; }
      KZ_HIP(kz_stream_sync(ctx, ctx->stream));                    // the pinned table is the next launch's
      kz_ktimer_flush(ctx);
      if (last) break;
    }
    return 0;
  };
  // ---- chunks of touched blocks, ascending: the decode into rows blockSize apart, then patch, encode, copy ----
  const KnzTable T(ctx, cmax);
  std::vector<kz_block_result> res((size_t)cmax), eres((size_t)cmax);
  std::vector<int64_t> W((size_t)cmax), off((size_t)cmax), eW((size_t)cmax);
  std::vector<int32_t> lens((size_t)cmax);
  int64_t next = 0;                                               // the first block not yet in the new stream
  size_t li = 0;                                                  // the next patch launch of the plan
  for (int64_t b0 = 0, c = 0; b0 < nb; b0 += CH, c++) {
    const int cnt = (int)std::min<int64_t>(CH, nb - b0);
    const uint8_t* covered = &R.covered[(size_t)b0];
    knz_chunk_entries(&R.blocks[(size_t)b0], covered, cnt, blockBitOff, blockBits, off.data(), W.data());
    knz_write_covered(R, b0, cnt, blockByteOff, false, res.data());
    // (behind it the pinned table becomes the segments')
    { const int rc = knz_chunk_decode(ctx, T, d_src, n, P, off.data(), W.data(), &hdrs[(size_t)b0], covered, cnt, rows, blockSize, res.data()); if (rc) return rc; }
    knz_write_covered(R, b0, cnt, blockByteOff, true, res.data());
    { const int rc = knz_write_settle(R, c, CH, blockByteOff, nIndex, blockSize, res.data(), lens.data(), ctx->err, sizeof(ctx->err)); if (rc) return rc; }
    // ---- the patch: the chunk's segments into the rows ----
    for (; li + 1 < R.cuts.size() && R.cuts[li] < R.first[(size_t)c + 1]; li++) {   // (a launch's segments are of one chunk)
      const int64_t s0 = R.cuts[li], s1 = R.cuts[li + 1];
      const int ns = (int)(s1 - s0);
      if (ctx->sw.writeGather) {                                   // the yardstick: the same segments through the ragged copy, a workgroup column each
        KnzCopy* t = (KnzCopy*)(ctx->knzPin.p + 64);
        int64_t maxLen = 0;
        for (int i = 0; i < ns; i++) {
          const KnzWriteSeg& g = R.segs[(size_t)(s0 + i)];
          t[i] = KnzCopy{g.src, (int64_t)g.slot * blockSize + g.off, g.len};
          maxLen = std::max<int64_t>(maxLen, g.len);
        }
        KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, t, (size_t)ns * sizeof(KnzCopy), hipMemcpyHostToDevice, ctx->stream));
        { const int rc = kz_knz_gather(ctx, d_data, (const KnzCopy*)(ctx->knzAux.p + 64), ns, maxLen, rows); if (rc) return rc; }
      } else {
        memcpy(ctx->knzPin.p + 64, &R.segs[(size_t)s0], (size_t)ns * sizeof(KnzWriteSeg));
        KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, ctx->knzPin.p + 64, (size_t)ns * sizeof(KnzWriteSeg), hipMemcpyHostToDevice, ctx->stream));
        const int64_t u0 = R.segs[(size_t)s0].unit0, uEnd = s1 < R.first[(size_t)c + 1] ? R.segs[(size_t)s1].unit0 : R.units[(size_t)c];
        const int rc = kz_knz_write(ctx, d_data, dataLen, (const KnzWriteSeg*)(ctx->knzAux.p + 64), ns, rows, blockSize, u0, uEnd - u0);
        if (rc) return rc;
      }
      KZ_HIP(kz_stream_sync(ctx, ctx->stream));                    // the pinned table is the next launch's; the encoder takes its input to be complete
      kz_ktimer_flush(ctx);
    }
    // ---- one batched encode of the chunk's rows, with the chain of the stream's header ----
    {
      int rc = kz_encode_blocks_pre(ctx, h.transformType, (uint32_t)h.entropyType, blockSize, rows, blockSize, lens.data(), cnt, enc, oS, eres.data(), KZ_MEM_DEVICE, nullptr);
      if (!rc) rc = knz_recoded_bits(ctx, &R.blocks[(size_t)b0], eres.data(), cnt, eW.data());
      if (rc) return rc;
    }
    // ---- the copy: every kept block since the previous chunk, and the chunk's recoded ones, behind the previous chunk's last bit ----
    const int64_t k1 = (int64_t)R.blocks[(size_t)(b0 + cnt - 1)] + 1;
    { const int64_t rc = emit(next, k1, b0, b0 + cnt, eW.data(), 0); if (rc) return rc; }
    next = k1;
  }
  // ---- the kept tail and the end marker (:491-492) ----
  { const int64_t rc = emit(next, nIndex, nb, nb, nullptr, 8); if (rc) return rc; }
  { const int hrc = knz_put_header(ctx, nh, (int64_t)(hb.pos >> 3), d_dst); if (hrc) return hrc; }
  KZ_HIP(kz_stream_sync(ctx, ctx->stream));
  kz_ktimer_flush(ctx);
  return (pos + 7) >> 3;
}



// =================================================================================================
// kz_write_bytes_device for ranges of N streams in one call (kz_write_bytes_many_device).  The open is the many-stream read's (k_knz_heads
// over the streams that some range names, one copy, parsed here); per stream the single call's table check and its plan (knz_write_plan_at:
// a stream's ranges are not side by side in the packed data); the merged plan is knz_write_many_plan (kz_knz_host.h: the touched blocks of
// all streams in one list of rows by header group, stream and block, cut into chunks inside a group).  Every entry the call uses, the
// kept blocks' and the decoded ones', is checked against its own stream (k_knz_check_rows) before anything is unpacked.  A chunk is the
// indexed calls' decode step over rows of many streams (k_knz_unpack_many), the settle per stream, the patch (k_knz_write), one batched
// encode under the group's header, and the emit: ONE k_knz_splice_many launch per bounded number of pieces that writes, for every
// stream with rows in the chunk, every kept block since that stream's last emitted one together with its recoded blocks behind that
// stream's last bit -- with the stream header in front when it is the stream's first emission, and with the kept tail and the end marker
// when the stream's last touched block is in the chunk.  A named stream with no touched block is a whole copy that rides in the first
// emit launch with room for it.  A fault that ends the single-stream call ends only its stream here: its rows are carried through the
// chunk's decode and then ignored, in later chunks they are left out.
namespace {
// The emit launches of the call: spans and pieces collect in the pinned tables (spans at 64, pieces behind cap spans) until either
// count reaches cap, or the caller flushes because the encoder rows that pieces name are about to be written again.
struct KnzEmit {
  kz_ctx* ctx; const uint8_t* d_src; uint8_t* d_dst; int cap;
  int nsp = 0, npc = 0; int64_t units = 0; bool open = false;
  KnzSpan* sp() const { return (KnzSpan*)(ctx->knzPin.p + 64); }
  size_t pcAt() const { return 64 + kz_align((size_t)cap * sizeof(KnzSpan), 64); }
  KnzPiece* pc() const { return (KnzPiece*)(ctx->knzPin.p + pcAt()); }
  static size_t bytes(int cap) { return kz_align((size_t)cap * sizeof(KnzSpan), 64) + (size_t)cap * sizeof(KnzPiece); }
  int room() const { return cap - npc; }
  int flush() {
    if (nsp == 0) return 0;
    KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, sp(), (size_t)nsp * sizeof(KnzSpan), hipMemcpyHostToDevice, ctx->stream));
    if (npc) KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + pcAt(), pc(), (size_t)npc * sizeof(KnzPiece), hipMemcpyHostToDevice, ctx->stream));
    { const int rc = kz_knz_splice_many(ctx, d_src, (const KnzSpan*)(ctx->knzAux.p + 64), nsp, (const KnzPiece*)(ctx->knzAux.p + pcAt()), d_dst, units); if (rc) return rc; }
    KZ_HIP(kz_stream_sync(ctx, ctx->stream));                      // the pinned tables are the next launch's
    kz_ktimer_flush(ctx);
    nsp = npc = 0; units = 0;
    return 0;
  }
  void begin(int64_t dst, int64_t startBit, const uint8_t* hdr, int hdrBytes) {
    KnzSpan& g = sp()[nsp];
    memset(&g, 0, sizeof(g));
    g.dst = dst; g.startBit = startBit; g.unit0 = units; g.piece0 = npc; g.hdrBytes = hdrBytes;
    if (hdrBytes) memcpy(g.hdr, hdr, (size_t)hdrBytes);
    open = true;
  }
  // the open span ends at endBit; a span of no bits is dropped
  int end(int64_t endBit) {
    KnzSpan& g = sp()[nsp];
    open = false;
    if (endBit <= g.startBit) { npc = g.piece0; return 0; }
    g.endBit = endBit;
    const uintptr_t a = (uintptr_t)d_dst + (uintptr_t)g.dst;
    units += (int64_t)((a + (uintptr_t)((endBit + 7) >> 3) - ((a + (uintptr_t)(g.startBit >> 3)) & ~(uintptr_t)15) + 15) >> 4);
    nsp++;
    return nsp == cap ? flush() : 0;
  }
  // a piece of the open span whose prefix starts at bit `at`: when the launch is full the span ends there and goes on in the next one
  int piece(int64_t at, const KnzPiece& p) {
    if (npc == cap) {
      const int64_t dst = sp()[nsp].dst;
      { int rc = end(at); if (!rc) rc = flush(); if (rc) return rc; }
      begin(dst, at, nullptr, 0);
    }
    pc()[npc++] = p;
    sp()[nsp].npieces++;
    return 0;
  }
};
}  // namespace

extern "C" int64_t kz_write_bytes_many_bound(const int64_t* indexFirst, const int64_t* blockBits, const int32_t* blockSize, int32_t nStreams, int64_t* slotCap) {
  return knz_write_many_bound(indexFirst, blockBits, blockSize, nStreams, slotCap);
}

extern "C" int32_t kz_write_bytes_many_device(kz_ctx* ctx, const uint8_t* d_src, const int64_t* srcOff, const int64_t* srcLen, int32_t nStreams,
                                              const int64_t* indexFirst, const int64_t* blockBitOff, const int64_t* blockBits,
                                              const int64_t* tableFirst, const int64_t* blockByteOff,
                                              const int32_t* rangeStream, const int64_t* rangeOff, const int64_t* rangeLen, int32_t nRanges,
                                              const uint8_t* d_data, int64_t dataLen,
                                              uint8_t* d_dst, const int64_t* dstOff, const int64_t* dstCap, int64_t* dstLen,
                                              int64_t* newBitOff, int64_t* newBits) {
  if (!ctx) return -KZ_ERR_INVALID_PARAM;
  {
    const int rc = knz_write_many_args(d_src, srcOff, srcLen, nStreams, indexFirst, blockBitOff, blockBits, tableFirst, blockByteOff, rangeStream, rangeOff, rangeLen,
                                       nRanges, d_data, dataLen, d_dst, dstOff, dstCap, dstLen, newBitOff, newBits);
    if (rc) return rc;
  }
  const char* call = "kz_write_bytes_many_device";
  const int ns = nStreams;
  for (int s = 0; s < ns; s++) dstLen[s] = 0;
  if (nRanges == 0) return 0;
  KZ_HIP(hipSetDevice(ctx->device));
  // ---- the streams that some range names, ascending, and each one's ranges in call order with their places in the packed data ----
  std::vector<int32_t> ids;
  std::vector<int64_t> rFirst((size_t)ns + 1, 0), rOff((size_t)nRanges), rLen((size_t)nRanges), rData((size_t)nRanges);
  std::vector<int32_t> rId((size_t)nRanges);
  {
    for (int32_t i = 0; i < nRanges; i++) rFirst[(size_t)rangeStream[i] + 1]++;
    for (int s = 0; s < ns; s++) { if (rFirst[(size_t)s + 1]) ids.push_back(s); rFirst[(size_t)s + 1] += rFirst[(size_t)s]; }
    std::vector<int64_t> fill(rFirst.begin(), rFirst.end() - 1);
    int64_t D = 0;
    for (int32_t i = 0; i < nRanges; i++) {
      const int64_t at = fill[(size_t)rangeStream[i]]++;
      rOff[(size_t)at] = rangeOff[i]; rLen[(size_t)at] = rangeLen[i]; rData[(size_t)at] = D; rId[(size_t)at] = i;
      D += rangeLen[i];
    }
  }
  const int nn = (int)ids.size();
  // ---- their heads in one copy; per stream the single call's open, table check and plan ----
  KnzStreamFaults F(ns);
  std::vector<uint8_t> use((size_t)ns, 0);
  std::vector<KnzPlan> plan((size_t)ns);
  std::vector<KnzWritePlan> wp((size_t)ns);
  std::vector<const int64_t*> tab((size_t)ns, nullptr);
  std::vector<int32_t> nIdx((size_t)ns, 0);
  {
    const size_t tBytes = kz_align((size_t)nn * sizeof(KnzSrc), 64);
    { const int rc = knz_tables(ctx, tBytes + (size_t)nn * 32); if (rc) return rc; }
    { const int rc = knz_many_heads(ctx, d_src, srcOff, srcLen, ids.data(), nn, tBytes); if (rc) return rc; }
    for (int k = 0; k < nn; k++) {
      const int s = ids[(size_t)k];
      HostBitsIn bs{ctx->knzPin.p + tBytes + (size_t)k * 32, (uint64_t)std::min<int64_t>(srcLen[s], 26) * 8, 0, false};
      KnzHeader h;
      char why[96] = "";
      const int hrc = read_stream_header(bs, h, why, sizeof(why));
      if (hrc) { F.fail(s, hrc, call, why[0] ? why : "not a stream header"); continue; }
      plan[(size_t)s] = knz_plan(ctx, h, srcLen[s], (int64_t)bs.pos);
      nIdx[(size_t)s] = (int32_t)(indexFirst[s + 1] - indexFirst[s]);
      tab[(size_t)s] = (tableFirst && tableFirst[s] >= 0) ? blockByteOff + tableFirst[s] : nullptr;
      if (knz_read_table(tab[(size_t)s], nIdx[(size_t)s], h.blockSize)) { F.fail(s, -KZ_ERR_INVALID_PARAM, call, "blockByteOff is not a table of block starts"); continue; }
      const int64_t a = rFirst[(size_t)s];
      const int32_t bad = knz_write_plan_at(tab[(size_t)s], nIdx[(size_t)s], h.blockSize, &rOff[(size_t)a], &rLen[(size_t)a], &rData[(size_t)a],
                                            (int32_t)(rFirst[(size_t)s + 1] - a), 0x7FFFFFFF, INT64_MAX, wp[(size_t)s]);
      if (bad >= 0) { snprintf(why, sizeof(why), "range %d ends behind the data", (int)rId[(size_t)(a + bad)]); F.fail(s, -KZ_ERR_INVALID_PARAM, call, why); continue; }
      use[(size_t)s] = 1;
    }
  }
  auto finish = [&]() -> int32_t {
    for (int s = 0; s < ns; s++) if (F.code[(size_t)s]) dstLen[s] = F.code[(size_t)s];
    F.tell(ctx);
    return 0;
  };
  // ---- the merged plan, and every entry it uses against its own stream before anything is unpacked: the kept blocks' and the decoded
  //      ones'; a wholly covered block's is not looked at.  A stream with an entry that does not match leaves the plan, which is then
  //      made again without it (and checked again: the rows have other places) ----
  std::vector<KnzManyWriteIn> st((size_t)ns);
  KnzManyWritePlan R;
  std::vector<KnzPlan> groups;                                     // a group's plan: its first stream's (the header's four fields, the staging row)
  std::vector<int> chunkBlocks;
  std::vector<uint64_t> hdrs;
  for (;;) {
    groups.clear(); chunkBlocks.clear();
    int64_t entries = 0;
    for (int s = 0; s < ns; s++) {
      st[(size_t)s] = KnzManyWriteIn{use[(size_t)s] != 0, -1, &wp[(size_t)s], rId.data() + rFirst[(size_t)s]};
      if (!use[(size_t)s]) continue;
      const KnzHeader& h = plan[(size_t)s].h;
      size_t g = 0;
      for (; g < groups.size(); g++) if (groups[g].h.transformType == h.transformType && groups[g].h.entropyType == h.entropyType && groups[g].h.blockSize == h.blockSize && groups[g].h.chkKind == h.chkKind) break;
      if (g == groups.size()) { groups.push_back(plan[(size_t)s]); chunkBlocks.push_back(knz_chunk_blocks(ctx, h.blockSize)); }
      st[(size_t)s].group = (int32_t)g;
      entries += nIdx[(size_t)s];
    }
    knz_write_many_plan(st.data(), ns, chunkBlocks.data(), KNZ_WRITE_LAUNCH, R);
    const int64_t nr = (int64_t)R.rowStream.size();
    hdrs.assign((size_t)nr, 0);
    if (entries == 0) break;
    std::vector<int64_t> rowOf((size_t)ns, -1);                    // a stream's first row
    for (int64_t r = nr - 1; r >= 0; r--) rowOf[(size_t)R.rowStream[(size_t)r]] = r;
    const int CK = (int)std::min<int64_t>(KNZ_CHECK_LAUNCH, entries);
    const size_t rowBytes = kz_align((size_t)CK * sizeof(KnzCheckRow), 64);
    { const int rc = knz_tables(ctx, rowBytes + (size_t)CK * 16); if (rc) return rc; }
    struct Entry { int32_t s, k; int64_t row; };
    std::vector<Entry> ent((size_t)CK);
    bool dropped = false;
    int kn = 0;                                                    // the stream (among ids) and the block of the next entry
    int64_t kk = 0, tr = -1;                                       // tr: that stream's next touched row, -1 before its first entry
    for (;;) {
      int cnt = 0;
      KnzCheckRow* t = (KnzCheckRow*)ctx->knzPin.p;
      while (cnt < CK && kn < nn) {
        const int s = ids[(size_t)kn];
        if (!use[(size_t)s] || kk >= nIdx[(size_t)s]) { kn++; kk = 0; tr = -1; continue; }
        if (tr < 0) tr = rowOf[(size_t)s] >= 0 ? rowOf[(size_t)s] : nr;
        const bool touched = tr < nr && R.rowStream[(size_t)tr] == s && R.rowBlock[(size_t)tr] == kk;
        const int64_t row = touched ? tr++ : -1;
        if (!(touched && R.rowCovered[(size_t)row])) {
          const int64_t e = indexFirst[s] + kk;
          t[cnt] = KnzCheckRow{srcOff[s], srcLen[s], blockBitOff[e], blockBits[e], plan[(size_t)s].hdrEnd};
          ent[(size_t)cnt++] = Entry{s, (int32_t)kk, row};
        }
        kk++;
      }
      if (cnt == 0) break;
      uint64_t* d_hdr = (uint64_t*)(ctx->knzAux.p + rowBytes);
      KZ_HIP(hipMemcpyAsync(ctx->knzAux.p, t, (size_t)cnt * sizeof(KnzCheckRow), hipMemcpyHostToDevice, ctx->stream));
      { const int rc = kz_knz_check_rows(ctx, d_src, (const KnzCheckRow*)ctx->knzAux.p, cnt, d_hdr, (int64_t*)(d_hdr + CK)); if (rc) return rc; }
      KZ_HIP(hipMemcpyAsync(ctx->knzPin.p + rowBytes, ctx->knzAux.p + rowBytes, (size_t)CK * 8 + (size_t)cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
      KZ_HIP(kz_stream_sync(ctx, ctx->stream));                    // the pinned table is the next launch's
      kz_ktimer_flush(ctx);
      const uint64_t* hw = (const uint64_t*)(ctx->knzPin.p + rowBytes);
      const int64_t* bad = (const int64_t*)(hw + CK);
      for (int i = 0; i < cnt; i++) {
        const Entry& e = ent[(size_t)i];
        if (e.row >= 0) hdrs[(size_t)e.row] = hw[i];
        if (!bad[i] || !use[(size_t)e.s]) continue;                // (of a stream's bad entries the first in block order is named)
        char why[96];
        snprintf(why, sizeof(why), "index entry %d does not match the stream", (int)e.k);
        F.fail(e.s, -KZ_ERR_INVALID_PARAM, call, why);
        use[(size_t)e.s] = 0;
        dropped = true;
      }
    }
    if (!dropped) break;
  }
  const int64_t nChunks = (int64_t)R.chunkGroup.size();
  if (groups.empty()) return finish();
  // ---- staging and tables for the largest chunk; PL = the pieces and the spans of an emit launch: the splice's chunk ----
  int cmax = 1, PL = 1;
  int64_t segMax = 0;
  size_t inMax = 0, outMax = 0, encMax = 0;
  for (size_t g = 0; g < groups.size(); g++) PL = std::max(PL, chunkBlocks[g]);
  for (int64_t c = 0; c < nChunks; c++) {
    const int cnt = (int)(R.chunkRow[(size_t)c + 1] - R.chunkRow[(size_t)c]);
    const KnzPlan& G = groups[(size_t)R.chunkGroup[(size_t)c]];
    cmax = std::max(cmax, cnt);
    inMax = std::max(inMax, (size_t)cnt * (size_t)G.iS);
    outMax = std::max(outMax, (size_t)cnt * (size_t)G.h.blockSize);
    encMax = std::max(encMax, (size_t)cnt * (size_t)kz_max_block_stream_bytes(G.h.blockSize));
  }
  for (size_t l = 0; l + 1 < R.cuts.size(); l++) segMax = std::max(segMax, R.cuts[l + 1] - R.cuts[l]);
  {
    int rc = kz_stage_reserve(ctx, ctx->devIn[0], std::max<size_t>(inMax, 64), false);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->devOut[0], std::max<size_t>(outMax, 64), false);
    if (!rc) rc = kz_stage_reserve(ctx, ctx->devOut[1], std::max<size_t>(encMax, 64), false);
    if (!rc) rc = knz_tables(ctx, std::max(std::max((size_t)cmax * sizeof(KnzRow), (size_t)segMax * std::max(sizeof(KnzWriteSeg), sizeof(KnzCopy))), KnzEmit::bytes(PL)));
    if (rc) return rc;
  }
  uint8_t* rows = ctx->devOut[0].p;
  uint8_t* enc = ctx->devOut[1].p;
  if ((uintptr_t)rows & 15) { snprintf(ctx->err, sizeof(ctx->err), "%s: staging rows off a 16-byte boundary", call); return -KZ_ERR_DEVICE; }   // (unit0 counts on it)
  // ---- what every written stream has in the new stream so far ----
  std::vector<int64_t> pos((size_t)ns, 0), nextBlk((size_t)ns, 0), tDone((size_t)ns, 0);
  std::vector<uint8_t> started((size_t)ns, 0);
  KnzEmit E{ctx, d_src, d_dst, PL};
  // Blocks [nextBlk[s], k1) of stream s behind its last bit, then tailBits zero bits: the blocks of the chunk's rows [i, j) (r0: the
  // chunk's first row; eW: their bits) come from the encoder's rows oS apart, all others from where they lie in the stream.  The room
  // is decided from the bit arithmetic before anything of it enters a launch.
  auto emit = [&](int s, int64_t k1, int64_t r0, int i, int j, const int64_t* eW, int64_t oS, int tailBits) -> int {
    const int64_t e0 = indexFirst[s];
    uint8_t nh[32];
    int64_t p = pos[(size_t)s];
    int hdrBytes = 0;
    if (!started[(size_t)s]) {                                     // the new stream's header: the old one's parameters and size
      const KnzHeader& h = plan[(size_t)s].h;
      HostBits hb{nh, 32, 0, false};
      write_stream_header(hb, h.transformType, (uint32_t)h.entropyType, h.blockSize, h.inputSize, h.chkKind);
      p = (int64_t)hb.pos;
      hdrBytes = (int)(hb.pos >> 3);
    }
    int64_t q = p;
    { int t = i; for (int64_t k = nextBlk[(size_t)s]; k < k1; k++) { const bool rec = t < j && R.rowBlock[(size_t)(r0 + t)] == k; const int64_t W = rec ? eW[t++] : blockBits[e0 + k]; q += 5 + knz_prefix_width((uint64_t)W) + W; } }
    if (((q + tailBits + 7) >> 3) > dstCap[s]) { F.fail(s, -KZ_ERR_WRITE_FILE, call, "destination too small"); return 0; }
    E.begin(dstOff[s], started[(size_t)s] ? p : 0, nh, hdrBytes);
    int t = i;
    for (int64_t k = nextBlk[(size_t)s]; k < k1; k++) {
      const bool rec = t < j && R.rowBlock[(size_t)(r0 + t)] == k;
      const int64_t W = rec ? eW[t] : blockBits[e0 + k];
      const int64_t pay = p + 5 + knz_prefix_width((uint64_t)W);
      const int rc = E.piece(p, rec ? KnzPiece{pay, W, (int64_t)((intptr_t)(enc + (int64_t)t * oS) - (intptr_t)d_src), (W + 7) >> 3, 0, 0}
                                    : KnzPiece{pay, W, srcOff[s], srcLen[s], blockBitOff[e0 + k], plan[(size_t)s].hdrEnd});
      if (rc) return rc;
      if (newBitOff) { newBitOff[e0 + k] = pay; newBits[e0 + k] = W; }
      if (rec) t++;
      p = pay + W;
    }
    p += tailBits;
    started[(size_t)s] = 1; pos[(size_t)s] = p; nextBlk[(size_t)s] = k1;
    return E.end(p);
  };
  // the named streams with no touched block, ascending: whole copies
  std::vector<int32_t> copies;
  for (int k = 0; k < nn; k++) if (use[(size_t)ids[(size_t)k]] && wp[(size_t)ids[(size_t)k]].blocks.empty()) copies.push_back(ids[(size_t)k]);
  size_t nextCopy = 0;
  // ---- chunks: decode under the group's header, settle per stream, patch, encode, emit ----
  ChecksumScope chk(ctx, ctx->checksum);                           // each chunk runs under its own group's kind and block size
  BlockSizeScope scope(ctx, ctx->blockSize);
  std::vector<kz_block_result> res((size_t)cmax), eres((size_t)cmax);
  std::vector<int64_t> W((size_t)cmax), off((size_t)cmax), eW((size_t)cmax);
  std::vector<int32_t> lens((size_t)cmax);
  std::vector<uint8_t> leftOut((size_t)cmax);
  size_t li = 0;                                                  // the next patch launch of the plan
  for (int64_t c = 0; c < nChunks; c++) {
    const int64_t r0 = R.chunkRow[(size_t)c];
    const int cnt = (int)(R.chunkRow[(size_t)c + 1] - r0);
    const KnzPlan& G = groups[(size_t)R.chunkGroup[(size_t)c]];
    const KnzHeader& h = G.h;
    const int32_t blockSize = h.blockSize;
    const int64_t oS = kz_max_block_stream_bytes(blockSize);
    ctx->checksum = h.chkKind;
    ctx->blockSize = blockSize; ctx->blockSizeSet = true;
    for (int i = 0; i < cnt; i++) {
      const int s = R.rowStream[(size_t)(r0 + i)];
      const int64_t e = indexFirst[s] + R.rowBlock[(size_t)(r0 + i)];
      leftOut[(size_t)i] = (R.rowCovered[(size_t)(r0 + i)] || F.code[(size_t)s]) ? 1 : 0;   // a failed stream's rows are left out from here on
      off[(size_t)i] = leftOut[(size_t)i] ? 0 : blockBitOff[e]; W[(size_t)i] = leftOut[(size_t)i] ? 0 : blockBits[e];
      memset(&res[(size_t)i], 0, sizeof(res[0]));
      res[(size_t)i].status = 1;
    }
    KnzRow* t = (KnzRow*)(ctx->knzPin.p + 64);
    // (behind it the pinned table becomes the segments')
    {
      const int rc = knz_chunk_decode_rows(ctx, G, [&](int i) { return srcLen[R.rowStream[(size_t)(r0 + i)]]; }, off.data(), W.data(), &hdrs[(size_t)r0], leftOut.data(), cnt,
        [&](int i, int64_t o, int64_t bits) { const int s = R.rowStream[(size_t)(r0 + i)]; t[i] = KnzRow{srcOff[s], srcLen[s], o, bits, (int64_t)i * G.iS}; },
        [&](int64_t maxBytes) -> int {
          KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, t, (size_t)cnt * sizeof(KnzRow), hipMemcpyHostToDevice, ctx->stream));
          return kz_knz_unpack_many(ctx, d_src, (const KnzRow*)(ctx->knzAux.p + 64), cnt, maxBytes, ctx->devIn[0].p);
        }, rows, blockSize, res.data());
      if (rc) return rc;
    }
    // ---- the settle: a wholly covered block counts as decoded to the table's length; per stream the length check of every block in
    //      block order and, without a table, the segments against the real end of a short last block ----
    for (int i = 0; i < cnt; i++) {
      const int s = R.rowStream[(size_t)(r0 + i)];
      const int32_t k = R.rowBlock[(size_t)(r0 + i)];
      lens[(size_t)i] = 0;
      if (F.code[(size_t)s]) continue;
      if (R.rowCovered[(size_t)(r0 + i)]) { res[(size_t)i].status = 0; res[(size_t)i].length = (int32_t)(tab[(size_t)s][k + 1] - tab[(size_t)s][k]); }
      const char* why = "its decode failed";
      if (!res[(size_t)i].status) {
        res[(size_t)i].status = knz_block_len_check(tab[(size_t)s], nIdx[(size_t)s], blockSize, k, res[(size_t)i].length);
        why = res[(size_t)i].status == -KZ_ERR_PROCESS_BLOCK ? "decodes to more than the block size" : "decodes to another length than its place in the data";
      }
      if (res[(size_t)i].status) {
        char text[128];
        snprintf(text, sizeof(text), "block %d: %s", (int)k, why);
        F.fail(s, res[(size_t)i].status, call, text);
        continue;
      }
      lens[(size_t)i] = res[(size_t)i].length;
    }
    for (int64_t q = R.first[(size_t)c]; q < R.first[(size_t)c + 1]; q++) {
      const KnzWriteSeg& g = R.segs[(size_t)q];
      const int s = R.rowStream[(size_t)(r0 + g.slot)];
      if (F.code[(size_t)s] || tab[(size_t)s] || (int64_t)g.off + g.len <= lens[(size_t)g.slot]) continue;
      char text[96];
      snprintf(text, sizeof(text), "range %d ends behind the data", (int)g.range);
      F.fail(s, -KZ_ERR_INVALID_PARAM, call, text);
    }
    // ---- the patch: the chunk's segments into the rows (a failed stream's land in rows that nobody reads) ----
    for (; li + 1 < R.cuts.size() && R.cuts[li] < R.first[(size_t)c + 1]; li++) {   // (a launch's segments are of one chunk)
      const int64_t s0 = R.cuts[li], s1 = R.cuts[li + 1];
      const int nseg = (int)(s1 - s0);
      if (ctx->sw.writeGather) {                                   // the yardstick: the same segments through the ragged copy, a workgroup column each
        KnzCopy* ct = (KnzCopy*)(ctx->knzPin.p + 64);
        int64_t maxLen = 0;
        for (int i = 0; i < nseg; i++) {
          const KnzWriteSeg& g = R.segs[(size_t)(s0 + i)];
          ct[i] = KnzCopy{g.src, (int64_t)g.slot * blockSize + g.off, g.len};
          maxLen = std::max<int64_t>(maxLen, g.len);
        }
        KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, ct, (size_t)nseg * sizeof(KnzCopy), hipMemcpyHostToDevice, ctx->stream));
        { const int rc = kz_knz_gather(ctx, d_data, (const KnzCopy*)(ctx->knzAux.p + 64), nseg, maxLen, rows); if (rc) return rc; }
      } else {
        memcpy(ctx->knzPin.p + 64, &R.segs[(size_t)s0], (size_t)nseg * sizeof(KnzWriteSeg));
        KZ_HIP(hipMemcpyAsync(ctx->knzAux.p + 64, ctx->knzPin.p + 64, (size_t)nseg * sizeof(KnzWriteSeg), hipMemcpyHostToDevice, ctx->stream));
        const int64_t u0 = R.segs[(size_t)s0].unit0, uEnd = s1 < R.first[(size_t)c + 1] ? R.segs[(size_t)s1].unit0 : R.units[(size_t)c];
        const int rc = kz_knz_write(ctx, d_data, dataLen, (const KnzWriteSeg*)(ctx->knzAux.p + 64), nseg, rows, blockSize, u0, uEnd - u0);
        if (rc) return rc;
      }
      KZ_HIP(kz_stream_sync(ctx, ctx->stream));                    // the pinned table is the next launch's; the encoder takes its input to be complete
      kz_ktimer_flush(ctx);
    }
    // ---- one batched encode of the chunk's rows with the chain of the group's header; the rows of failed streams are left out of
    //      it, so what stands side by side goes in one call ----
    for (int i = 0; i < cnt;) {
      if (F.code[(size_t)R.rowStream[(size_t)(r0 + i)]]) { i++; continue; }
      int j = i + 1;
      while (j < cnt && !F.code[(size_t)R.rowStream[(size_t)(r0 + j)]]) j++;
      const int rc = kz_encode_blocks_pre(ctx, h.transformType, (uint32_t)h.entropyType, blockSize, rows + (int64_t)i * blockSize, blockSize, lens.data() + i, j - i,
                                          enc + (int64_t)i * oS, oS, eres.data() + i, KZ_MEM_DEVICE, nullptr);
      if (rc) return rc;
      i = j;
    }
    for (int i = 0; i < cnt; i++) {
      const int s = R.rowStream[(size_t)(r0 + i)];
      if (F.code[(size_t)s]) continue;
      if (eres[(size_t)i].status || eres[(size_t)i].bits <= 0) {
        char text[96];
        snprintf(text, sizeof(text), "block %d: its encode failed", (int)R.rowBlock[(size_t)(r0 + i)]);
        F.fail(s, eres[(size_t)i].status ? eres[(size_t)i].status : -KZ_ERR_PROCESS_BLOCK, call, text);
        continue;
      }
      eW[(size_t)i] = eres[(size_t)i].bits;
    }
    // ---- the emit: per stream with rows here every kept block since its last emitted one and its recoded ones; with the stream's last
    //      touched block also its kept tail and the end marker (:491-492).  Whole copies ride along while the launch has room ----
    for (int i = 0; i < cnt;) {                                    // the rows of a stream lie side by side
      const int s = R.rowStream[(size_t)(r0 + i)];
      int j = i + 1;
      while (j < cnt && R.rowStream[(size_t)(r0 + j)] == s) j++;
      if (!F.code[(size_t)s]) {
        const bool last = tDone[(size_t)s] + (j - i) == (int64_t)wp[(size_t)s].blocks.size();
        const int64_t k1 = last ? nIdx[(size_t)s] : (int64_t)R.rowBlock[(size_t)(r0 + j - 1)] + 1;
        const int rc = emit(s, k1, r0, i, j, eW.data(), oS, last ? 8 : 0);
        if (rc) return rc;
        tDone[(size_t)s] += j - i;
      }
      i = j;
    }
    for (; nextCopy < copies.size() && E.nsp > 0 && E.nsp < E.cap && nIdx[(size_t)copies[nextCopy]] <= E.room(); nextCopy++) {
      const int s = copies[nextCopy];
      const int rc = emit(s, nIdx[(size_t)s], 0, 0, 0, nullptr, 0, 8);
      if (rc) return rc;
    }
    { const int rc = E.flush(); if (rc) return rc; }               // the encoder's rows are the next chunk's
  }
  // ---- the whole copies that found no room ----
  for (; nextCopy < copies.size(); nextCopy++) {
    const int s = copies[nextCopy];
    const int rc = emit(s, nIdx[(size_t)s], 0, 0, 0, nullptr, 0, 8);
    if (rc) return rc;
  }
  { const int rc = E.flush(); if (rc) return rc; }
  for (int k = 0; k < nn; k++) {
    const int s = ids[(size_t)k];
    if (!F.code[(size_t)s]) dstLen[s] = (pos[(size_t)s] + 7) >> 3;
  }
  return finish();
}
