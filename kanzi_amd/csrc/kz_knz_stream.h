// kz_knz_stream.h -- what the host-buffer stream calls (kz_stream.hip) and the device-buffer ones (kz_stream_device.hip) share
// beyond the host-only core: batch and chunk sizes, the plan of a reading call, the scopes over the context's per-stream entries, and
// the host arithmetic of the calls that read a stream by a caller's index.
#pragma once
#include "kz_internal.h"
#include "kz_knz_host.h"

// blocks per kz_encode_blocks / kz_decode_blocks call of the host-buffer entry points: 8 GiB of input per call
// (device scratch is bounded separately by the arena budget, which splits a call into sub-batches); the
// serial kernels want a thousand blocks or more in flight.  The strided host staging buffers are allocated
// uninitialised, so only the bytes actually produced/consumed are ever touched.
static inline int batch_blocks(int blockSize) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (8LL << 30) / blockSize)); }
// blocks per pipeline step of kz_compress: about 1 GiB of input
static inline int stream_chunk_blocks(const kz_ctx* ctx, int blockSize) {
  if (ctx->sw.streamChunk > 0) return ctx->sw.streamChunk;
  return (int)std::max<int64_t>(8, std::min<int64_t>(2048, (1LL << 30) / blockSize));
}
// blocks per step of the device writers and of the indexed reads: the writer's chunk, one launch's rows at the most.  (Not the
// decoder's chunk, KnzPlan::CH, which is cut from the decoder's batch.)
static inline int knz_chunk_blocks(const kz_ctx* ctx, int blockSize) { return std::min(stream_chunk_blocks(ctx, blockSize), KZ_MAX_BATCH); }

// The plan of a call that reads a stream of n bytes whose header h ends at bit hdrEnd.  NB is kz_decompress's batch: 8 GiB of blocks,
// 2048 at the most, and no more than the stream can need (declared size if present, else >= 8 bytes of stream per block).  CH is the
// device reader's chunk inside a batch: the whole batch (the decoder's serial per-block chains want that many blocks in flight: in
// chunks of the writer's size a 2048 x 4 MiB stream decodes at a quarter of the speed), one launch's rows at the most,
// or KZ_STREAM_CHUNK blocks (the tests' seams).
static inline KnzPlan knz_plan(const kz_ctx* ctx, const KnzHeader& h, int64_t n, int64_t hdrEnd) {
  KnzPlan P;
  P.h = h;
  P.nbFunctions = knz_nb_functions(h.transformType);
  P.iS = knz_dec_row_stride(h.blockSize);
  P.NB = batch_blocks(h.blockSize);
  if (h.szMask && h.inputSize > 0) P.NB = std::min<int64_t>(P.NB, (h.inputSize + h.blockSize - 1) / h.blockSize);
  else P.NB = std::min<int64_t>(P.NB, n / 8 + 1);
  P.CH = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->sw.streamChunk > 0 ? ctx->sw.streamChunk : P.NB, std::min<int64_t>(P.NB, KZ_MAX_BATCH)));
  P.hdrEnd = hdrEnd;
  return P;
}

struct BlockSizeScope {                                            // the context's "blockSize" entry = this stream's (TEXT reads it)
  kz_ctx* c; int saved; bool savedSet;
  BlockSizeScope(kz_ctx* c_, int v) : c(c_), saved(c_->blockSize), savedSet(c_->blockSizeSet) { c->blockSize = v; c->blockSizeSet = true; }
  ~BlockSizeScope() { c->blockSize = saved; c->blockSizeSet = savedSet; }
};
struct ChecksumScope {                                             // the context's checksum kind = this stream's, while its blocks are decoded
  kz_ctx* c; int saved;
  ChecksumScope(kz_ctx* c_, int v) : c(c_), saved(c_->checksum) { c->checksum = v; }
  ~ChecksumScope() { c->checksum = saved; }
};

// run fn(i) for i in [0, n) on the host pool (blocks are independent)
template <typename F>
static void parallel_blocks(int n, F fn, int maxThreads = 32) {
  struct Thunk { static void run(int i, void* a) { (*(F*)a)(i); } };
  kz_parallel_for(n, maxThreads, &Thunk::run, (void*)&fn);
}

// ---- the steps of the calls that read a stream of n bytes by a caller's index (the indexed read, the byte-addressed read and write),
//      as far as they are the same arithmetic for host and device memory; the rest is in kz_stream.hip and kz_stream_device.hip ----
// The open: the stream header from bs (a reader over the stream's first bytes) with its faults and texts, and the plan.
static inline int knz_open_plan(kz_ctx* ctx, HostBitsIn& bs, int64_t n, KnzPlan& P) {
  KnzHeader h;
  { const int hrc = read_stream_header(bs, h, ctx->err, sizeof(ctx->err)); if (hrc) return hrc; }
  P = knz_plan(ctx, h, n, (int64_t)bs.pos);
  return 0;
}
// the indexed read's, behind the open: a destination row that cannot hold a block
static inline int indexed_stride(kz_ctx* ctx, int64_t dstStride, const KnzPlan& P) {
  if (dstStride >= P.h.blockSize) return 0;
  snprintf(ctx->err, sizeof(ctx->err), "dstStride %lld is less than the stream's block size %d", (long long)dstStride, P.h.blockSize);
  return -KZ_ERR_INVALID_PARAM;
}
// the byte-addressed calls': a blockByteOff that is no table of block starts, refused in the name of the call
static inline int knz_table_refusal(kz_ctx* ctx, const char* call, const int64_t* blockByteOff, int32_t nIndex, int32_t blockSize) {
  if (!knz_read_table(blockByteOff, nIndex, blockSize)) return 0;
  snprintf(ctx->err, sizeof(ctx->err), "%s: blockByteOff is not a table of block starts", call);
  return -KZ_ERR_INVALID_PARAM;
}
// the byte-addressed calls': (off[i], W[i]) = the index entry of the chunk's block blk[i]; zeros for one that is left out of the
// decode (leftOut, may be null: the write's wholly covered blocks, whose entries are not looked at)
static inline void knz_chunk_entries(const int32_t* blk, const uint8_t* leftOut, int cnt, const int64_t* blockBitOff, const int64_t* blockBits, int64_t* off, int64_t* W) {
  for (int i = 0; i < cnt; i++) {
    const bool out = leftOut && leftOut[i];
    off[i] = out ? 0 : blockBitOff[blk[i]]; W[i] = out ? 0 : blockBits[blk[i]];
  }
}
// the byte-addressed write's: eW[i] = the bits of the chunk's recoded block blk[i], or the code and the text of the first whose
// encode failed
static inline int knz_recoded_bits(kz_ctx* ctx, const int32_t* blk, const kz_block_result* eres, int cnt, int64_t* eW) {
  for (int i = 0; i < cnt; i++) {
    if (eres[i].status || eres[i].bits <= 0) {
      snprintf(ctx->err, sizeof(ctx->err), "block %d: its encode failed (%d)", (int)blk[i], (int)eres[i].status);
      return eres[i].status ? eres[i].status : -KZ_ERR_PROCESS_BLOCK;
    }
    eW[i] = eres[i].bits;
  }
  return 0;
}
static inline int indexed_mismatch(kz_ctx* ctx, int64_t i) {
  snprintf(ctx->err, sizeof(ctx->err), "index entry %lld does not match the stream", (long long)i);
  return -KZ_ERR_INVALID_PARAM;
}
// Decode the chunk's entries that passed their prechecks (res[i].status == 0 on entry), rows `P.iS` apart at `rows`, into out rows
// `dstStride` apart: one kz_decode_blocks call per run of neighbours, so that every block lands in its own row.
static inline int indexed_decode_runs(kz_ctx* ctx, const KnzPlan& P, const uint8_t* rows, const int64_t* W, int cnt, uint8_t* out, int64_t dstStride,
                                      kz_block_result* res, int memKind) {
  for (int i = 0; i < cnt;) {
    if (res[i].status) { i++; continue; }
    int j = i + 1;
    while (j < cnt && !res[j].status) j++;
    const int rc = kz_decode_blocks(ctx, P.h.transformType, (uint32_t)P.h.entropyType, P.h.blockSize, rows + (int64_t)i * P.iS, P.iS, W + i, j - i,
                                    out + (int64_t)i * dstStride, dstStride, res + i, memKind);
    if (rc) return rc;
    i = j;
  }
  return 0;
}
